"""CPU suite of the wide form of the polar SC decoder: the host walk of its memory plan (qldpc_polar_decode_wide_host) against the host mirror and
the numpy restatement of tests/polar_ref.py bit for bit, the layout of qldpc_polar_wide_core.h, the refusals of qldpc_polar_create_form, and the
sanitizer program.  No GPU, no device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import polar_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qcrypto-ldpc_amd", "csrc")
MAXQ = (1, 31, 126)


def _same(a, b, what):
    assert set(a) == set(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, what + ": " + k
        assert np.array_equal(a[k].view(np.uint32 if a[k].dtype == np.float32 else a[k].dtype), b[k].view(np.uint32 if b[k].dtype == np.float32 else b[k].dtype)), what + ": " + k


@pytest.mark.parametrize("messages", ["i8", "f32"])
@pytest.mark.parametrize("n", range(1, 15))
def test_walk_is_the_mirror(q, n, messages):
    """u, info, x and leaf, floats by bit pattern, with and without frozen values; at n = 6, 9 and 12 the restatement too"""
    rng = np.random.default_rng([n, messages == "i8", 31])
    N, F, maxq = 1 << n, 3, MAXQ[n % 3]
    pos, mask = R.random_code(rng, N)
    llr = R.i8_inputs(rng, F, N, maxq) if messages == "i8" else R.f32_inputs(rng, F, N)
    fv = rng.integers(0, 2, (F, N), dtype=np.uint8)
    for values in (None, fv):
        fz = None if values is None else R.pack(values)
        walk = q.polar_decode_wide_host(n, pos, llr, fz, messages, maxq, leaf=True)
        _same(walk, q.polar_decode_host(n, pos, llr, fz, messages, maxq, leaf=True), "n=%d %s" % (n, messages))
        if n in (6, 9, 12):
            R.check_outputs(walk, R.decode(llr, mask, values, messages, maxq), pos, N, mask, "n=%d %s" % (n, messages))
        plain = q.polar_decode_wide_host(n, pos, llr, fz, messages, maxq)
        assert set(plain) == {"u", "info", "x"} and all(np.array_equal(plain[k], walk[k]) for k in plain)


@pytest.mark.parametrize("K", ["none", "all"])
def test_walk_on_the_edge_codes(q, K):
    rng = np.random.default_rng(3)
    n, N = 13, 1 << 13
    pos, _ = R.random_code(rng, N, 0 if K == "none" else N)
    llr = R.f32_inputs(rng, 2, N)
    fz = R.pack(rng.integers(0, 2, (2, N), dtype=np.uint8))
    _same(q.polar_decode_wide_host(n, pos, llr, fz, "f32", leaf=True), q.polar_decode_host(n, pos, llr, fz, "f32", leaf=True), K)


# ---- the layout ----------------------------------------------------------------------------------------------------------------------------

LAYOUT_C = r"""
#include <stdio.h>
#include "qldpc_polar_wide_core.h"
int main(void)
{
    printf("C %d %d %d LANES %d WIN %d\n", PLW_CHIP_LOG, PLW_CHIP_MIN, PLW_CHIP_MAX, PLW_LANES, PLW_WIN);
    for (int c = PLW_CHIP_MIN; c <= PLW_CHIP_MAX; c++)
        for (int n = 1; n <= PL_MAX_LOG2N; n++) {
            printf("N %d %d %d %zu %zu %zu\n", c, n, n > 5 ? plw_chip(n, c) : 0, plw_scratch_elems(n, c), plw_lds_elems(n, c), n > 5 ? plw_win_words(n) : (size_t)0);
            for (int l = 6; l < n; l++)
                printf("L %d %d %d %d %zu\n", c, n, l, l > plw_chip(n, c), l > plw_chip(n, c) ? plw_level_off(n, l) : plw_lds_off(plw_chip(n, c), l));
        }
    return 0;
}
"""


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    """what the core header states, printed by a C program: the constants, per (c, n) the sizes, per level where it lives and its offset"""
    d = tmp_path_factory.mktemp("plw")
    src, exe = str(d / "layout.c"), str(d / "layout")
    open(src, "w").write(LAYOUT_C)
    subprocess.check_call(["gcc", "-std=gnu11", "-Wall", "-Wextra", "-I" + CSRC, "-o", exe, src])
    consts, sizes, levels = None, {}, {}
    for row in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split("\n"):
        w = row.split()
        if w and w[0] == "C":
            consts = dict(chip=int(w[1]), chip_min=int(w[2]), chip_max=int(w[3]), lanes=int(w[5]), win=int(w[7]))
        elif w and w[0] == "N":
            sizes[int(w[1]), int(w[2])] = tuple(int(v) for v in w[3:])
        elif w:
            levels.setdefault((int(w[1]), int(w[2])), []).append((int(w[3]), int(w[4]), int(w[5])))
    return consts, sizes, levels


def test_layout_constants(layout):
    consts = layout[0]
    assert 6 <= consts["chip_min"] <= consts["chip"] <= consts["chip_max"] <= 13 and consts["lanes"] in (64, 256, 512, 1024) and consts["win"] == 64
    # float messages at the highest chip level, and the four windows, fit the 160 KiB of LDS
    assert 4 * (2 << consts["chip_max"]) + 4 * 4 * consts["win"] <= 160 * 1024


def test_layout_levels_tile_their_arrays(layout):
    """for every chip level and every n: the levels n - 1 .. 6 of a frame lie in the scratch or in LDS, those of each array are disjoint, inside
    the stated size and add up to it; the scratch is below N elements; levels above the chip level are the scratch's"""
    consts, sizes, levels = layout
    for (c, n), (chip, s_elems, l_elems, win) in sizes.items():
        N = 1 << n
        if n <= 5:
            assert (s_elems, l_elems) == (0, 0)
            continue
        assert chip == min(c, n - 1) and win == min(64, N // 32) and s_elems < N
        for in_scratch, total in ((1, s_elems), (0, l_elems)):
            spans = sorted((off, off + (1 << l)) for l, where, off in levels.get((c, n), []) if where == in_scratch)
            assert all(a[1] == b[0] for a, b in zip(spans, spans[1:])), (c, n, spans)
            assert (spans[0][0] == 0 and spans[-1][1] == total) if spans else total == 0, (c, n, spans, total)
        assert all(where == (l > chip) for l, where, _ in levels.get((c, n), []))
        # quads: every level starts on a multiple of 4 elements, and so does the next frame's scratch
        assert all(off % 4 == 0 for _, _, off in levels.get((c, n), [])) and s_elems % 4 == 0


# ---- the refusals ------------------------------------------------------------------------------------------------------------------------

def _status(q, fn, *args, **kw):
    with pytest.raises(q.QldpcError) as e:
        fn(*args, **kw)
    assert str(e.value)
    return e.value


def test_create_form_refuses_an_unknown_form(q):
    for form in (-1, 2):
        e = _status(q, q.Polar, 8, [3], form=form)
        assert e.status == -1 and "QLDPC_POLAR_LANES" in str(e) and "QLDPC_POLAR_WIDE" in str(e)
    assert _status(q, q.Polar, 8, [3], form="deep").status == -1
    h = q._vp()
    assert q._L.qldpc_polar_create_form(8, 0, None, 0, 31, 1, 7, 0, C.byref(h)) == -1 and not h.value
    assert q._L.qldpc_polar_create_form(8, 0, None, 0, 31, 1, 1, 0, None) == -1


@pytest.mark.parametrize("form", ["lanes", "wide"])
def test_create_form_refuses_what_create_refuses_without_a_device(q, form):
    """status and message of every refusal of qldpc_polar_create, before the first HIP call"""
    ESIZE, EINVAL = -6, -1
    cases = [((0, []), {}, ESIZE), ((21, []), {}, ESIZE), ((4, [16]), {}, ESIZE), ((4, [3, 3]), {}, EINVAL), ((4, [3]), dict(maxq=127), ESIZE),
             ((4, [3]), dict(maxq=0), ESIZE), ((4, [3]), dict(max_frames=0), EINVAL), ((8, [256]), {}, ESIZE), ((8, [3]), dict(max_frames=(1 << 24) + 1), EINVAL)]
    def create(n, pos, maxq=31, max_frames=4096):                 # qldpc_polar_create itself, which the class no longer calls
        pos = np.ascontiguousarray(pos, dtype=np.int32)
        return q._create("Polar", q._L.qldpc_polar_create, n, pos.size, pos.ctypes.data_as(q._ip), 0, maxq, max_frames, 0)

    for args, kw, status in cases:
        old, new = _status(q, create, *args, **kw), _status(q, q.Polar, *args, form=form, **kw)
        assert old.status == new.status == status and str(old) == str(new), (args, kw)
    assert _status(q, q.Polar, 4, [3], messages="bf16", form=form).status == EINVAL
    h = q._vp()
    assert q._L.qldpc_polar_create_form(8, 0, None, 2, 31, 1, q.POLAR_FORMS[form], 0, C.byref(h)) == EINVAL      # messages neither value


def test_walk_refuses_what_the_mirror_refuses(q):
    ESIZE, EINVAL = -6, -1
    z = lambda n, dt=np.int8: np.zeros((1, 1 << n), dt)
    for args, kw, status in [((0, [], np.zeros((1, 1), np.int8)), {}, ESIZE), ((21, [], np.zeros((1, 1), np.int8)), {}, ESIZE), ((3, [0, 8], z(3)), {}, ESIZE),
                             ((3, [1, 2, 1], z(3)), {}, EINVAL), ((3, [1], z(3)), dict(maxq=127), ESIZE), ((3, [1], z(3)), dict(messages="f16"), EINVAL),
                             ((7, [1], z(6)), {}, ESIZE)]:
        assert _status(q, q.polar_decode_wide_host, *args, **kw).status == _status(q, q.polar_decode_host, *args, **kw).status == status
    L = q._L
    assert L.qldpc_polar_decode_wide_host(7, 0, None, 0, 31, 1, None, None, None, None, None, None) == EINVAL
    assert L.qldpc_polar_decode_wide_host(7, 0, None, 0, 31, -1, None, None, None, None, None, None) == EINVAL
    assert L.qldpc_polar_decode_wide_host(7, 0, None, 0, 31, 0, None, None, None, None, None, None) == 0


def test_header_names_the_forms():
    text = open(os.path.join(ROOT, "include", "qldpc.h")).read()
    assert re.search(r"enum\s*\{\s*QLDPC_POLAR_LANES\s*=\s*0\s*,\s*QLDPC_POLAR_WIDE\s*=\s*1\s*\}", text)


# ---- the sanitizer program ---------------------------------------------------------------------------------------------------------------

def test_wide_walk_under_asan_ubsan(tmp_path):
    """the walk at n = 1 .. 13 with every row malloc'ed at its exact size, each output alone and all together, against the mirror, as a
    stand-alone program (nothing loaded into Python is sanitised)"""
    exe = str(tmp_path / "polar_wide_sanitize")
    subprocess.check_call(["gcc", "-std=gnu11", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "c", "polar_wide_sanitize.c"),
                           os.path.join(CSRC, "qldpc_polar_wide_host.c"), os.path.join(CSRC, "qldpc_polar_host.c"), "-lm"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "sanitizer pass ok" in r.stdout, r.stdout + r.stderr
