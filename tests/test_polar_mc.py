"""CPU suite of the Monte-Carlo loop around the polar decoders (qldpc_polar_mc_*): the host mirror of its frames against the numpy restatement of
tests/polar_mc_ref.py bit for bit, the AWGN table builder in both roundings, the restated counters, the published SC and list-4 curves on the
mirror's frames, the argument checks and the sanitizer program.  No GPU, no device."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import polar_list_ref as LR
import polar_mc_ref as M
import polar_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qcrypto-ldpc_amd", "csrc")
TWO32 = 1 << 32
CRC32 = (32, 0x04C11DB7)
FIRSTS = (0, 7, (1 << 32) - 2, (1 << 32) + 12345, (1 << 63) + 5)


def table(levels, messages, rng):
    """a threshold table of `levels` levels: ascending rows with runs of equal thresholds (levels of probability zero), a first level nothing
    reaches and, from 64 levels on, last levels nothing reaches; int8 messages get integers over the whole int8 range, one of them 0"""
    rows = []
    for _ in (0, 1):
        r = np.sort(rng.integers(0, TWO32, levels - 1, dtype=np.uint64))
        if levels >= 3:
            r[0] = 0
        if levels >= 64:
            r[10:14] = r[10]
            r[-3:] = TWO32
        rows.append(np.sort(r))
    if messages == "i8":
        value = rng.integers(-128, 128, levels).astype(np.float32)
        value[:2] = (-128.0, 127.0)
    else:
        value = (rng.standard_normal(levels) * 6.0).astype(np.float32)
    value[levels // 2] = 0.0
    return rows[0], rows[1], value


def codes(n):
    """(K, crc) of a size: K = 0, K = N, K no multiple of 32, a message shorter than a word (A < 32), each CRC the K allows"""
    N = 1 << n
    out = []
    for K in sorted({0, N, N // 2 + 1 if N > 2 else 1, min(N, 16), min(N, 40)}):
        out += [(K, crc) for crc in ((0, 0), LR.CRC11, CRC32) if crc[0] <= K]
    return out


@pytest.mark.parametrize("messages", ["i8", "f32"])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 6, 10])
def test_mirror_is_the_restatement(q, n, messages):
    """info, u, x, llr and flips of the mirror against numpy, over the codes, the CRCs, the modes, the table shapes and first frames above 2^32"""
    rng = np.random.default_rng([n, messages == "i8", 5])
    N, F = 1 << n, 5
    for t, (K, crc) in enumerate(codes(n)):
        pos, _ = R.random_code(rng, N, K)
        frozen, source, levels = ("zero", "random")[t & 1], ("random", "zero")[(t >> 1) % 3 == 0], (2, 3, 64, 256)[t % 4]
        tab, seed, first = table(levels, messages, rng), int(rng.integers(0, 1 << 63)), FIRSTS[t % len(FIRSTS)]
        what = "n=%d %s K=%d crc=%d %s %s Q=%d first=%d" % (n, messages, K, crc[0], frozen, source, levels, first)
        got = q.polar_mc_frames_host(n, pos, first, F, seed, tab, messages, crc[0], crc[1], frozen, source)
        assert set(got) == set(q.POLAR_MC_OUTPUTS)
        M.check_frames(got, M.frames(n, pos, seed, first, F, tab, messages, crc, frozen, source), what)
        # the info row's own remainder is 0, and a frame's flips are what its LLRs say
        assert not q.polar_crc_host(crc[0], crc[1], got["info"], K).any(), what
        x = R.unpack(got["x"], N)
        assert np.array_equal(got["flips"], np.where(x == 1, got["llr"] > 0, got["llr"] < 0).sum(axis=1)), what


@pytest.mark.parametrize("messages", ["i8", "f32"])
def test_ranges_add_up(q, messages):
    """frames [a, a + n) in one call are the same frames in two calls, across 2^32 too"""
    rng = np.random.default_rng(17)
    pos, _ = R.random_code(rng, 64, 37)
    tab = table(64, messages, rng)
    for a in (3, (1 << 32) - 4):
        args = dict(seed=99, table=tab, messages=messages, crc_len=11, crc_poly=0x621, frozen="random")
        whole = q.polar_mc_frames_host(6, pos, a, 9, **args)
        parts = [q.polar_mc_frames_host(6, pos, a, 4, **args), q.polar_mc_frames_host(6, pos, a + 4, 5, **args)]
        for k in whole:
            assert np.array_equal(whole[k], np.concatenate([p[k] for p in parts])), k
    only = q.polar_mc_frames_host(6, pos, 3, 9, want=("u", "flips"), **args)
    assert set(only) == {"u", "flips"}


def test_a_bsc_is_the_two_level_table(q):
    """{+mag, -mag}: the LLR is +-mag, x_v = 0 sees -mag with probability qber, and flips counts them"""
    pos = R.nr_order(1024)[512:]
    t = int(math.floor(0.06 * TWO32))
    got = q.polar_mc_frames_host(10, pos, 0, 200, 3, ([TWO32 - t], [t], [2.75, -2.75]), "f32", frozen="random")
    x = R.unpack(got["x"], 1024)
    assert set(np.unique(got["llr"]).tolist()) == {-2.75, 2.75}
    assert np.array_equal(got["flips"], ((got["llr"] < 0) != (x == 1)).sum(axis=1))
    assert abs(got["flips"].sum() / (200 * 1024) - 0.06) < 4 * math.sqrt(0.06 * 0.94 / (200 * 1024))
    assert abs(x.mean() - 0.5) < 4 * 0.5 / math.sqrt(200 * 1024)             # the reconciliation form: x is a uniformly random word


# ---- the table builder -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sigma, rmax, maxq", [(0.8414, 3.0, 31), (0.7, 4.0, 31), (1.3, 4.0, 7), (0.5, 2.5, 127)])
def test_awgn_table_by_floor_is_the_ldpc_loops(q, sigma, rmax, maxq):
    a, b = q.polar_mc_awgn_table(sigma, rmax, maxq, "floor"), q.mc_awgn_table(sigma, rmax, maxq)
    assert len(a[2]) == 2 * maxq + 2
    for x, y in zip(a, b):
        assert x.dtype == np.asarray(y).dtype and np.array_equal(x, y)


@pytest.mark.parametrize("sigma, rmax, maxq", [(0.8414, 4.0, 31), (0.6, 3.0, 15), (1.1, 4.0, 127)])
def test_awgn_table_by_round_is_the_list_scripts_quantiser(q, sigma, rmax, maxq):
    """a received value r = (1 - 2 b) + sigma z corresponds to the draw u = floor(2^32 Phi(z)): the table's level of u carries
    round(clip(r, -rmax, rmax) / rmax * maxq).  The grid of r is the part a 32-bit draw resolves: |z| <= 4.5, where the density of 2^32 Phi is
    above 6e4 per unit of z, and 1e-3 quantiser steps clear of a rounding boundary, which is 1e-3 rmax / (maxq sigma) > 1.9e-5 in z for the
    shapes here, so that u and the boundary's threshold differ by more than one count"""
    cum0, cum1, value = q.polar_mc_awgn_table(sigma, rmax, maxq, "round")
    assert len(value) == 2 * maxq + 1 and len(cum0) == len(cum1) == 2 * maxq
    assert np.array_equal(value, np.arange(-maxq, maxq + 1, dtype=np.float32))
    grid = np.arange(-1.0 - 4.5 * sigma, 1.0 + 4.5 * sigma, 0.00937)
    scaled = np.clip(grid, -rmax, rmax) / rmax * maxq
    grid = grid[np.abs(scaled - np.floor(scaled) - 0.5) > 1e-3]
    for b, cum in ((0, cum0), (1, cum1)):
        r = grid[np.abs(grid - (1 - 2 * b)) <= 4.5 * sigma]
        assert len(r) > 500
        u = np.array([math.floor(TWO32 * 0.5 * math.erfc(-((v - (1 - 2 * b)) / sigma) / math.sqrt(2.0))) for v in r], np.uint64)
        level = np.searchsorted(cum, u, side="right")
        assert np.array_equal(value[level], np.round(np.clip(r, -rmax, rmax) / rmax * maxq).astype(np.float32)), b


# ---- the counters, restated ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", [None, 4])
def test_restated_counters_are_numpys(q, L):
    """the yardstick of the GPU suite (the mirror's frames through the host decoders) against numpy from end to end on a small code"""
    n, N, F, seed, first = 6, 64, 60, 5, (1 << 32) - 20
    crc = LR.CRC11 if L else (0, 0)
    pos = R.nr_order(N)[N - 32 - crc[0]:]
    tab = q.polar_mc_awgn_table(0.95, 4.0, 31, "round")
    got, failed = M.counters(q, n, pos, seed, first, F, tab, "i8", 31, L, crc, "random")
    fr = M.frames(n, pos, seed, first, F, tab, "i8", crc, "random")
    mask = np.ones(N, bool)
    mask[pos] = False
    if L:
        ref = LR.decode(fr["llr"], mask, fr["u"], "i8", 31, L, pos, *crc)
        info, pick = ref["info"], ref["pick"]
    else:
        info, pick = R.decode(fr["llr"], mask, fr["u"], "i8", 31)[0][:, pos], np.zeros(F, np.int32)
    A = len(pos) - crc[0]
    be = (info[:, :A] != fr["info"][:, :A]).sum(axis=1)
    want = dict(frames=F, bit_errors=int(be.sum()), frame_errors=int((be > 0).sum()), undetected=int(((be > 0) & (pick >= 0)).sum()),
                crc_fails=int((pick < 0).sum()), channel_flips=int(fr["flips"].sum()), channel_bits=F * N)
    assert got == want and 0 < want["frame_errors"] < F
    assert failed.dtype == np.uint64 and failed.tolist() == [first + int(f) for f in np.nonzero(be > 0)[0]]


# ---- the published curves on the mirror's frames -------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sc_points(q):
    out = []
    for k in range(5):
        row, pos, tab, F = M.sc_point(q, k)
        out.append((row, F, M.counters(q, 10, pos, M.MC_SEED, 0, F, tab, "i8", 31)[0]))
    return out


@pytest.fixture(scope="module")
def list_points(q):
    out = []
    for k in range(4):
        row, pos, tab, F = M.list_point(q, k)
        out.append((row, F, M.counters(q, 10, pos, M.MC_SEED, 0, F, tab, "i8", 31, 4, LR.CRC11)[0]))
    return out


def _in_band(row, F, c):
    fer = c["frame_errors"] / F
    print("Eb/N0 %.2f dB: %d / %d = %.5f, published %.4f (%d / %d), band +-%.5f; undetected %d, crc fails %d, channel flips %.5f" % (
        row[0], c["frame_errors"], F, fer, row[1], row[3], row[5], R.fer_band(row, F), c["undetected"], c["crc_fails"], c["channel_flips"] / c["channel_bits"]))
    assert c["frames"] == F and abs(fer - row[1]) <= R.fer_band(row, F)


@pytest.mark.parametrize("k", range(5))
def test_published_sc_curve_on_the_mirrors_frames(sc_points, k):
    row, F, c = sc_points[k]
    _in_band(row, F, c)
    assert c["crc_fails"] == 0 and c["undetected"] == c["frame_errors"]         # SC detects nothing


@pytest.mark.parametrize("k", range(4))
def test_published_list_curve_on_the_mirrors_frames(list_points, k):
    row, F, c = list_points[k]
    _in_band(row, F, c)
    assert c["undetected"] == 0 and c["crc_fails"] == c["frame_errors"]         # a frame that passed the CRC is the message sent


# ---- the argument checks -------------------------------------------------------------------------------------------------------------------

def _status(q, fn, *args, **kw):
    with pytest.raises(q.QldpcError) as e:
        fn(*args, **kw)
    assert str(e.value)
    return e.value.status


def test_mirror_refusals(q):
    ESIZE, EINVAL, ESTATE = -6, -1, -8
    f = q.polar_mc_frames_host
    tab = ([1 << 31], [1 << 30], [3.0, -3.0])
    assert _status(q, f, 0, [], 0, 1, table=tab) == ESIZE
    assert _status(q, f, 21, [], 0, 1, table=tab) == ESIZE
    assert _status(q, f, 3, [8], 0, 1, table=tab) == ESIZE
    assert _status(q, f, 3, [1, 1], 0, 1, table=tab) == EINVAL
    assert _status(q, f, 3, [1], 0, -1, table=tab) == EINVAL
    assert _status(q, f, 3, [1], 0, 1, table=tab, messages="f16") == EINVAL
    assert _status(q, f, 3, [1], 0, 1, table=tab, frozen="alice") == EINVAL
    assert _status(q, f, 3, [1], 0, 1, table=tab, frozen=2) == EINVAL
    assert _status(q, f, 3, [1], 0, 1, table=tab, source=2) == EINVAL
    assert _status(q, f, 3, [1, 2], 0, 1, table=tab, crc_len=3, crc_poly=3) == ESIZE             # crc_len above n_info
    assert _status(q, f, 3, [1, 2], 0, 1, table=tab, crc_len=2, crc_poly=4) == ESIZE             # a coefficient past crc_len
    assert _status(q, f, 3, [1], 0, 1, table=None) == ESTATE                                     # llr and flips without a table
    assert set(f(3, [1], 0, 1, table=None, want=("info", "u", "x"))) == {"info", "u", "x"}
    # the table: qldpc_mc_set_channel's refusals, and the integer rule of the int8 messages
    assert _status(q, f, 3, [1], 0, 1, table=([], [], [1.0])) == ESIZE
    assert _status(q, f, 3, [1], 0, 1, table=(np.arange(256), np.arange(256), np.zeros(257))) == ESIZE
    assert _status(q, f, 3, [1], 0, 1, table=([5, 4], [1, 2], [1.0, 2.0, 3.0])) == EINVAL
    assert _status(q, f, 3, [1], 0, 1, table=([TWO32 + 1], [1], [1.0, 2.0])) == EINVAL
    assert _status(q, f, 3, [1], 0, 1, table=([1], [1, 2], [1.0, 2.0])) == ESIZE                 # the binding: rows of unequal length
    for bad in (0.5, 128.0, -129.0, float("nan"), float("inf")):
        assert _status(q, f, 3, [1], 0, 1, table=([1], [1], [1.0, bad]), messages="i8") == EINVAL
    assert f(3, [1], 0, 1, table=([1], [1], [1.0, 0.5]), messages="f32")["llr"].dtype == np.float32
    assert f(3, [1], 0, 1, table=([1], [1], [-128.0, 127.0]), messages="i8")["llr"].dtype == np.int8
    L = q._L
    assert L.qldpc_polar_mc_frames_host(3, 0, None, 0, 0, 0, 0, 0, 0, 2, None, None, None, 0, 1, None, None, None, (C.c_int8 * 8)(), None) == EINVAL


def test_table_builder_refusals(q):
    ESIZE, EINVAL = -6, -1
    t = q.polar_mc_awgn_table
    assert _status(q, t, 0.0, 4.0, 31, "round") == _status(q, t, 0.0, 4.0, 31, "floor") == ESIZE
    assert _status(q, t, 0.8, -1.0, 31, "round") == _status(q, t, float("nan"), 4.0, 31, "round") == ESIZE
    assert _status(q, t, 0.8, 4.0, 0, "round") == _status(q, t, 0.8, 4.0, 0, "floor") == ESIZE
    assert _status(q, t, 0.8, 4.0, 128, "round") == _status(q, t, 0.8, 4.0, 128, "floor") == ESIZE
    assert len(t(0.8, 4.0, 127, "round")[2]) == 255 and len(t(0.8, 4.0, 127, "floor")[2]) == 256
    assert _status(q, t, 0.8, 4.0, 31, "nearest") == EINVAL and _status(q, t, 0.8, 4.0, 31, 2) == EINVAL
    assert q._L.qldpc_polar_mc_awgn_table(0.8, 4.0, 31, 1, None, None, None) == EINVAL


def test_object_refusals_without_a_device(q):
    """what the calls on an object refuse before they touch it or the device"""
    EINVAL, L = -1, q._L
    h = q._vp()
    assert L.qldpc_polar_mc_create(None, None, 0, 0, 16, 0, C.byref(h)) == EINVAL and not h.value               # neither context
    assert "exactly one" in L.qldpc_last_error().decode()
    assert L.qldpc_polar_mc_create(q._vp(8), q._vp(8), 0, 0, 16, 0, C.byref(h)) == EINVAL and not h.value         # both
    assert L.qldpc_polar_mc_create(None, None, 0, 0, 16, 0, None) == EINVAL
    ctr, ms = (C.c_uint64 * 16)(), (C.c_double * 8)()
    assert L.qldpc_polar_mc_run(None, 0, 1, 0, ctr, ms) == EINVAL
    assert L.qldpc_polar_mc_frames_dev(None, 0, 1, None, None, None, None, None) == EINVAL
    assert L.qldpc_polar_mc_set_channel(None, 2, None, None, None) == EINVAL
    assert L.qldpc_polar_mc_set_source(None, 0) == EINVAL
    assert L.qldpc_polar_mc_failed_frames(None, None, 0) == EINVAL
    assert L.qldpc_polar_mc_device_bytes(None) == 0
    L.qldpc_polar_mc_free(None)
    assert _status(q, q.PolarMonteCarlo, None, frozen="bob") == EINVAL


def test_header_names_the_loop():
    text = open(os.path.join(ROOT, "include", "qldpc.h")).read()
    assert "typedef struct qldpc_polar_mc qldpc_polar_mc;" in text and "QLDPC_POLAR_MC_COUNTERS = 16" in text
    assert "QLDPC_POLAR_MC_FROZEN_ZERO = 0, QLDPC_POLAR_MC_FROZEN_RANDOM = 1" in text


# ---- the sanitizer program -----------------------------------------------------------------------------------------------------------------

def test_mirror_under_asan_ubsan(tmp_path):
    """the mirror and the table builder with every array malloc'ed at its stated size, as a stand-alone program (nothing loaded into Python is
    sanitised)"""
    exe = str(tmp_path / "polar_mc_sanitize")
    subprocess.check_call(["gcc", "-std=gnu11", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "c", "polar_mc_sanitize.c"),
                           os.path.join(CSRC, "qldpc_polar_mc_host.c"), os.path.join(CSRC, "qldpc_polar_host.c"), os.path.join(CSRC, "qldpc_mc_host.c"),
                           os.path.join(CSRC, "qldpc_graph.c"), "-lm"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "sanitizer pass ok" in r.stdout, r.stdout + r.stderr
