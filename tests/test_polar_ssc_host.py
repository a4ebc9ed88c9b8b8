"""CPU suite of the simplified SC decoder: the host mirror (qldpc_polar_decode_ssc_host) and the plan (qldpc_polar_ssc_plan_host) against the numpy
restatement of tests/polar_ssc_ref.py bit for bit, the mirror against the SC mirror where the theorem of qldpc_polar_ssc_core.h says they are
equal, the published SC curve and the reconciliation form through the SSC mirror, the argument checks and the sanitizer program.  No GPU, no
device."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import polar_ref as R
import polar_ssc_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = 70
SEED = 20261
KINDS = ("i8", "f32")


def _inputs(rng, messages, N, frames=F):
    return R.i8_inputs(rng, frames, N, 31) if messages == "i8" else R.f32_inputs(rng, frames, N)


def _codes(rng, n):
    """(name, info_pos, frozen mask) of a size: a random code, a clustered one, and at their sizes the 5G set and K = 0, K = N"""
    N = 1 << n
    yield ("random",) + R.random_code(rng, N)
    yield ("clustered",) + S.clustered_code(rng, n)
    if n == 10:
        pos = R.nr_order(N)[N // 2:]
        yield "5g", pos, S.mask_of(pos, N)
    if n in (4, 7):
        yield ("none",) + R.random_code(rng, N, 0)
        yield ("all",) + R.random_code(rng, N, N)


# ---- the mirror and the plan against the restatement -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("messages", KINDS)
@pytest.mark.parametrize("n", range(1, 13))
def test_mirror_is_the_restatement(q, n, messages):
    """u, info and x bit for bit on ties, +-0.0, denormals and 1e30, the frozen values given and NULL"""
    rng = np.random.default_rng([SEED, n, messages == "i8"])
    N = 1 << n
    for name, pos, mask in _codes(rng, n):
        llr = _inputs(rng, messages, N)
        for fv in (rng.integers(0, 2, (F, N), dtype=np.uint8), None):
            out = q.polar_decode_ssc_host(n, pos, llr, None if fv is None else R.pack(fv), messages, 31)
            assert set(out) == {"u", "info", "x"}
            S.check_outputs(out, S.decode(llr, mask, fv, messages, 31), pos, "n=%d %s %s" % (n, name, messages))


@pytest.mark.parametrize("n", range(1, 13))
def test_plan_is_the_restatement(q, n):
    rng = np.random.default_rng([SEED, n, 2])
    N = 1 << n
    for draw in range(4):
        for name, pos, mask in list(_codes(rng, n)) + [("no_pair",) + S.no_pair_code(rng, n)]:
            got = q.polar_ssc_plan(n, pos)
            assert got.dtype == np.int32 and np.array_equal(got, S.plan(mask)), "n=%d %s" % (n, name)
            # the steps tile the frame in leaf order, aligned, and none is a uniform node that could have been larger
            blocks = np.maximum(1 << np.maximum(got[:, 1] - 5, 0), 1)
            assert got[0, 0] == 0 and np.array_equal(got[1:, 0], np.cumsum(blocks)[:-1]) and int(blocks.sum()) == max(N // 32, 1)
            assert not (got[:, 0] % blocks).any() and len(got) <= max(N // 32, 1)


def test_plan_of_the_clustered_codes_holds_what_the_tests_need(q):
    """the generator gives rate-0 and rate-1 steps of 2^5 .. 2^9 leaves, as left and as right children, within four draws a size"""
    seen = set()
    for n in (6, 7, 9, 11, 12):
        rng = np.random.default_rng([SEED, n, 9])
        for _ in range(4):
            for j, lam, kind in q.polar_ssc_plan(n, S.clustered_code(rng, n)[0]).tolist():
                if kind != S.MIXED:
                    seen.add((kind, lam, (j >> (lam - 5)) & 1))
    for kind in (S.RATE0, S.RATE1):
        assert {lam for k, lam, _ in seen if k == kind} >= set(range(5, 10)), seen
        assert {side for k, _, side in seen if k == kind} == {0, 1}


# ---- against the SC mirror -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("messages", KINDS)
@pytest.mark.parametrize("n", range(1, 11))
def test_rate_0_pruning_is_exact(q, n, messages):
    """a code with no rate-1 node of two leaves or more: SSC is SC on every input kind, frames full of zeros included"""
    rng = np.random.default_rng([SEED, n, messages == "i8", 3])
    N = 1 << n
    pos, mask = S.no_pair_code(rng, n)
    llr = _inputs(rng, messages, N)
    fz = R.pack(rng.integers(0, 2, (F, N), dtype=np.uint8))
    ssc, sc = q.polar_decode_ssc_host(n, pos, llr, fz, messages, 31), q.polar_decode_host(n, pos, llr, fz, messages, 31)
    assert all(np.array_equal(ssc[k], sc[k]) for k in ("u", "info", "x"))


@pytest.mark.parametrize("n", [6, 7, 9, 10, 11, 12])
def test_tie_free_floats_decode_as_sc(q, n):
    """4 standard_normal float inputs on clustered codes and the 5G set: no frame is flagged, and SSC is SC bit for bit"""
    rng = np.random.default_rng([SEED, n, 4])
    N = 1 << n
    for name, pos, mask in _codes(rng, n):
        if name == "random":
            continue
        llr = (4.0 * rng.standard_normal((F, N))).astype(np.float32)
        fv = rng.integers(0, 2, (F, N), dtype=np.uint8)
        flag = S.decode(llr, mask, fv, "f32")[2]
        assert not flag.any(), "n=%d %s: %d frames flagged" % (n, name, int(flag.sum()))
        ssc, sc = q.polar_decode_ssc_host(n, pos, llr, R.pack(fv), "f32"), q.polar_decode_host(n, pos, llr, R.pack(fv), "f32")
        assert all(np.array_equal(ssc[k], sc[k]) for k in ("u", "info", "x")), "n=%d %s" % (n, name)


@pytest.mark.parametrize("messages", KINDS)
@pytest.mark.parametrize("n", range(1, 13))
def test_unflagged_frames_decode_as_sc(q, n, messages):
    """the theorem on every input kind: a frame in which no belief of a rate-1 node is 0 decodes as under SC, bit for bit"""
    rng = np.random.default_rng([SEED, n, messages == "i8", 5])
    N = 1 << n
    for name, pos, mask in _codes(rng, n):
        llr = _inputs(rng, messages, N)
        fv = rng.integers(0, 2, (F, N), dtype=np.uint8)
        ok = ~S.decode(llr, mask, fv, messages, 31)[2]
        ssc, sc = q.polar_decode_ssc_host(n, pos, llr, R.pack(fv), messages, 31), q.polar_decode_host(n, pos, llr, R.pack(fv), messages, 31)
        print("n=%d %s %s: %d of %d frames flagged" % (n, name, messages, int((~ok).sum()), F))
        assert all(np.array_equal(ssc[k][ok], sc[k][ok]) for k in ("u", "info", "x")), "n=%d %s" % (n, name)


@pytest.mark.parametrize("messages", KINDS)
@pytest.mark.parametrize("n", [4, 7])
def test_closed_forms(q, n, messages):
    rng = np.random.default_rng([SEED, n, 6])
    N = 1 << n
    llr = _inputs(rng, messages, N)
    fz = R.pack(rng.integers(0, 2, (F, N), dtype=np.uint8))
    out = q.polar_decode_ssc_host(n, np.arange(N, dtype=np.int32), llr, fz, messages, 31)
    assert np.array_equal(out["x"], R.pack(np.asarray(llr) < 0))      # K = N: the signs of what was received
    assert np.array_equal(q.polar_encode_host(n, out["u"]), out["x"]) and np.array_equal(out["info"], out["u"])
    out = q.polar_decode_ssc_host(n, [], llr, fz, messages, 31)
    assert np.array_equal(out["u"], fz) and out["info"].shape == (F, 0)      # K = 0: the frozen values
    assert np.array_equal(out["x"], q.polar_encode_host(n, fz))


# ---- the published curve and the reconciliation form -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [2, 3])
def test_published_sc_curve_on_the_ssc_mirror(q, k):
    row, pos, msg, rq = R.fer_point(k)
    info = R.info_bits(q.polar_decode_ssc_host(10, pos, rq, None, "i8", 31)["info"], len(pos))
    errors, frames = int((info != msg).any(axis=1).sum()), len(msg)
    print("Eb/N0 %.1f dB: %d / %d = %.5f, published %.4f (%d / %d), band +-%.5f" % (row[0], errors, frames, errors / frames, row[1], row[3], row[5],
                                                                                     R.fer_band(row, frames)))
    assert abs(errors / frames - row[1]) <= R.fer_band(row, frames)


def test_reconciliation_form(q):
    """BSC LLRs are all ties, so SSC and SC are different decoders here: their failure counts differ by no more than 4 sqrt(d), d the frames on
    which their x differ (each such frame moves the difference by at most one)"""
    pos, x, frozen, llr = R.recon_frames(5, qber=0.06)
    ssc, sc = q.polar_decode_ssc_host(10, pos, llr, frozen, "f32")["x"], q.polar_decode_host(10, pos, llr, frozen, "f32")["x"]
    key = R.pack(x)
    fails_ssc, fails_sc = int((ssc != key).any(axis=1).sum()), int((sc != key).any(axis=1).sum())
    d = int((ssc != sc).any(axis=1).sum())
    print("fails: SSC %d, SC %d of %d; x differs on %d frames" % (fails_ssc, fails_sc, len(x), d))
    assert abs(fails_ssc - fails_sc) <= 4.0 * math.sqrt(d)


# ---- argument checks -------------------------------------------------------------------------------------------------------------------------

def _status(q, fn, *args, **kw):
    with pytest.raises(q.QldpcError) as e:
        fn(*args, **kw)
    assert str(e.value)
    return e.value.status


def test_argument_checks(q):
    ESIZE, EINVAL = -6, -1
    z = lambda n, dt=np.int8: np.zeros((1, 1 << n), dt)
    dec = q.polar_decode_ssc_host
    assert _status(q, dec, 0, [], np.zeros((1, 1), np.int8)) == ESIZE
    assert _status(q, dec, 21, [], np.zeros((1, 1), np.int8)) == ESIZE
    assert _status(q, dec, 3, [0, 8], z(3)) == ESIZE                                # a position at N
    assert _status(q, dec, 3, [-1], z(3)) == ESIZE
    assert _status(q, dec, 3, [1, 2, 1], z(3)) == EINVAL                            # a position twice
    assert _status(q, dec, 2, [0, 1, 2, 3, 0], z(2)) == ESIZE                       # more positions than bits
    assert _status(q, dec, 3, [1], z(3), maxq=127) == ESIZE                         # f gives maxq + 1 = 128
    assert _status(q, dec, 3, [1], z(3), maxq=0) == ESIZE
    assert _status(q, dec, 3, [1], z(3), messages="f16") == EINVAL
    assert _status(q, dec, 3, [1], z(2)) == ESIZE                                   # llr rows of the wrong length
    assert _status(q, dec, 3, [1], z(3), frozen=np.zeros((2, 1), np.uint32)) == ESIZE
    assert "polar_decode_ssc_host" in str(pytest.raises(q.QldpcError, dec, 3, [1], z(3), maxq=127).value)
    dec(3, [1], z(3, np.float32), messages="f32", maxq=127)                       # the float messages ignore maxq
    L = q._L
    assert L.qldpc_polar_decode_ssc_host(3, 0, None, 0, 31, 1, None, None, None, None, None) == EINVAL      # llr NULL
    assert L.qldpc_polar_decode_ssc_host(3, 0, None, 0, 31, -1, None, None, None, None, None) == EINVAL
    assert L.qldpc_polar_decode_ssc_host(3, 0, None, 2, 31, 0, None, None, None, None, None) == EINVAL
    assert L.qldpc_polar_decode_ssc_host(3, 1, None, 0, 31, 0, None, None, None, None, None) == ESIZE
    assert L.qldpc_polar_decode_ssc_host(3, 0, None, 0, 31, 0, None, None, None, None, None) == 0          # no frames: nothing to do
    assert _status(q, q.polar_ssc_plan, 0, []) == ESIZE
    assert _status(q, q.polar_ssc_plan, 21, []) == ESIZE
    assert _status(q, q.polar_ssc_plan, 3, [8]) == ESIZE
    assert _status(q, q.polar_ssc_plan, 3, [1, 1]) == EINVAL
    assert L.qldpc_polar_ssc_plan_host(3, 0, None, None, None) == EINVAL


def test_create_rule_checks_its_arguments_without_a_device(q):
    """every refusal of qldpc_polar_create_rule comes before the first HIP call, so it is the same on a machine without a GPU"""
    ESIZE, EINVAL, EUNSUPPORTED = -6, -1, -7
    make = lambda *a, **kw: q.Polar(*a, **kw)
    assert _status(q, make, 4, [3], rule="fast") == EINVAL
    assert _status(q, make, 4, [3], rule=2) == EINVAL
    assert _status(q, make, 4, [3], form=7, rule="ssc") == EINVAL
    assert _status(q, make, 14, [3], form="wide", rule="ssc") == EUNSUPPORTED
    assert "QLDPC_POLAR_LANES" in str(pytest.raises(q.QldpcError, make, 14, [3], form="wide", rule="ssc").value)
    assert _status(q, make, 21, [3], form="wide", rule="ssc") == ESIZE            # the size is checked first
    for rule in ("sc", "ssc"):
        assert _status(q, make, 0, [], rule=rule) == ESIZE
        assert _status(q, make, 4, [16], rule=rule) == ESIZE
        assert _status(q, make, 4, [3, 3], rule=rule) == EINVAL
        assert _status(q, make, 4, [3], maxq=127, rule=rule) == ESIZE
        assert _status(q, make, 4, [3], max_frames=0, rule=rule) == EINVAL
    h = C.c_void_p(1)
    assert q._L.qldpc_polar_create_rule(8, 0, None, 0, 31, 1, 0, 5, 0, C.byref(h)) == EINVAL and not h.value
    assert q._L.qldpc_polar_create_rule(8, 0, None, 0, 31, 1, 0, 1, 0, None) == EINVAL


# ---- the sanitizer program -------------------------------------------------------------------------------------------------------------------

def test_host_code_under_asan_ubsan(tmp_path):
    """the SSC mirror and the plan at every size up to 2^12 with every row malloc'ed at its exact size and each output alone, as a stand-alone
    program (nothing loaded into Python is sanitised)"""
    exe = str(tmp_path / "polar_ssc_sanitize")
    csrc = os.path.join(ROOT, "qcrypto-ldpc_amd", "csrc")
    subprocess.check_call(["gcc", "-std=gnu11", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                           "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-o", exe, os.path.join(ROOT, "tests", "c", "polar_ssc_sanitize.c"),
                           os.path.join(csrc, "qldpc_polar_ssc_host.c"), os.path.join(csrc, "qldpc_polar_host.c"), "-lm"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "sanitizer pass ok" in r.stdout, r.stdout + r.stderr
