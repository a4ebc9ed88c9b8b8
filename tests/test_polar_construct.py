"""CPU suite of the genie-aided polar code construction (qldpc_polar_tally_host, qldpc_polar_construct_order_host, qldpc_polar_construct_k_host):
the tally's mirror against the numpy restatement of tests/polar_tally_ref.py count for count, against the leaf beliefs of a K = 0 decode_host,
two calls adding up, the two helpers against np.lexsort and a cumulative sum, the refusals, the sanitizer program, and the point of it all: on a
BSC the constructed information set loses fewer frames than the 5G set and the polarization-weight set.  No GPU, no device."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import polar_mc_ref as M
import polar_ref as R
import polar_tally_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qcrypto-ldpc_amd", "csrc")
TWO32 = 1 << 32
SIZES = [1, 2, 3, 4, 5, 6, 7, 8, 11]
KINDS = [("i8", 1), ("i8", 31), ("f32", 0)]


def inputs(rng, n, F, messages, maxq):
    """llr [F, N] (the kinds of polar_ref's inputs: full-range int8 levels, floats with +-0.0, BSC ties, denormals) and true rows as bits and words"""
    N = 1 << n
    llr = R.i8_inputs(rng, F, N, maxq) if messages == "i8" else R.f32_inputs(rng, F, N)
    u = rng.integers(0, 2, (F, N), dtype=np.uint8)
    return llr, u, R.pack(u)


@pytest.mark.parametrize("messages, maxq", KINDS)
@pytest.mark.parametrize("n", SIZES)
def test_mirror_is_the_restatement(q, n, messages, maxq):
    rng = np.random.default_rng([n, maxq, 21])
    F = 12 if n < 11 else 5
    llr, u, words = inputs(rng, n, F, messages, maxq)
    got = q.polar_tally_host(n, llr, words, messages, maxq)
    want = T.tally(llr, u, messages, maxq)
    assert got.dtype == np.uint64 and got.shape == (2, 1 << n) and np.array_equal(got, want)
    assert want[0].sum() > 0 and want[1].sum() > 0                                                        # both rows are exercised
    # the same thing from the leaf beliefs of a code with no information position, frozen to the truth
    leaf = q.polar_decode_host(n, [], llr, words, messages, maxq, leaf=True)["leaf"]
    assert np.array_equal(got[1], (leaf == 0).sum(axis=0)) and np.array_equal(got[0], ((leaf != 0) & ((leaf < 0) != (u == 1))).sum(axis=0))
    # two calls add up, into the caller's row
    acc = q.polar_tally_host(n, llr[:F // 3], words[:F // 3], messages, maxq)
    assert q.polar_tally_host(n, llr[F // 3:], words[F // 3:], messages, maxq, out=acc) is acc and np.array_equal(acc, want)
    assert np.array_equal(q.polar_tally_host(n, llr[:0], words[:0], messages, maxq, out=acc), want)


def test_a_negative_zero_is_a_tie(q):
    llr = np.array([[-0.0, 0.0, -0.0, 0.0]], np.float32)
    got = q.polar_tally_host(2, llr, R.pack(np.array([[1, 1, 0, 1]], np.uint8)), "f32")
    assert np.array_equal(got, [[0, 0, 0, 0], [1, 1, 1, 1]])


@pytest.mark.parametrize("n", [1, 5, 6, 10])
def test_order_and_k_are_lexsort_and_a_cumulative_sum(q, n):
    rng = np.random.default_rng([n, 4])
    N = 1 << n
    for case in range(4):
        t = rng.integers(0, (0, 2, 50, 1 << 40)[case] + 1, (2, N)).astype(np.uint64)        # all equal (zero), many equal scores, few, counts up to 2^40
        for prior in (None, q.polar_pw_order(n), rng.permutation(N).astype(np.int32)):
            got = q.polar_construct_order(t[0], t[1], prior)
            want = T.order(t, prior)
            assert got.dtype == np.int32 and np.array_equal(got, want), (case, prior is None)
            if case == 0:
                assert np.array_equal(got, np.arange(N) if prior is None else prior)
            cum = np.cumsum(T.score(t)[want[::-1]])
            for bound in {0, int(cum[0]), int(cum[0]) + 1, int(cum[N // 2]), int(cum[N // 2]) - 1 if cum[N // 2] else 0, int(cum[-1]), int(cum[-1]) + 5}:
                k = C.c_int(-1)
                assert q._L.qldpc_polar_construct_k_host(n, t.ctypes.data_as(q._u64p), got.ctypes.data_as(q._ip), bound, C.byref(k)) == 0
                assert k.value == T.best_k(t, want, bound), (case, bound)
    # the wrapper's bound: floor(2 frames eps)
    t = np.stack([np.arange(N), np.zeros(N, np.int64)]).astype(np.uint64)
    od = q.polar_construct_order(t[0], t[1])
    assert np.array_equal(od, np.arange(N)[::-1])
    for frames, eps in ((1000, 0.0), (1000, 0.0005), (1000, 0.0031), (7, 0.5), (10, 100.0)):
        assert q.polar_construct_k(t[0], t[1], od, frames, eps) == T.best_k(t, od, math.floor(2 * frames * eps)), (frames, eps)


def _status(q, fn, *args, **kw):
    with pytest.raises(q.QldpcError) as e:
        fn(*args, **kw)
    assert str(e.value)
    return e.value.status


def test_refusals(q):
    ESIZE, EINVAL, L = -6, -1, q._L
    llr, row, t = np.zeros((1, 128), np.int8), np.zeros((1, 4), np.uint32), np.zeros((2, 128), np.uint64)
    f = q.polar_tally_host
    assert _status(q, f, 0, np.zeros((1, 1), np.int8), np.zeros((1, 1), np.uint32)) == ESIZE
    assert _status(q, f, 21, np.zeros((1, 1), np.int8), np.zeros((1, 1), np.uint32)) == ESIZE
    assert _status(q, f, 7, llr, row, "i8", 127) == ESIZE and _status(q, f, 7, llr, row, "i8", 0) == ESIZE
    assert _status(q, f, 7, llr, row, "f16") == EINVAL
    assert _status(q, f, 7, llr[:, :64], row) == ESIZE and _status(q, f, 7, llr, row[:, :3]) == ESIZE
    assert _status(q, f, 7, llr, None) == EINVAL
    assert _status(q, f, 7, llr, row, out=np.zeros((2, 64), np.uint64)) == ESIZE
    p = lambda a, typ: a.ctypes.data_as(typ)
    assert L.qldpc_polar_tally_host(7, 0, 31, -1, p(llr, q._vp), p(row, q._up), p(t, q._u64p)) == EINVAL
    assert L.qldpc_polar_tally_host(7, 0, 31, 1, None, p(row, q._up), p(t, q._u64p)) == EINVAL
    assert L.qldpc_polar_tally_host(7, 0, 31, 1, p(llr, q._vp), None, p(t, q._u64p)) == EINVAL
    assert L.qldpc_polar_tally_host(7, 0, 31, 1, p(llr, q._vp), p(row, q._up), None) == EINVAL
    assert L.qldpc_polar_tally_host(7, 0, 31, 0, None, None, None) == 0
    # the helpers: a size that is no power of two, a prior or an order that is no permutation, counts above 2^40
    od = np.arange(128, dtype=np.int32)
    assert _status(q, q.polar_construct_order, np.zeros(100), np.zeros(100)) == ESIZE
    assert _status(q, q.polar_construct_order, t[0], t[1], od[:64]) == ESIZE
    assert _status(q, q.polar_construct_k, t[0], t[1], od[:64], 10, 0.1) == ESIZE
    assert _status(q, q.polar_construct_k, t[0], t[1], od, 10, -0.1) == EINVAL
    for bad in (5, 128, -1):
        b = od.copy()
        b[6] = bad
        assert _status(q, q.polar_construct_order, t[0], t[1], b) == EINVAL
        assert _status(q, q.polar_construct_k, t[0], t[1], b, 10, 0.1) == EINVAL
    big = t.copy()
    big[1, 77] = (1 << 40) + 1
    assert _status(q, q.polar_construct_order, big[0], big[1]) == ESIZE and _status(q, q.polar_construct_k, big[0], big[1], od, 1, 1.0) == ESIZE
    assert L.qldpc_polar_construct_order_host(7, None, None, p(od, q._ip)) == EINVAL
    assert L.qldpc_polar_construct_order_host(7, p(t, q._u64p), None, None) == EINVAL
    assert L.qldpc_polar_construct_k_host(7, p(t, q._u64p), p(od, q._ip), 0, None) == EINVAL
    # what the device calls refuse before they touch a context or the device
    assert L.qldpc_polar_tally_dev(None, 1, None, None, None) == EINVAL
    assert L.qldpc_polar_mc_construct(None, 0, 1, p(t, q._u64p), None) == EINVAL


def test_header_names_the_calls():
    text = open(os.path.join(ROOT, "include", "qldpc.h")).read()
    for name in ("qldpc_polar_tally_dev", "qldpc_polar_tally_host", "qldpc_polar_mc_construct", "qldpc_polar_construct_order_host", "qldpc_polar_construct_k_host"):
        assert "int    %s(" % name in text, name
    assert "The construction is the caller's" not in text and "genie-aided code construction" in text


def test_host_code_under_asan_ubsan(tmp_path):
    """the mirror and the helpers with every array malloc'ed at its stated size, as a stand-alone program (nothing loaded into Python is sanitised)"""
    exe = str(tmp_path / "polar_tally_sanitize")
    subprocess.check_call(["gcc", "-std=gnu11", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "c", "polar_tally_sanitize.c"),
                           os.path.join(CSRC, "qldpc_polar_tally_host.c"), os.path.join(CSRC, "qldpc_polar_host.c"), "-lm"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "sanitizer pass ok" in r.stdout, r.stdout + r.stderr


# ---- the point of the feature ---------------------------------------------------------------------------------------------------------------

def test_the_constructed_set_beats_the_5g_and_the_pw_set_on_a_bsc(q):
    """N = 1 024, BSC of QBER 0.05, float messages: the tally of 4 000 frames of seed 1 (a K = 0 code with random frozen values, so u is uniformly
    random), ordered with the polarization-weight order as the prior; the SC frame errors of its last 512 positions on 4 000 frames of seed 3
    (random frozen values) beside those of the 5G set and of the polarization-weight set on the same seed.  Everything is a function of the two
    seeds.  Measured: 29 frame errors against 74 (5G) and 79 (polarization weight) of 4 000"""
    n, N, K, F, qber = 10, 1024, 512, 4000, 0.05
    t = int(math.floor(qber * TWO32))
    mag = np.float32(math.log((1.0 - qber) / qber))
    table = ([TWO32 - t], [t], [mag, -mag])
    train = q.polar_mc_frames_host(n, [], 0, F, 1, table, "f32", frozen="random", want=("u", "llr"))
    tally = q.polar_tally_host(n, train["llr"], train["u"], "f32")
    assert (tally <= F).all()
    pw = q.polar_pw_order(n)
    order = q.polar_construct_order(tally[0], tally[1], pw)
    errors = {}
    for name, pos in (("constructed", order[N - K:]), ("5g", R.nr_order(N)[N - K:]), ("pw", pw[N - K:])):
        errors[name] = M.counters(q, n, np.sort(pos).astype(np.int32), 3, 0, F, table, "f32", 31, None, (0, 0), "random")[0]["frame_errors"]
    print("frame errors of %d at QBER %.2f, K = %d: %s" % (F, qber, K, errors))
    assert errors["constructed"] < errors["5g"] and errors["constructed"] < errors["pw"]
