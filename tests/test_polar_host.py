"""CPU suite of the polar subsystem: the host mirrors (qldpc_polar_encode_host, qldpc_polar_decode_host) against the numpy restatement of
tests/polar_ref.py bit for bit, the published SC curve of the reference's fixed-point script, the reconciliation form, the argument checks,
polar_pw_order and the sanitizer program.  No GPU, no device."""
import os
import subprocess

import numpy as np
import pytest

import polar_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the encoder -------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", range(1, 13))
def test_encoder_is_the_restatement_and_an_involution(q, n):
    rng = np.random.default_rng(100 + n)
    N = 1 << n
    u = rng.integers(0, 2, (5, N), dtype=np.uint8)
    x = q.polar_encode_host(n, R.pack(u))
    assert np.array_equal(x, R.pack(R.encode(u)))
    assert np.array_equal(q.polar_encode_host(n, x), R.pack(u))


@pytest.mark.parametrize("n", range(1, 9))
def test_encoder_is_the_kronecker_power(q, n):
    N = 1 << n
    G = R.kron_matrix(n)
    u = np.eye(N, dtype=np.uint8)                                  # every unit vector: the rows of the matrix
    assert np.array_equal(R.unpack(q.polar_encode_host(n, R.pack(u)), N), G)
    rng = np.random.default_rng(n)
    v = rng.integers(0, 2, (7, N), dtype=np.uint8)
    assert np.array_equal(R.unpack(q.polar_encode_host(n, R.pack(v)), N), (v.astype(np.int64) @ G) % 2)


def test_encoder_ignores_the_bits_past_n(q):
    assert q.polar_encode_host(3, np.array([[0xffffffff]], np.uint32))[0, 0] == R.pack(R.encode(np.ones((1, 8), np.uint8)))[0, 0]


# ---- the decoder's mirror against the restatement ------------------------------------------------------------------------------------------

def _codes(rng, N):
    yield R.random_code(rng, N, 0)
    yield R.random_code(rng, N, N)
    yield R.random_code(rng, N)
    yield R.random_code(rng, N, N // 2)


@pytest.mark.parametrize("maxq", [1, 31, 126])
@pytest.mark.parametrize("n", range(1, 11))
def test_mirror_is_the_restatement_i8(q, n, maxq):
    rng = np.random.default_rng([n, maxq])
    N, F = 1 << n, 6
    for pos, mask in _codes(rng, N):
        llr = R.i8_inputs(rng, F, N, maxq)
        for fv in (None, rng.integers(0, 2, (F, N), dtype=np.uint8)):
            out = q.polar_decode_host(n, pos, llr, None if fv is None else R.pack(fv), "i8", maxq, leaf=True)
            R.check_outputs(out, R.decode(llr, mask, fv, "i8", maxq), pos, N, mask, "n=%d K=%d" % (n, len(pos)))


def test_unsaturated_f_reaches_maxq_plus_one(q):
    """f(-32, -32) = +32 at maxq = 31: the left leaf of two received -32 holds 32"""
    out = q.polar_decode_host(1, [0, 1], np.full((1, 2), -32, np.int8), None, "i8", 31, leaf=True)
    assert out["leaf"][0].tolist() == [32, -32] and R.unpack(out["u"], 2)[0].tolist() == [0, 1]
    out = q.polar_decode_host(1, [0, 1], np.full((1, 2), -128, np.int8), None, "i8", 126, leaf=True)
    assert out["leaf"][0].tolist() == [127, -127]


@pytest.mark.parametrize("n", range(1, 11))
def test_mirror_is_the_restatement_f32(q, n):
    rng = np.random.default_rng([n, 77])
    N, F = 1 << n, 10
    for pos, mask in _codes(rng, N):
        llr = R.f32_inputs(rng, F, N)
        for fv in (None, rng.integers(0, 2, (F, N), dtype=np.uint8)):
            out = q.polar_decode_host(n, pos, llr, None if fv is None else R.pack(fv), "f32", leaf=True)
            R.check_outputs(out, R.decode(llr, mask, fv, "f32"), pos, N, mask, "n=%d K=%d" % (n, len(pos)))


def test_zero_and_negative_zero_decide_zero(q):
    llr = np.array([[0.0, -0.0, -0.0, 0.0]], np.float32)
    out = q.polar_decode_host(2, [0, 1, 2, 3], llr, None, "f32", leaf=True)
    assert not out["u"].any() and not out["x"].any()


def test_frozen_bits_outside_the_frozen_set_are_ignored(q):
    rng = np.random.default_rng(5)
    n, N = 6, 64
    pos, mask = R.random_code(rng, N, 20)
    llr = R.i8_inputs(rng, 4, N, 31)
    fv = rng.integers(0, 2, (4, N), dtype=np.uint8)
    a = q.polar_decode_host(n, pos, llr, R.pack(fv), "i8", 31)
    b = q.polar_decode_host(n, pos, llr, R.pack(fv * mask), "i8", 31)
    assert all(np.array_equal(a[k], b[k]) for k in a)


# ---- the published curve -----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fer_points(q):
    """per published point: (row, frames, block errors of the mirror, of the restatement on the first 400 frames, of the mirror on the same)"""
    out = []
    for k in range(5):
        row, pos, msg, rq = R.fer_point(k)
        info = R.info_bits(q.polar_decode_host(10, pos, rq, None, "i8", 31)["info"], len(pos))
        bad = (info != msg).any(axis=1)
        mask = np.ones(1024, bool)
        mask[pos] = False
        u, _, _ = R.decode(rq[:400], mask, None, "i8", 31)
        out.append((row, len(msg), int(bad.sum()), int((u[:, pos] != msg[:400]).any(axis=1).sum()), int(bad[:400].sum())))
    return out


@pytest.mark.parametrize("k", range(5))
def test_published_sc_curve_on_the_mirror(fer_points, k):
    row, F, errors, _, _ = fer_points[k]
    fer = errors / F
    print("Eb/N0 %.1f dB: %d / %d = %.5f, published %.4f (%d / %d), band +-%.5f" % (row[0], errors, F, fer, row[1], row[3], row[5], R.fer_band(row, F)))
    assert abs(fer - row[1]) <= R.fer_band(row, F)


def test_mirror_counts_the_restatements_errors(fer_points):
    """a 2 000-frame subset (400 frames of each point): the same block errors, exactly"""
    assert sum(p[3] for p in fer_points) > 0
    assert [p[3] for p in fer_points] == [p[4] for p in fer_points]


# ---- the reconciliation form -------------------------------------------------------------------------------------------------------------

def test_reconciliation_form(q):
    """Alice's encode(x) on the frozen positions is her syndrome; Bob's SC with those positions pinned re-encodes to her key"""
    pos, x, frozen, llr = R.recon_frames(1)
    out = q.polar_decode_host(10, pos, llr, frozen, "f32")
    good = int((out["x"] == R.pack(x)).all(axis=1).sum())
    print("reconciled %d of %d" % (good, len(x)))
    assert good >= 1995
    assert np.array_equal(q.polar_encode_host(10, out["u"]), out["x"])


# ---- argument checks ---------------------------------------------------------------------------------------------------------------------

def _status(q, fn, *args, **kw):
    with pytest.raises(q.QldpcError) as e:
        fn(*args, **kw)
    assert str(e.value)
    return e.value.status


def test_argument_checks(q):
    ESIZE, EINVAL = -6, -1
    z = lambda n, dt=np.int8: np.zeros((1, 1 << n), dt)
    assert _status(q, q.polar_decode_host, 0, [], np.zeros((1, 1), np.int8)) == ESIZE
    assert _status(q, q.polar_decode_host, 21, [], np.zeros((1, 1), np.int8)) == ESIZE
    assert _status(q, q.polar_encode_host, 0, np.zeros((1, 1), np.uint32)) == ESIZE
    assert _status(q, q.polar_encode_host, 21, np.zeros((1, 1), np.uint32)) == ESIZE
    assert _status(q, q.polar_encode_host, 6, np.zeros((1, 1), np.uint32)) == ESIZE                  # a row of 64 bits has two words
    assert _status(q, q.polar_decode_host, 3, [0, 8], z(3)) == ESIZE                                # a position at N
    assert _status(q, q.polar_decode_host, 3, [-1], z(3)) == ESIZE
    assert _status(q, q.polar_decode_host, 3, [1, 2, 1], z(3)) == EINVAL                            # a position twice
    assert _status(q, q.polar_decode_host, 2, [0, 1, 2, 3, 0], z(2)) == ESIZE                       # more positions than bits
    assert _status(q, q.polar_decode_host, 3, [1], z(3), maxq=127) == ESIZE                         # f gives maxq + 1 = 128
    assert _status(q, q.polar_decode_host, 3, [1], z(3), maxq=0) == ESIZE
    assert _status(q, q.polar_decode_host, 3, [1], z(3), messages="f16") == EINVAL
    assert _status(q, q.polar_decode_host, 3, [1], z(2)) == ESIZE                                   # llr rows of the wrong length
    assert _status(q, q.polar_decode_host, 3, [1], z(3), frozen=np.zeros((2, 1), np.uint32)) == ESIZE
    assert "int8" in str(pytest.raises(q.QldpcError, q.polar_decode_host, 3, [1], z(3), maxq=127).value)
    # the float messages ignore maxq
    q.polar_decode_host(3, [1], z(3, np.float32), messages="f32", maxq=127)
    # the raw calls: a NULL row, a negative frame count, messages neither value
    L = q._L
    assert L.qldpc_polar_decode_host(3, 0, None, 0, 31, 1, None, None, None, None, None, None) == EINVAL
    assert L.qldpc_polar_decode_host(3, 0, None, 0, 31, -1, None, None, None, None, None, None) == EINVAL
    assert L.qldpc_polar_decode_host(3, 0, None, 2, 31, 0, None, None, None, None, None, None) == EINVAL
    assert L.qldpc_polar_decode_host(3, 1, None, 0, 31, 0, None, None, None, None, None, None) == ESIZE
    assert L.qldpc_polar_encode_host(3, 1, None, None) == EINVAL
    assert L.qldpc_polar_encode_host(3, -1, None, None) == EINVAL
    assert L.qldpc_polar_decode_host(3, 0, None, 0, 31, 0, None, None, None, None, None, None) == 0    # no frames: nothing to do


def test_create_checks_its_arguments_without_a_device(q):
    """every refusal of qldpc_polar_create comes before the first HIP call, so it is the same on a machine without a GPU"""
    ESIZE, EINVAL = -6, -1
    make = lambda *a, **kw: q.Polar(*a, **kw)
    assert _status(q, make, 0, []) == ESIZE
    assert _status(q, make, 21, []) == ESIZE
    assert _status(q, make, 4, [16]) == ESIZE
    assert _status(q, make, 4, [3, 3]) == EINVAL
    assert _status(q, make, 4, [3], maxq=127) == ESIZE
    assert _status(q, make, 4, [3], maxq=0) == ESIZE
    assert _status(q, make, 4, [3], max_frames=0) == EINVAL
    assert _status(q, make, 4, [3], messages="bf16") == EINVAL
    assert "126" in str(pytest.raises(q.QldpcError, make, 4, [3], maxq=127).value)


# ---- polar_pw_order ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 5, 8, 10])
def test_pw_order(q, n):
    N = 1 << n
    order = q.polar_pw_order(n)
    assert sorted(order.tolist()) == list(range(N)) and order[0] == 0 and order[-1] == N - 1
    rank = np.empty(N, np.int64)
    rank[order] = np.arange(N)
    i = np.arange(N)
    for j in range(n):                                             # adding a set bit never lowers the rank; by transitivity every subset relation
        lower = i[(i >> j) & 1 == 0]
        assert (rank[lower] < rank[lower | (1 << j)]).all()


def test_golden_reliability_sequence(q):
    seq = R.nr_order(1024)
    assert sorted(seq.tolist()) == list(range(1024)) and seq[0] == 0 and seq[-1] == 1023
    assert sorted(R.nr_order(64).tolist()) == list(range(64))


# ---- the sanitizer program ---------------------------------------------------------------------------------------------------------------

def test_host_code_under_asan_ubsan(tmp_path):
    """the mirrors at every size up to 2^12 with every row malloc'ed at its exact size, each output alone and all together, and every
    refusal, as a stand-alone program (nothing loaded into Python is sanitised)"""
    exe = str(tmp_path / "polar_sanitize")
    csrc = os.path.join(ROOT, "qcrypto-ldpc_amd", "csrc")
    subprocess.check_call(["gcc", "-std=gnu11", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                           "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-o", exe, os.path.join(ROOT, "tests", "c", "polar_sanitize.c"),
                           os.path.join(csrc, "qldpc_polar_host.c"), "-lm"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "sanitizer pass ok" in r.stdout, r.stdout + r.stderr
