"""CPU suite of the polar list decoder: the host mirror (qldpc_polar_list_decode_host) against the numpy restatement of tests/polar_list_ref.py bit
for bit, its identity with the SC mirror at list size 1, the CRC, the refusals, the published list-4 curve of the reference's fixed-point script,
the reconciliation form against SC, and the sanitizer program.  No GPU, no device."""
import os
import subprocess

import numpy as np
import pytest

import polar_list_ref as LR
import polar_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LISTS = (1, 2, 4, 8)


def _crc_for(rng, K):
    """a CRC that fits K information bits: CRC 11 where it does, a short one below, none at K = 0"""
    if K >= 11:
        return LR.CRC11
    if K == 0:
        return 0, 0
    crc_len = int(rng.integers(1, K + 1))
    return crc_len, int(rng.integers(0, 1 << crc_len))


def _case(q, rng, n, L, messages, maxq, pos, mask, F, what):
    N = 1 << n
    llr = R.i8_inputs(rng, F, N, maxq) if messages == "i8" else R.f32_inputs(rng, F, N)
    crc_len, crc_poly = _crc_for(rng, len(pos))
    for fv in (None, rng.integers(0, 2, (F, N), dtype=np.uint8)):
        crc = rng.integers(0, 1 << crc_len, F).astype(np.uint32) if crc_len and fv is not None else None
        ref = LR.decode(llr, mask, fv, messages, maxq, L, pos, crc_len, crc_poly, crc)
        out = q.polar_list_decode_host(n, pos, llr, None if fv is None else R.pack(fv), crc, messages, maxq, L, crc_len, crc_poly)
        assert set(out) == set(q.LIST_OUTPUTS)
        LR.check_outputs(out, ref, what)


# ---- the mirror against the restatement ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("messages", ["i8", "f32"])
@pytest.mark.parametrize("L", LISTS)
@pytest.mark.parametrize("n", range(1, 9))
def test_mirror_is_the_restatement(q, n, L, messages):
    """random codes (K = 0, K = N, a random K, K = N / 2), random frozen values and expected remainders; the inputs' all-zero and +-|LLR| frames
    force ties in the metrics"""
    maxq = (1, 31, 126)[(n + L) % 3]
    rng = np.random.default_rng([n, L, messages == "i8"])
    N = 1 << n
    for K in (0, N, None, N // 2):
        pos, mask = R.random_code(rng, N, K)
        _case(q, rng, n, L, messages, maxq, pos, mask, 10, "n=%d L=%d %s K=%d maxq=%d" % (n, L, messages, len(pos), maxq))


@pytest.mark.parametrize("messages", ["i8", "f32"])
@pytest.mark.parametrize("n", [1, 3, 5, 6, 8, 10])
def test_list_of_one_is_the_sc_decoder(q, n, messages):
    rng = np.random.default_rng([n, messages == "i8", 1])
    N, F = 1 << n, 12
    pos, _ = R.random_code(rng, N)
    llr = R.i8_inputs(rng, F, N, 31) if messages == "i8" else R.f32_inputs(rng, F, N)
    fz = R.pack(rng.integers(0, 2, (F, N), dtype=np.uint8))
    for frozen in (None, fz):
        sc = q.polar_decode_host(n, pos, llr, frozen, messages, 31)
        out = q.polar_list_decode_host(n, pos, llr, frozen, None, messages, 31, 1)
        assert all(np.array_equal(out[k], sc[k]) for k in ("u", "info", "x"))
        assert not out["pick"].any() and np.array_equal(out["list_x"][:, 0], sc["x"])


# ---- edge cases ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("messages", ["i8", "f32"])
def test_fewer_information_bits_than_the_list_needs(q, messages):
    """n_info < log2 L: 2^n_info live paths, the other slots all ones / +inf and zero rows"""
    rng = np.random.default_rng(3)
    n, N, F = 6, 64, 10
    for K, L in ((1, 4), (2, 8), (1, 8), (0, 8)):
        pos, mask = R.random_code(rng, N, K)
        _case(q, rng, n, L, messages, 31, pos, mask, F, "K=%d L=%d" % (K, L))
        llr = R.i8_inputs(rng, F, N, 31) if messages == "i8" else R.f32_inputs(rng, F, N)
        out = q.polar_list_decode_host(n, pos, llr, None, None, messages, 31, L)
        dead = out["metric"][:, 1 << K:]
        assert (dead.view(np.uint32) == (0xffffffff if messages == "i8" else 0x7f800000)).all() and not out["list_x"][:, 1 << K:].any()


@pytest.mark.parametrize("crc_len,crc_poly", [(7, 0x09), (32, 0x04C11DB7)])
def test_crc_as_long_as_the_information_word_and_of_32_bits(q, crc_len, crc_poly):
    """crc_len = n_info, and crc_len = 32 (no bit is lost in the shift)"""
    rng = np.random.default_rng(crc_len)
    n, N, F = 7, 128, 10
    for K in (crc_len, 40):
        pos, mask = R.random_code(rng, N, K)
        llr = R.i8_inputs(rng, F, N, 31)
        # expected remainders that single out a path other than the first for some frames: those of the restatement's last path
        free = LR.decode(llr, mask, None, "i8", 31, 4, pos, crc_len, crc_poly)
        u_last = np.stack([R.encode(free["list_x"][f, 3][None])[0] for f in range(F)])
        crc = LR.crc_bits(u_last[:, pos], crc_len, crc_poly)
        ref = LR.decode(llr, mask, None, "i8", 31, 4, pos, crc_len, crc_poly, crc)
        out = q.polar_list_decode_host(n, pos, llr, None, crc, "i8", 31, 4, crc_len, crc_poly)
        LR.check_outputs(out, ref, "crc_len=%d K=%d" % (crc_len, K))
        assert (out["pick"] >= 0).all() and (out["pick"] > 0).any()


# ---- the CRC -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("crc_len,crc_poly", [(0, 0), (1, 1), (5, 0x05), (11, 0x621), (16, 0x1021), (24, 0x864CFB), (32, 0x04C11DB7)])
def test_crc_host(q, crc_len, crc_poly):
    rng = np.random.default_rng(crc_len)
    for n_bits in (0, 1, 31, 32, 33, 500):
        bits = rng.integers(0, 2, (9, n_bits), dtype=np.uint8)
        rows = R.pack(bits) if n_bits else np.zeros((9, 0), np.uint32)
        got = q.polar_crc_host(crc_len, crc_poly, rows, n_bits)
        assert np.array_equal(got, LR.crc_bits(bits, crc_len, crc_poly))
        if crc_len and n_bits:
            word = np.concatenate([bits, LR.crc_word(got, crc_len)], axis=1)          # an appended CRC gives remainder 0 ..
            assert not q.polar_crc_host(crc_len, crc_poly, R.pack(word), n_bits + crc_len).any()
            word[np.arange(9), rng.integers(0, n_bits + crc_len, 9)] ^= 1              # .. and a single flipped bit does not
            assert q.polar_crc_host(crc_len, crc_poly, R.pack(word), n_bits + crc_len).all()


def test_crc11_of_the_reference_by_hand(q):
    """x^11 + x^10 + x^9 + x^5 + 1: the remainder of the message 1 (one bit) is the polynomial's low part, of x it is that shifted and reduced"""
    assert q.polar_crc_host(11, 0x621, np.array([[0x80000000]], np.uint32), 1)[0] == 0x621
    assert q.polar_crc_host(11, 0x621, np.array([[0x80000000]], np.uint32), 2)[0] == ((0x621 << 1) & 0x7ff) ^ 0x621


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------

def _status(q, fn, *args, **kw):
    with pytest.raises(q.QldpcError) as e:
        fn(*args, **kw)
    assert str(e.value)
    return e.value.status


def test_argument_checks(q):
    ESIZE, EINVAL = -6, -1
    z = lambda n, dt=np.int8: np.zeros((1, 1 << n), dt)
    dec = q.polar_list_decode_host
    assert _status(q, dec, 0, [], np.zeros((1, 1), np.int8)) == ESIZE
    assert _status(q, dec, 17, [], np.zeros((1, 1), np.int8)) == ESIZE                       # the SC decoder goes to 2^20, the list to 2^16
    for L in (0, 3, 5, 6, 7, 9, 16, -1):
        assert _status(q, dec, 3, [1], z(3), list_size=L) == ESIZE
    assert _status(q, dec, 3, [1, 2], z(3), crc_len=-1) == ESIZE
    assert _status(q, dec, 6, list(range(40)), z(6), crc_len=33) == ESIZE
    assert _status(q, dec, 3, [1, 2], z(3), crc_len=3, crc_poly=1) == ESIZE                   # a CRC longer than the information word
    assert _status(q, dec, 3, [1, 2, 3], z(3), crc_len=3, crc_poly=8) == ESIZE               # x^crc_len is implied, not given
    assert _status(q, dec, 3, [1, 2, 3], z(3), crc_len=0, crc_poly=1) == ESIZE
    assert _status(q, dec, 3, [1, 2, 3], z(3), crc=np.zeros(1, np.uint32), crc_len=0) == EINVAL   # an expected remainder without a CRC
    assert _status(q, dec, 3, [0, 8], z(3)) == ESIZE
    assert _status(q, dec, 3, [1, 2, 1], z(3)) == EINVAL
    assert _status(q, dec, 3, [1], z(3), maxq=127) == ESIZE
    assert _status(q, dec, 3, [1], z(3), messages="f16") == EINVAL
    assert _status(q, dec, 3, [1], z(2)) == ESIZE
    assert _status(q, dec, 3, [1], z(3), frozen=np.zeros((2, 1), np.uint32)) == ESIZE
    assert _status(q, dec, 3, [1], z(3), crc=np.zeros(2, np.uint32), crc_len=1, crc_poly=1) == ESIZE
    assert _status(q, q.polar_crc_host, 33, 0, np.zeros((1, 1), np.uint32), 3) == ESIZE
    assert _status(q, q.polar_crc_host, -1, 0, np.zeros((1, 1), np.uint32), 3) == ESIZE
    assert _status(q, q.polar_crc_host, 4, 16, np.zeros((1, 1), np.uint32), 3) == ESIZE
    assert _status(q, q.polar_crc_host, 4, 3, np.zeros((1, 2), np.uint32), 3) == ESIZE
    L = q._L
    nul = (None,) * 9
    assert L.qldpc_polar_list_decode_host(3, 0, None, 0, 31, 4, 0, 0, 1, *nul) == EINVAL          # frames without an llr row
    assert L.qldpc_polar_list_decode_host(3, 0, None, 0, 31, 4, 0, 0, -1, *nul) == EINVAL
    assert L.qldpc_polar_list_decode_host(3, 0, None, 2, 31, 4, 0, 0, 0, *nul) == EINVAL
    assert L.qldpc_polar_list_decode_host(3, 0, None, 0, 31, 4, 0, 0, 0, *nul) == 0                # no frames: nothing to do
    assert L.qldpc_polar_crc_host(4, 3, -1, 0, None, None) == EINVAL
    assert L.qldpc_polar_crc_host(4, 3, 3, 1, None, None) == EINVAL
    assert L.qldpc_polar_crc_host(4, 3, 3, 0, None, None) == 0


def test_create_checks_its_arguments_without_a_device(q):
    """every refusal of qldpc_polar_list_create comes before the first HIP call, so it is the same on a machine without a GPU"""
    ESIZE, EINVAL = -6, -1
    make = lambda *a, **kw: q.PolarList(*a, **kw)
    assert _status(q, make, 0, []) == ESIZE
    assert _status(q, make, 17, []) == ESIZE
    assert _status(q, make, 4, [3], list_size=3) == ESIZE
    assert _status(q, make, 4, [3], list_size=16) == ESIZE
    assert _status(q, make, 4, [3], crc_len=2, crc_poly=1) == ESIZE
    assert _status(q, make, 4, [3, 4], crc_len=2, crc_poly=4) == ESIZE
    assert _status(q, make, 4, [3], crc_len=33) == ESIZE
    assert _status(q, make, 4, [16]) == ESIZE
    assert _status(q, make, 4, [3, 3]) == EINVAL
    assert _status(q, make, 4, [3], maxq=127) == ESIZE
    assert _status(q, make, 4, [3], max_frames=0) == EINVAL
    assert _status(q, make, 4, [3], messages="bf16") == EINVAL


# ---- the published curve -------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def list_points(q):
    """per published point of the list-4 curve: (row, frames, block errors, block errors among the frames a path was picked for)"""
    out = []
    for k in range(4):
        row, pos, msg, rq = LR.list_point(k)
        got = q.polar_list_decode_host(10, pos, rq, None, None, "i8", 31, 4, *LR.CRC11, want=("info", "pick"))
        bad = (R.info_bits(got["info"], len(pos))[:, :msg.shape[1]] != msg).any(axis=1)
        out.append((row, len(msg), int(bad.sum()), int((bad & (got["pick"] >= 0)).sum())))
    return out


@pytest.mark.parametrize("k", range(4))
def test_published_list_curve_on_the_mirror(list_points, k):
    row, F, errors, _ = list_points[k]
    fer = errors / F
    print("Eb/N0 %.2f dB: %d / %d = %.5f, published %.4f (%d / %d), band +-%.5f" % (row[0], errors, F, fer, row[1], row[3], row[5], R.fer_band(row, F)))
    assert abs(fer - row[1]) <= R.fer_band(row, F)


@pytest.mark.parametrize("k", [2, 3])
def test_no_undetected_error_on_the_published_frames(list_points, k):
    """a frame whose picked path passed the CRC is the message sent"""
    print("Eb/N0 %.2f dB: %d block errors with a path picked" % (list_points[k][0][0], list_points[k][3]))
    assert list_points[k][3] == 0


# ---- the reconciliation form ---------------------------------------------------------------------------------------------------------------

def recon_case(q):
    """LR.recon_frames and Alice's CRC 11 of her information word, from u = encode(x) as her frozen values are -> (pos, x, frozen rows, crc, llr)"""
    pos, x, frozen, llr = LR.recon_frames()
    crc = q.polar_crc_host(*LR.CRC11, R.pack(R.encode(x)[:, pos]), len(pos))
    return pos, x, frozen, crc, llr


def test_reconciliation_form_beats_sc(q):
    pos, x, frozen, crc, llr = recon_case(q)
    want = R.pack(x)
    sc = q.polar_list_decode_host(10, pos, llr, frozen, None, "f32", 31, 1, want=("x",))
    l4 = q.polar_list_decode_host(10, pos, llr, frozen, crc, "f32", 31, 4, *LR.CRC11, want=("x", "pick"))
    fail_sc = int((sc["x"] != want).any(axis=1).sum())
    wrong4 = (l4["x"] != want).any(axis=1)
    fail_4 = int((wrong4 | (l4["pick"] < 0)).sum())
    accepted_wrong = int((wrong4 & (l4["pick"] >= 0)).sum())
    print("QBER 0.06, 2 000 keys: SC fails %d, list 4 + CRC 11 fails %d, wrong keys accepted %d" % (fail_sc, fail_4, accepted_wrong))
    assert fail_sc > 0 and 2 * fail_4 < fail_sc
    assert accepted_wrong == 0


# ---- the sanitizer program -----------------------------------------------------------------------------------------------------------------

def test_host_code_under_asan_ubsan(tmp_path):
    """the list mirror at every size up to 2^9 and every list size with every row malloc'ed at its exact size, each output alone and all together,
    and every refusal, as a stand-alone program (nothing loaded into Python is sanitised)"""
    exe = str(tmp_path / "polar_list_sanitize")
    csrc = os.path.join(ROOT, "qcrypto-ldpc_amd", "csrc")
    subprocess.check_call(["gcc", "-std=gnu11", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                           "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-o", exe, os.path.join(ROOT, "tests", "c", "polar_list_sanitize.c"),
                           os.path.join(csrc, "qldpc_polar_list_host.c"), os.path.join(csrc, "qldpc_polar_host.c"), "-lm"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "sanitizer pass ok" in r.stdout, r.stdout + r.stderr
