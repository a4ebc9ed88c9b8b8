"""CPU suite: the keyed tag of the sessions' verify step (qldpc_recon_*_tagged) without a device.  The host mirrors run the functions of
qcrypto-ldpc_amd/csrc/qldpc_recon_tag_core.h over the kernels' own decomposition (the CRC's chunks, Horner per lane, the fold tree); the reference is
tests/polyhash_ref.py, the Horner loop of the definition in Python integers.  Equality is exact."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import polyhash_ref as R
from recon_tag_ref import EDECODE, OK, batch, check_verdict, crc_collision, expected
from recon_tag_ref import hash_keys as _hash_keys, masked as _masked, words as _words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = R.P
LANES = [1, 2, 64, 256, 1024]
# 255, 256 and 257 words cross the chunk boundary of 256 lanes (c = 1, then c = 2 with 255 zero words in front); 2^18 bits is the sessions' maximum
BITS = [1, 31, 32, 33, 64, 255 * 32, 256 * 32, 257 * 32, 8191, 52429, 1 << 18]


def test_tag_equals_reference_polyhash_and_itself(q):
    """every length x every hash key x every lane count, the words keeping whatever lies in their tail bits"""
    rng = np.random.default_rng(18)
    keys = _hash_keys(rng)
    assert [R.key_of(*k) for k in keys[:5]] == [0, 1, 0, P - 1, 0]
    for bits in BITS:
        w = _words(rng, (bits + 31) // 32)
        for hk in keys:
            want = R.tag(w, bits, hk).tolist()
            assert q.polyhash_host(w, bits, hk).tolist() == want
            for lanes in LANES:
                assert q.recon_tag_host(w, bits, hk, lanes).tolist() == want, (bits, hk, lanes)


def test_chunks_cross_the_lane_boundary(q):
    """all-ones words at 255, 256, 257 words: a dropped or doubled chunk word would show"""
    hk = R.key_words(0x0123456789ABCDEF)
    for W in (255, 256, 257, 511, 513):
        w = np.full(W, 0xFFFFFFFF, np.uint32)
        assert R.tag(w, 32 * W, hk).tolist() == R.as_words(R.closed_all_ones(32 * W, R.key_of(*hk))).tolist()
        for lanes in LANES:
            assert q.recon_tag_host(w, 32 * W, hk, lanes).tolist() == R.tag(w, 32 * W, hk).tolist()


def test_garbage_past_key_bits_changes_nothing(q):
    rng = np.random.default_rng(19)
    hk = R.key_words(int(rng.integers(1, 1 << 62)))
    for bits in (1, 31, 33, 1000, 255 * 32 + 5, 257 * 32 - 1):
        w = _words(rng, (bits + 31) // 32)
        g = w.copy()
        g[-1] ^= np.uint32((1 << (32 - bits % 32)) - 1)          # every bit past key_bits flipped
        assert (g != w).any()
        long = np.concatenate([g, _words(rng, 5)])                # and words past the block
        for lanes in (1, 256):
            assert q.recon_tag_host(w, bits, hk, lanes).tolist() == q.recon_tag_host(g, bits, hk, lanes).tolist() == q.recon_tag_host(long, bits, hk, lanes).tolist() \
                == R.tag(w, bits, hk).tolist()


def test_sensitivity(q):
    """asserted on the reference first: a flip of any single bit below key_bits changes the tag, and so does another length over an all-zero block"""
    rng = np.random.default_rng(20)
    hk = R.key_words(int(rng.integers(1, 1 << 62)) | 1)
    for bits in (1, 33, 70, 1000):
        w = _words(rng, (bits + 31) // 32)
        base = R.tag(w, bits, hk).tolist()
        assert q.recon_tag_host(w, bits, hk).tolist() == base
        for p in range(bits):
            f = w.copy()
            f[p >> 5] ^= np.uint32(0x80000000 >> (p & 31))
            assert R.tag(f, bits, hk).tolist() != base
            assert q.recon_tag_host(f, bits, hk).tolist() == R.tag(f, bits, hk).tolist()
    zero = np.zeros(4, np.uint32)
    for a, b in ((1, 2), (32, 33), (64, 96), (97, 128)):
        assert R.tag(zero, a, hk).tolist() != R.tag(zero, b, hk).tolist()
        assert q.recon_tag_host(zero, a, hk).tolist() == R.tag(zero, a, hk).tolist() != q.recon_tag_host(zero, b, hk).tolist() == R.tag(zero, b, hk).tolist()


def verify_host(q, B):
    return q.recon_verify_tag_host(B["out"], B["keys"], B["key_bits"], B["crc_want"], B["ok"], B["iters"], B["hash_keys"])


@pytest.mark.parametrize("r", [1, 2, 4])
@pytest.mark.parametrize("shared", [True, False])
def test_verify_mirror_on_synthetic_batches(q, r, shared):
    rng = np.random.default_rng(21 + r)
    B = batch(q, rng, [1, 33, 1000, 255 * 32 + 5, 256 * 32, 257 * 32 - 1, 65, 2000, 31], r, shared, collide=(7,))
    want = expected(q, B)
    assert sorted(set(want["status"].tolist())) == [EDECODE, OK] and (want["status"] == OK).sum() >= 4
    got = verify_host(q, B)
    check_verdict(got, want)
    bad = want["status"] != OK
    assert not got["tags"][bad].any() and got["tags"][~bad].any(axis=1).all()      # nothing is disclosed for a bad block
    assert not got["corrected"][bad].any()


def test_the_crc_passes_a_wrong_key_and_the_tag_does_not(q):
    """the reason the tag exists: a decoded row that differs from Alice's key by a difference the CRC does not see is accepted by the verify step -- and
    its tag under a random key is not Alice's"""
    rng = np.random.default_rng(22)
    for bits in (64, 1000, 52429):
        W = (bits + 31) // 32
        K = _words(rng, W)
        d = crc_collision(q, K, bits, rng)
        wrong = K ^ d
        assert (_masked(wrong, bits) != _masked(K, bits)).any()
        assert q.crc32_words(wrong, bits) == q.crc32_words(K, bits)
        hk = R.key_words(int(rng.integers(1, 1 << 62)))
        got = q.recon_verify_tag_host(wrong.reshape(1, W), _words(rng, W).reshape(1, W), [bits], [q.crc32_words(K, bits)], [1], [5], hk)
        assert got["status"].tolist() == [OK] and (got["keys"][0] == _masked(wrong, bits)).all()      # the CRC passes a wrong key
        assert got["tags"][0].tolist() == R.tag(wrong, bits, hk).tolist() != R.tag(K, bits, hk).tolist()
        assert q.recon_tag_host(K, bits, hk).tolist() == R.tag(K, bits, hk).tolist()


def test_special_hash_keys_in_the_verdict(q):
    rng = np.random.default_rng(23)
    for hk in _hash_keys(rng):
        B = batch(q, rng, [33, 1000, 64, 257 * 32 - 1], 1, True)
        B["hash_keys"] = hk
        check_verdict(verify_host(q, B), expected(q, B))


def test_refusals(q):
    rng = np.random.default_rng(24)
    w, hk = np.zeros(2, np.uint32), np.array([1, 2], np.uint32)
    for args in ((w, 0, hk), (w, 65, hk), (w, 64, hk[:1]), (w, 64, hk, 0), (w, 64, hk, 3), (w, 64, hk, 1 << 21)):
        with pytest.raises(q.QldpcError):
            q.recon_tag_host(*args)
    B = batch(q, rng, [33, 64, 40], 1, True)
    for field, value in (("hash_keys", np.zeros(0, np.uint32)), ("hash_keys", np.zeros(10, np.uint32)), ("hash_keys", np.zeros(3, np.uint32)),
                         ("hash_keys", np.zeros((2, 2), np.uint32)), ("key_bits", np.array([33, 64, 97], np.int32)), ("key_bits", np.array([33, 0, 40], np.int32)),
                         ("ok", np.ones(2, np.int32))):
        with pytest.raises(q.QldpcError):
            verify_host(q, dict(B, **{field: value}))
    up = C.POINTER(C.c_uint32)
    tag = np.full(2, 7, np.uint32)
    assert q._L.qldpc_recon_tag_host(None, 64, hk.ctypes.data_as(up), 256, tag.ctypes.data_as(up)) == -1 and tag.tolist() == [7, 7]


def test_leaked_bits(q):
    m = q.ReconMsg(rate_index=1, key_bits=1000, code_k=1024, code_m=440, crc32=0, n_punct=40)
    assert q.Recon.leaked_bits(m) == 432
    for r in (1, 2, 3, 4):
        assert q.recon_leaked_bits_tagged(m, r) == 432 + 61 * r == q.Recon.leaked_bits(m) + q.polyhash_leaked_bits(r)
    for bad in (0, 5, -1):
        with pytest.raises(q.QldpcError):
            q.recon_leaked_bits_tagged(m, bad)
        assert q._L.qldpc_recon_leaked_bits_tagged(C.byref(m), bad) == 0
    assert q._L.qldpc_recon_leaked_bits_tagged(None, 1) == 0


def test_host_code_under_asan_ubsan(tmp_path):
    """the two mirrors over the shapes above with every buffer malloc'ed at its exact size, as a stand-alone program (nothing loaded into Python is
    sanitised)"""
    exe = str(tmp_path / "recon_tag_sanitize")
    csrc = os.path.join(ROOT, "qcrypto-ldpc_amd", "csrc")
    subprocess.check_call(["gcc", "-std=gnu11", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                           "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-o", exe, os.path.join(ROOT, "tests", "c", "recon_tag_sanitize.c"),
                           os.path.join(csrc, "qldpc_recon_tag_host.c"), "-lm"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "sanitizer pass ok" in r.stdout, r.stdout + r.stderr
