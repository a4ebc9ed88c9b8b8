"""CPU suite: the error-verification hash (qldpc_polyhash_*) without a device.  The host mirror runs the functions of
qcrypto-ldpc_amd/csrc/qldpc_polyhash_core.h over the kernels' own decomposition (tiles, virtual lanes, fast and checked rows, power tables, the
fold of the partials); the reference is tests/polyhash_ref.py, the Horner loop of the definition in Python integers.  Equality is exact."""
import os
import subprocess

import numpy as np
import pytest

import polyhash_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = R.P
LANES = [1, 2, 3, 64, 256, 1000]
TILES = [0, 1024]


def _words(rng, bits, ones):
    W = (bits + 31) // 32
    return np.full(W, 0xFFFFFFFF, np.uint32) if ones else rng.integers(0, 1 << 32, W, dtype=np.uint64).astype(np.uint32)


def test_pinned_vectors(q):
    """two tags computed from the definition, fixed here: a short ragged block, and 2^24 ones under k = p - 1 (the geometric series)"""
    w1 = np.array([0xDEADBEEF, 0x01234567, 0xFFFFFFFF], np.uint32)
    k1 = np.array([0x01234567, 0x89ABCDEF], np.uint32)
    assert R.tag(w1, 70, k1).tolist() == [0x183DC405, 0x2969F83A]
    n2 = 1 << 24
    w2 = np.full(n2 // 32, 0xFFFFFFFF, np.uint32)
    k2 = np.array([0xFFFFFFFF, 0xFFFFFFFE], np.uint32)
    assert R.key_of(*k2) == P - 1
    assert R.as_words(R.closed_all_ones(n2, P - 1)).tolist() == [0x1FFFFFFF, 0xFEFFFFFF]
    assert R.tag(w2, n2, k2).tolist() == [0x1FFFFFFF, 0xFEFFFFFF]
    for lanes in (1, 256):
        for tile in TILES:
            assert q.polyhash_host(w1, 70, k1, lanes, tile).tolist() == [0x183DC405, 0x2969F83A]
            assert q.polyhash_host(w2, n2, k2, lanes, tile).tolist() == [0x1FFFFFFF, 0xFEFFFFFF]


def test_mirror_equals_reference_at_every_edge(q):
    """every edge length x every edge key x random and all-ones words x every lane count x both tiles; the words keep whatever lies in
    their tail bits, which the reference masks"""
    rng = np.random.default_rng(61)
    keys = R.edge_keys(rng)
    assert [R.key_of(k >> 32, k) for k in keys[:7]] == [0, 1, 2, P - 1, 0, 0, 0]
    n = 0
    for bits in R.EDGE_BITS:
        for ones in (False, True):
            w = _words(rng, bits, ones)
            for k64 in keys:
                hk = R.key_words(k64)
                want = R.tag(w, bits, hk).tolist()
                for lanes in LANES:
                    for tile in TILES:
                        assert q.polyhash_host(w, bits, hk, lanes, tile).tolist() == want, (bits, ones, hex(k64), lanes, tile)
                        n += 1
    assert n == len(R.EDGE_BITS) * 2 * 8 * len(LANES) * len(TILES) and len(R.EDGE_BITS) == 36


def test_tail_bits_do_not_matter(q):
    rng = np.random.default_rng(7)
    hk = R.key_words(int(rng.integers(1, 1 << 62)))
    for bits in (1, 31, 33, 70, 32 * 1023 - 1, 32 * 1024 + 1):
        w = _words(rng, bits, False)
        g = w.copy()
        g[-1] ^= np.uint32((1 << (32 - bits % 32)) - 1)          # every bit past key_bits flipped
        assert (g != w).any()
        a, b = q.polyhash_host(w, bits, hk), q.polyhash_host(g, bits, hk)
        assert a.tolist() == b.tolist() == R.tag(w, bits, hk).tolist()
        long = np.concatenate([w, rng.integers(0, 1 << 32, 5, dtype=np.uint64).astype(np.uint32)])      # and words past the block
        assert q.polyhash_host(long, bits, hk).tolist() == a.tolist()


def test_length_is_hashed(q):
    """the same words under another key_bits give another tag: zero padding cannot collide (asserted on the reference first)"""
    rng = np.random.default_rng(8)
    hk = R.key_words(0x0123456789ABCDEF)
    zero = np.zeros(4, np.uint32)
    for a, b in ((1, 2), (32, 33), (64, 96), (97, 128)):
        assert R.tag(zero, a, hk).tolist() != R.tag(zero, b, hk).tolist()
        assert q.polyhash_host(zero, a, hk).tolist() == R.tag(zero, a, hk).tolist() != q.polyhash_host(zero, b, hk).tolist() == R.tag(zero, b, hk).tolist()
    w = _words(rng, 128, False)
    w[3] = 0
    assert R.tag(w, 96, hk).tolist() != R.tag(w, 128, hk).tolist()
    assert q.polyhash_host(w, 96, hk).tolist() != q.polyhash_host(w, 128, hk).tolist()


def test_field_multiply_and_key(q):
    rng = np.random.default_rng(9)
    edge = [0, 1, 2, (1 << 32) - 1, 1 << 32, (1 << 29) - 1, 1 << 29, P - 2, P - 1, P >> 1, 0x1FFFFFFF00000000, P, 1 << 61, (1 << 64) - 1]
    for a in edge:
        for b in edge:
            assert q.polyhash_mul(a, b) == a * b % P, (hex(a), hex(b))
    for _ in range(20000):
        a, b = int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2)), int(rng.integers(0, 1 << 63)) * 2 + int(rng.integers(0, 2))
        assert q.polyhash_mul(a, b) == a * b % P
    assert q.POLYHASH_PRIME == P
    for k64 in [0, 1, 2, P - 1, P, 1 << 61, (1 << 61) + 5, (1 << 64) - 1, (1 << 64) - 2] + [int(rng.integers(0, 1 << 63)) * 2 + 1 for _ in range(100)]:
        assert q.polyhash_key(k64 >> 32, k64 & 0xFFFFFFFF) == R.key_of(k64 >> 32, k64) == (0 if k64 & P == P else k64 & P)
    assert q.polyhash_key(0xFFFFFFFF, 0xFFFFFFFF) == 0 and q.polyhash_key(0x20000000, 0) == 0 and q.polyhash_key(0xFFFFFFFF, 0xFFFFFFFE) == P - 1


def test_bound_and_leak(q):
    import math
    for bits, r in ((1, 1), (32, 1), (33, 2), (52429, 1), (52429, 3), (1 << 24, 1), (1 << 24, 4)):
        W = (bits + 31) // 32
        assert abs(q.polyhash_bound_log2(bits, r) - r * (math.log2(W + 2) - 61)) < 1e-9
        assert q.polyhash_leaked_bits(r) == 61 * r
    assert -42.0 - 1e-4 < q.polyhash_bound_log2(1 << 24, 1) < -41.99 and -50.4 < q.polyhash_bound_log2(52429, 1) < -50.2
    for bad in ((0, 1), (8, 0), (8, 5)):
        with pytest.raises(q.QldpcError):
            q.polyhash_bound_log2(*bad)
    with pytest.raises(q.QldpcError):
        q.polyhash_leaked_bits(0)


def test_mirror_refusals(q):
    w, hk = np.zeros(2, np.uint32), np.array([1, 2], np.uint32)
    for args in ((w, 0, hk), (w, 65, hk), (w, 64, hk[:1]), (w, 64, hk, 0), (w, 64, hk, 256, 512), (w, 64, hk, 256, -1)):
        with pytest.raises(q.QldpcError):
            q.polyhash_host(*args)
    assert q.polyhash_host(w, 64, hk, 256, 8192).tolist() == q.polyhash_host(w, 64, hk).tolist() == R.tag(w, 64, hk).tolist()


def test_host_code_under_asan_ubsan(tmp_path):
    """the field arithmetic against 128-bit integers, the split of a tile into fast and checked rows, the doubling table and the mirror at
    every lane count and tile with every key malloc'ed at its exact size, as a stand-alone program (nothing loaded into Python is sanitised)"""
    exe = str(tmp_path / "polyhash_sanitize")
    csrc = os.path.join(ROOT, "qcrypto-ldpc_amd", "csrc")
    subprocess.check_call(["gcc", "-std=gnu11", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                           "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-o", exe, os.path.join(ROOT, "tests", "c", "polyhash_sanitize.c"),
                           os.path.join(csrc, "qldpc_polyhash_host.c"), "-lm"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "sanitizer pass ok" in r.stdout, r.stdout + r.stderr
