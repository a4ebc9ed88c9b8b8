"""The NTT method of the Toeplitz hash (QLDPC_TOEPLITZ_NTT), host suite: qldpc_toeplitz_ntt_host runs the pass kernels' own functions
(csrc/qldpc_toeplitz_ntt_core.h) over the same tiles and passes, so the arithmetic of the lanes is checked here without a device.  The
references are the direct method's host mirror and the numpy restatement of y_i = XOR_{j < n} x_j t_(i+j); every comparison is exact
equality of words."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE_N = (1, 31, 32, 33, 63, 64, 65, 1000, 4097)          # the lists of tests/test_toeplitz.py, restated
EDGE_M = (1, 31, 32, 33, 63, 64, 65, 257)
SMALL = 5                                                  # B of the small kernel instance
PASSES = (1, 2, SMALL, 0)
# n + m - 1 = 2^k and 2^k + 1 (k = 5: one pass of the small instance; 7: ragged two; 10: two; 11 and 13: ragged three; 9: one production
# pass, 10 and up: ragged two), n = 1, m > n
SHAPES = [(16, 17), (17, 17), (100, 29), (100, 30), (1000, 25), (1000, 26), (24, 1001), (1, 1), (1, 32), (1, 33), (1, 2048), (3, 2046),
          (3, 2047), (8000, 193), (8000, 194), (5, 700), (511, 2), (512, 1), (512, 2)]
P = 2013265921


def ref_bits(x, t):
    return (np.correlate(t.astype(np.int64), x.astype(np.int64), "valid") & 1).astype(np.uint8)


def draw(q, rng, n, m, garbage=True):
    """key bits, seed bits and their packed words, the unused tail bits of both last words set"""
    x, t = rng.integers(0, 2, n), rng.integers(0, 2, n + m - 1)
    key, seed = q.pack_bits(x), q.pack_bits(t)
    if garbage:
        key[-1] |= np.uint32((1 << ((-n) % 32)) - 1)
        seed[-1] |= np.uint32((1 << ((-(n + m - 1)) % 32)) - 1)
    return x, t, key, seed


def test_field_multiply_and_roots(q):
    assert q.TOEPLITZ_NTT_PRIME == P and (P - 1) % (1 << 25) == 0 and (1 << 24) < P < (1 << 31)
    rng = np.random.default_rng(7)
    fixed = [0, 1, P - 1, 1 << 16, 1 << 30]
    pairs = [(a, b) for a in fixed for b in fixed] + [(int(a), int(b)) for a, b in rng.integers(0, P, (4000, 2))]
    for a, b in pairs:
        assert q.toeplitz_ntt_mul(a, b) == a * b % P, (a, b)
    for k in range(26):
        r = q.toeplitz_ntt_root(k)
        assert 0 < r < P and pow(r, 1 << k, P) == 1, k
        if k:
            assert pow(r, 1 << (k - 1), P) == P - 1, k
    with pytest.raises(q.QldpcError):
        q.toeplitz_ntt_root(26)
    with pytest.raises(q.QldpcError):
        q.toeplitz_ntt_root(-1)


def test_transform_length(q):
    f = q.toeplitz_ntt_length
    assert f(1, 1) == 32 and f(16, 17) == 32 and f(17, 17) == 64 and f(56880, 41935) == 1 << 17
    assert f(1 << 24, 1 << 24) == 1 << 25 and f(1 << 24, 1) == 1 << 24 and f((1 << 24) - 1, 2) == 1 << 24
    for n, m in ((0, 10), (10, 0), (-3, 10), (10, -1), ((1 << 24) + 1, 1)):
        assert f(n, m) == 0
    for n, m in SHAPES:
        assert f(n, m) >= n + m - 1 and (f(n, m) == 32 or f(n, m) < 2 * (n + m - 1))


@pytest.mark.parametrize("n", EDGE_N)
def test_mirror_equals_the_direct_mirror_and_the_reference(q, n):
    rng = np.random.default_rng(n)
    for m in EDGE_M:
        x, t, key, seed = draw(q, rng, n, m)
        ref = q.pack_bits(ref_bits(x, t))
        assert (q.toeplitz_host(key, n, seed, m) == ref).all()
        for b in PASSES:
            got = q.toeplitz_ntt_host(key, n, seed, m, b)
            assert got.dtype == np.uint32 and got.shape == ref.shape and (got == ref).all(), (n, m, b)


@pytest.mark.parametrize("n,m", SHAPES)
def test_mirror_at_the_powers_of_two_and_one_past(q, n, m):
    rng = np.random.default_rng(n * 4099 + m)
    x, t, key, seed = draw(q, rng, n, m)
    ref = q.pack_bits(ref_bits(x, t))
    assert (q.toeplitz_host(key, n, seed, m) == ref).all()
    for b in PASSES + (3, 4, 7, 12):                        # exponents the pass size does not divide: a ragged pass
        assert (q.toeplitz_ntt_host(key, n, seed, m, b) == ref).all(), (n, m, b)


@pytest.mark.parametrize("n,m", [(33, 65), (1000, 257), (4097, 31), (31, 33)])
def test_tail_bits_are_ignored_and_the_output_tail_is_zero(q, n, m):
    rng = np.random.default_rng(n + m)
    x, t, key, seed = draw(q, rng, n, m, garbage=False)
    clean = q.toeplitz_ntt_host(key, n, seed, m)
    assert (clean == q.pack_bits(ref_bits(x, t))).all()
    key_g, seed_g = key.copy(), seed.copy()
    key_g[-1] |= np.uint32((1 << ((-n) % 32)) - 1)
    seed_g[-1] |= np.uint32((1 << ((-(n + m - 1)) % 32)) - 1)
    assert (key_g != key).any() or n % 32 == 0
    assert (seed_g != seed).any() or (n + m - 1) % 32 == 0
    for b in (0, SMALL, 2):
        assert (q.toeplitz_ntt_host(key_g, n, seed_g, m, b) == clean).all()
    # words past the rows are not part of the block either
    ones = np.uint32(0xFFFFFFFF)
    assert (q.toeplitz_ntt_host(np.concatenate([key_g, [ones]]), n, np.concatenate([seed_g, [ones, ones]]), m) == clean).all()
    if m % 32:
        assert int(clean[-1]) & ((1 << ((-m) % 32)) - 1) == 0
        full = q.toeplitz_ntt_host(np.full(key.size, 0xFFFFFFFF, np.uint32), n, np.full(seed.size, 0xFFFFFFFF, np.uint32), m, SMALL)
        assert int(full[-1]) & ((1 << ((-m) % 32)) - 1) == 0 and (q.unpack_bits(full, m) == n % 2).all()


@pytest.mark.parametrize("n,m", [(65536, 65536), (65535, 3000), (40000, 25537), (4097, 700)])
def test_the_largest_counts_an_all_ones_key(q, n, m):
    """c_i = S[i + n] - S[i] with S the prefix sums of the seed: every product term is live, the counts are as large as n allows, and a
    residue left in [p, 2p) at the end would flip bits"""
    rng = np.random.default_rng(n + m)
    t = rng.integers(0, 2, n + m - 1)
    S = np.concatenate([[0], np.cumsum(t)])
    ref = q.pack_bits(((S[n:n + m] - S[:m]) & 1).astype(np.uint8))
    key = np.full((n + 31) // 32, 0xFFFFFFFF, np.uint32)
    for b in (0, SMALL):
        assert (q.toeplitz_ntt_host(key, n, q.pack_bits(t), m, b) == ref).all(), b
    full = q.toeplitz_ntt_host(key, n, np.full((n + m - 1 + 31) // 32, 0xFFFFFFFF, np.uint32), m)
    assert (q.unpack_bits(full, m) == n % 2).all()


@pytest.mark.parametrize("n,m", [(1000, 257), (33, 4097), (1, 65), (64, 65)])
def test_linear_in_the_key_and_in_the_seed(q, n, m):
    rng = np.random.default_rng(n * m)
    x1, t1, k1, s1 = draw(q, rng, n, m)
    x2, t2, k2, s2 = draw(q, rng, n, m)
    for b in (0, SMALL):
        def f(k, s):
            return q.toeplitz_ntt_host(k, n, s, m, b)
        assert (f(k1 ^ k2, s1) == f(k1, s1) ^ f(k2, s1)).all()
        assert (f(k1, s1 ^ s2) == f(k1, s1) ^ f(k1, s2)).all()
        assert (f(k1, s1) == q.pack_bits(ref_bits(x1, t1))).all()
        assert not f(np.zeros_like(k1), s1).any() and not f(k1, np.zeros_like(s1)).any()


@pytest.mark.parametrize("n,m", [(37, 11), (100, 70), (65, 257)])
def test_a_key_of_one_bit_returns_a_window_of_the_seed(q, n, m):
    rng = np.random.default_rng(n)
    t = rng.integers(0, 2, n + m - 1)
    seed = q.pack_bits(t)
    for j in (0, 1, 31, 32, n - 1):
        x = np.zeros(n, np.uint8)
        x[j] = 1
        assert (q.unpack_bits(q.toeplitz_ntt_host(q.pack_bits(x), n, seed, m, SMALL), m) == t[j:j + m]).all(), j


def test_host_mirror_argument_checks(q):
    key, seed = np.zeros(2, np.uint32), np.zeros(3, np.uint32)
    with pytest.raises(q.QldpcError):
        q.toeplitz_ntt_host(key[:1], 64, seed, 10)              # too few key words
    with pytest.raises(q.QldpcError):
        q.toeplitz_ntt_host(key, 64, seed[:2], 10)              # too few seed words: 64 + 10 - 1 bits need 3
    with pytest.raises(q.QldpcError):
        q.toeplitz_ntt_host(key, 0, seed, 10)
    with pytest.raises(q.QldpcError):
        q.toeplitz_ntt_host(key, -5, seed, 10)
    with pytest.raises(q.QldpcError):
        q.toeplitz_ntt_host(key, 64, seed, -1)
    for bad in (-1, 26):
        with pytest.raises(q.QldpcError) as e:
            q.toeplitz_ntt_host(key, 64, seed, 10, pass_log2=bad)
        assert e.value.status == -1
    assert (q.toeplitz_ntt_host(key, 64, seed, 10, pass_log2=25) == 0).all()       # the largest pass there is; a zero key
    out = q.toeplitz_ntt_host(key, 64, seed, 0)
    assert out.size == 0 and out.dtype == np.uint32


def test_core_header_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "toeplitz_ntt_sanitize")
    subprocess.check_call(["gcc", "-std=gnu11", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "c", "toeplitz_ntt_sanitize.c"), "-lm"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "sanitizer pass ok" in r.stdout, r.stdout + r.stderr
