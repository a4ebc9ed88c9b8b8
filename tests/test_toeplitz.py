"""Toeplitz-hash privacy amplification (qldpc_toeplitz_*), host suite: qldpc_toeplitz_host runs the kernel's own window / fold functions
(csrc/qldpc_toeplitz_core.h), so the arithmetic of the lanes is checked here without a device.  The reference restates the definition
y_i = XOR_{j < n} x_j t_(i+j) in numpy; every comparison is exact equality of words."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE_N = (1, 31, 32, 33, 63, 64, 65, 1000, 4097)
EDGE_M = (1, 31, 32, 33, 63, 64, 65, 257)
TILES = (1, 2, 7, 64, 0)


def ref_bits(x, t):
    """y = np.correlate(t, x, "valid") & 1 over the bits x[0..n), t[0..n+m-1)"""
    return (np.correlate(t.astype(np.int64), x.astype(np.int64), "valid") & 1).astype(np.uint8)


def draw(q, rng, n, m, garbage=True):
    """key bits, seed bits and their packed words, the unused tail bits of both last words set"""
    x, t = rng.integers(0, 2, n), rng.integers(0, 2, n + m - 1)
    key, seed = q.pack_bits(x), q.pack_bits(t)
    if garbage:
        key[-1] |= np.uint32((1 << ((-n) % 32)) - 1)
        seed[-1] |= np.uint32((1 << ((-(n + m - 1)) % 32)) - 1)
    return x, t, key, seed


@pytest.mark.parametrize("n", EDGE_N)
def test_host_mirror_equals_the_reference(q, n):
    rng = np.random.default_rng(n)
    for m in EDGE_M:
        x, t, key, seed = draw(q, rng, n, m)
        ref = q.pack_bits(ref_bits(x, t))
        assert ref.size == (m + 31) // 32
        for tile in TILES:
            got = q.toeplitz_host(key, n, seed, m, tile)
            assert got.dtype == np.uint32 and got.shape == ref.shape and (got == ref).all(), (n, m, tile)


@pytest.mark.parametrize("n,m", [(33, 65), (1000, 257), (4097, 31), (31, 33)])
def test_tail_bits_are_ignored_and_the_output_tail_is_zero(q, n, m):
    rng = np.random.default_rng(n + m)
    x, t, key, seed = draw(q, rng, n, m, garbage=False)
    clean = q.toeplitz_host(key, n, seed, m)
    assert (clean == q.pack_bits(ref_bits(x, t))).all()
    key_g, seed_g = key.copy(), seed.copy()
    key_g[-1] |= np.uint32((1 << ((-n) % 32)) - 1)
    seed_g[-1] |= np.uint32((1 << ((-(n + m - 1)) % 32)) - 1)
    assert (key_g != key).any() or n % 32 == 0
    assert (seed_g != seed).any() or (n + m - 1) % 32 == 0
    for tile in (0, 7):
        assert (q.toeplitz_host(key_g, n, seed_g, m, tile) == clean).all()
    # words past the rows are not part of the block either
    assert (q.toeplitz_host(np.concatenate([key_g, [np.uint32(0xFFFFFFFF)]]), n, np.concatenate([seed_g, [np.uint32(0xFFFFFFFF)]]), m) == clean).all()
    if m % 32:
        assert int(clean[-1]) & ((1 << ((-m) % 32)) - 1) == 0
        ones = q.toeplitz_host(np.full(key.size, 0xFFFFFFFF, np.uint32), n, np.full(seed.size, 0xFFFFFFFF, np.uint32), m)
        assert int(ones[-1]) & ((1 << ((-m) % 32)) - 1) == 0 and (q.unpack_bits(ones, m) == n % 2).all()


@pytest.mark.parametrize("n,m", [(37, 11), (100, 70), (65, 257)])
def test_a_key_of_one_bit_returns_a_window_of_the_seed(q, n, m):
    rng = np.random.default_rng(n)
    t = rng.integers(0, 2, n + m - 1)
    seed = q.pack_bits(t)
    for j in (0, 1, 31, 32, n - 1):
        x = np.zeros(n, np.uint8)
        x[j] = 1
        assert (q.unpack_bits(q.toeplitz_host(q.pack_bits(x), n, seed, m), m) == t[j:j + m]).all(), j


def test_equals_the_explicit_toeplitz_matrix(q):
    n, m = 37, 11
    rng = np.random.default_rng(3711)
    x, t, key, seed = draw(q, rng, n, m)
    i, j = np.meshgrid(np.arange(m), np.arange(n), indexing="ij")
    T = t[i - j + n - 1]
    y = T @ x[::-1] % 2
    for tile in TILES:
        assert (q.unpack_bits(q.toeplitz_host(key, n, seed, m, tile), m) == y).all()
    assert (ref_bits(x, t) == y).all()


@pytest.mark.parametrize("n,m", [(1000, 257), (33, 4097), (1, 65), (64, 65)])
def test_linear_in_the_key_and_in_the_seed_also_for_more_output_than_key(q, n, m):
    rng = np.random.default_rng(n * m)
    x1, t1, k1, s1 = draw(q, rng, n, m)
    x2, t2, k2, s2 = draw(q, rng, n, m)
    f = q.toeplitz_host
    assert (f(k1 ^ k2, n, s1, m) == f(k1, n, s1, m) ^ f(k2, n, s1, m)).all()
    assert (f(k1, n, s1 ^ s2, m) == f(k1, n, s1, m) ^ f(k1, n, s2, m)).all()
    assert (f(k1, n, s1, m) == q.pack_bits(ref_bits(x1, t1))).all()
    assert not f(np.zeros_like(k1), n, s1, m).any() and not f(k1, n, np.zeros_like(s1), m).any()


def test_seed_words(q):
    assert q.toeplitz_seed_words(1, 1) == 1
    assert q.toeplitz_seed_words(32, 1) == 1
    assert q.toeplitz_seed_words(32, 2) == 2
    assert q.toeplitz_seed_words(56880, 41935) == (56880 + 41935 - 1 + 31) // 32
    assert q.toeplitz_seed_words(0, 10) == 0 and q.toeplitz_seed_words(10, 0) == 0 and q.toeplitz_seed_words(-3, 10) == 0 and q.toeplitz_seed_words(10, -1) == 0


def test_host_mirror_argument_checks(q):
    key, seed = np.zeros(2, np.uint32), np.zeros(3, np.uint32)
    with pytest.raises(q.QldpcError):
        q.toeplitz_host(key[:1], 64, seed, 10)                  # too few key words
    with pytest.raises(q.QldpcError):
        q.toeplitz_host(key, 64, seed[:2], 10)                  # too few seed words: 64 + 10 - 1 bits need 3
    with pytest.raises(q.QldpcError):
        q.toeplitz_host(key, 0, seed, 10)
    with pytest.raises(q.QldpcError):
        q.toeplitz_host(key, -5, seed, 10)
    with pytest.raises(q.QldpcError):
        q.toeplitz_host(key, 64, seed, -1)
    with pytest.raises(q.QldpcError) as e:
        q.toeplitz_host(key, 64, seed, 10, tile_words=-1)
    assert e.value.status == -6
    out = q.toeplitz_host(key, 64, seed, 0)
    assert out.size == 0 and out.dtype == np.uint32


def test_core_header_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "toeplitz_sanitize")
    subprocess.check_call(["gcc", "-std=gnu11", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "c", "toeplitz_sanitize.c"), "-lm"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "sanitizer pass ok" in r.stdout, r.stdout + r.stderr
