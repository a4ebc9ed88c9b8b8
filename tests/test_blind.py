"""CPU suite: the host side of blind reconciliation -- the weakest-VN select (qldpc_weakest_host, the functions the kernel's lanes run, against
the lexsort of tests/blind_ref.py) and Alice's answer (qldpc_recon_disclose_host).  No GPU compute."""
import numpy as np
import pytest

import blind_ref

SIZES = [1, 31, 32, 33, 1008]


def ds(N):
    return [0, 1, N, N + 5]


def posts(N, rng):
    """what a posterior row can look like: distinct floats, three magnitudes (ties decide), signed zeros among small values"""
    rnd = (rng.standard_normal(N) * 7).astype(np.float32)
    ties = rng.choice(np.array([0.75, 1.5, 23.03], np.float32), N) * rng.choice(np.array([-1, 1], np.float32), N)
    zeros = np.where(rng.random(N) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    zeros[rng.random(N) < 0.3] = np.float32(1e-40)      # a denormal: above both zeros
    zeros[rng.random(N) < 0.2] = np.float32(-2.5)
    return {"random": rnd, "ties": ties.astype(np.float32), "zeros": zeros}


def masks(N, rng):
    W = (N + 31) // 32
    tail = np.zeros(N, np.uint8)
    tail[32 * (W - 1):] = 1                               # only the VNs of the last word
    return {"all": None, "random": (rng.random(N) < 0.4).astype(np.uint8), "empty": np.zeros(N, np.uint8), "last_word": tail,
            "one": np.eye(1, N, N - 1, dtype=np.uint8)[0]}


@pytest.mark.parametrize("N", SIZES)
def test_weakest_host_is_the_lexsort(q, N):
    rng = np.random.default_rng(N)
    for pname, post in posts(N, rng).items():
        for mname, cand in masks(N, rng).items():
            for d in ds(N):
                want = blind_ref.weakest(post, d, cand)
                got, n = q.weakest_host(post, d, None if cand is None else blind_ref.pack_row(cand))
                assert (got == want).all(), (pname, mname, d)
                assert n == min(d, N if cand is None else int(cand.sum())), (pname, mname, d)


def test_weakest_host_ignores_candidate_bits_past_n(q):
    N = 33
    rng = np.random.default_rng(5)
    post = rng.standard_normal(N).astype(np.float32)
    cand = np.full(2, 0xffffffff, np.uint32)              # the 31 tail bits of the last word set
    got, n = q.weakest_host(post, N + 5, cand)
    assert n == N and (got == blind_ref.weakest(post, N, None)).all() and got[1] == 0x80000000


def test_weakest_host_orders_zeros_and_ties_by_index(q):
    post = np.array([1.0, -0.0, 0.0, -1.0, 1.0, 0.0], np.float32)
    for d, want in [(1, [1]), (2, [1, 2]), (3, [1, 2, 5]), (4, [0, 1, 2, 5]), (5, [0, 1, 2, 3, 5])]:
        got, n = q.weakest_host(post, d)
        assert n == d and list(np.flatnonzero(blind_ref.unpack_row(got, 6))) == want


def test_weakest_host_argument_errors(q):
    post = np.zeros(8, np.float32)
    with pytest.raises(q.QldpcError) as e:
        q.weakest_host(post, -1)
    assert e.value.status == -1
    with pytest.raises(q.QldpcError):
        q.weakest_host(np.zeros(0, np.float32), 1)
    with pytest.raises(q.QldpcError):
        q.weakest_host(np.zeros(40, np.float32), 1, np.zeros(1, np.uint32))      # a mask of the wrong length


@pytest.mark.parametrize("key_bits", [1, 31, 32, 33, 1000])
def test_disclose_is_unpack_bits(q, key_bits):
    rng = np.random.default_rng(key_bits)
    words = rng.integers(0, 1 << 32, (key_bits + 31) // 32, dtype=np.uint64).astype(np.uint32)
    bits = q.unpack_bits(words, key_bits)
    pos = rng.permutation(key_bits)[:max(1, key_bits // 3)]
    assert (q.recon_disclose(words, key_bits, pos) == bits[pos]).all()
    assert q.recon_disclose(words, key_bits, []).size == 0
    for bad in ([key_bits], [-1], [0, key_bits + 3]):
        with pytest.raises(q.QldpcError) as e:
            q.recon_disclose(words, key_bits, bad)
        assert e.value.status == -1


def test_host_code_under_asan_ubsan(tmp_path):
    """the select and Alice's answer as a stand-alone program with exactly sized buffers"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "blind_sanitize")
    subprocess.check_call(["gcc", "-std=gnu11", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                           "-I" + os.path.join(root, "include"), "-o", exe, os.path.join(root, "tests", "c", "blind_sanitize.c"), "-lm"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "sanitizer pass ok" in r.stdout, r.stdout + r.stderr
