"""Puncture patterns of the Monte-Carlo loop (qldpc_mc_pattern_host), host suite: the host mirror runs the radix select of
csrc/qldpc_mc_core.h that the pattern kernel runs, checked here without a device against the numpy lexsort of tests/mc_search_ref.py.
Every comparison is exact equality."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mc_search_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x0123456789ABCDEF
N_CAND = (1, 3, 4, 5, 63, 64, 65, 255, 257, 410, 1000)
PATTERNS = (0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 63 + 5)


def _cut_is_inside_a_run(u, got, n_cand):
    """is some candidate with the threshold key taken and some other not -- and then the taken ones are the lower indices?"""
    T = u[got].max()
    left = np.setdiff1d(np.arange(n_cand), got)
    tied = left[u[left] == T]
    assert tied.size == 0 or tied.min() > got[u[got] == T].max()
    return tied.size > 0


@pytest.mark.parametrize("key_bits", [32, 8, 3, 1])
@pytest.mark.parametrize("n_cand", N_CAND)
def test_pattern_host_equals_the_lexsort(q, n_cand, key_bits):
    """The grid of the issue, exact equality.  For key_bits <= 3 and n_cand >= 63 (at most 8 distinct keys among 63 or more candidates) every
    interior n_punct must cut inside a run of equal keys, so that the tie rule decides; where a grid value happens to fall exactly between
    two keys (the reference's own keys say so), the neighbouring n_punct is compared too and must cut inside one."""
    def check(p, n_punct):
        got = q.mc_pattern_host(SEED, p, n_cand, n_punct, key_bits)
        ref = mc_search_ref.pattern(SEED, p, n_cand, n_punct, key_bits)
        assert got.dtype == np.int32 and got.shape == ref.shape == (n_punct,) and (got == ref).all(), (p, n_punct)
        return got

    for p in PATTERNS:
        u = mc_search_ref.keys(SEED, p, n_cand, key_bits)
        assert int(u.max()) < 2 ** key_bits
        for n_punct in sorted({0, 1, n_cand // 3, n_cand - 1, n_cand}):
            got = check(p, n_punct)
            if key_bits <= 3 and n_cand >= 63 and 0 < n_punct < n_cand and not _cut_is_inside_a_run(u, got, n_cand):
                near = n_punct + 1 if n_punct < n_cand - 1 else n_punct - 1
                assert _cut_is_inside_a_run(u, check(p, near), n_cand), (p, n_punct, near)
    assert (q.mc_pattern_host(SEED, 0, n_cand, n_cand, 0) == q.mc_pattern_host(SEED, 0, n_cand, n_cand, 32)).all()      # key_bits 0 = 32


def test_patterns_differ_by_seed_and_index(q):
    a = q.mc_pattern_host(SEED, 0, 410, 100)
    assert (np.diff(a) > 0).all() and a.min() >= 0 and a.max() < 410
    for other in (q.mc_pattern_host(SEED, 1, 410, 100), q.mc_pattern_host(SEED + 1, 0, 410, 100), q.mc_pattern_host(SEED, 2 ** 32, 410, 100)):
        assert other.shape == a.shape and (other != a).any()
    # growing n_punct only adds candidates: the order (u', c) does not depend on n_punct
    assert np.isin(a, q.mc_pattern_host(SEED, 0, 410, 101)).all()


def test_pattern_host_argument_checks(q):
    for n_cand, n_punct, key_bits in ((10, 11, 32), (10, -1, 32), (-1, 0, 32), (10, 3, 33), (10, 3, -1), (0, 1, 32)):
        with pytest.raises(q.QldpcError) as e:
            q.mc_pattern_host(SEED, 0, n_cand, n_punct, key_bits)
        assert e.value.status == -6, (n_cand, n_punct, key_bits)
    # a refused call writes nothing
    idx = np.full(8, -7, np.int32)
    ip = idx.ctypes.data_as(C.POINTER(C.c_int))
    assert q._L.qldpc_mc_pattern_host(SEED, 0, 4, 5, 32, ip) == -6 and q._L.qldpc_mc_pattern_host(SEED, 0, 8, 3, 40, ip) == -6
    assert (idx == -7).all()
    assert q._L.qldpc_mc_pattern_host(SEED, 0, 8, 3, 32, None) == -1
    assert q._L.qldpc_mc_pattern_host(SEED, 0, 8, 3, 32, ip) == 0 and (idx[:3] >= 0).all() and (idx[3:] == -7).all()      # exactly n_punct entries
    assert q.mc_pattern_host(SEED, 0, 0, 0).size == 0 and q.mc_pattern_host(SEED, 5, 9, 0).size == 0


def test_inclusion_frequency_is_uniform(q):
    """Each of 64 candidates is in a pattern of 16 with probability p = 1/4, so its count over 2 000 independent patterns is
    Binomial(2000, 1/4): mean 500, sigma = sqrt(2000 * 1/4 * 3/4) = 19.36.  Bound: +- 6 sigma = +- 116.2 per candidate (two-sided tail
    2e-9 each, 1.3e-7 over the 64).  An ordering bug that favours low indices moves the ends of the list by far more."""
    n, n_cand, n_punct = 2000, 64, 16
    count = np.zeros(n_cand, np.int64)
    for p in range(n):
        idx = q.mc_pattern_host(SEED, p, n_cand, n_punct)
        assert idx.size == n_punct
        count[idx] += 1
    sigma = np.sqrt(n * 0.25 * 0.75)
    print(count.min(), count.max(), 6 * sigma)
    assert count.sum() == n * n_punct and (np.abs(count - n * 0.25) <= 6 * sigma).all(), count
    # and the halves of the index range are balanced: 32 candidates x 2000 patterns, each half's total within 6 sigma of a hypergeometric draw
    # (variance per pattern 16 * 1/2 * 1/2 * 48/63 = 3.05)
    assert abs(int(count[:32].sum()) - n * 8) <= 6 * np.sqrt(n * 16 * 0.25 * 48 / 63)


def test_pattern_mirror_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "mc_search_sanitize")
    csrc = os.path.join(ROOT, "qcrypto-ldpc_amd", "csrc")
    subprocess.check_call(["gcc", "-std=gnu11", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                           "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-o", exe, os.path.join(ROOT, "tests", "c", "mc_search_sanitize.c"),
                           os.path.join(csrc, "qldpc_mc_host.c"), os.path.join(csrc, "qldpc_graph.c"), "-lm"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "sanitizer pass ok" in r.stdout, r.stdout + r.stderr
