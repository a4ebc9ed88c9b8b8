"""CPU suite: the host side of the syndrome-weight QBER estimate -- the mirrors of the counting and argmax kernels (qldpc_qber_counts_host,
qldpc_qber_argmax_host: the functions the lanes run) and the tables, against the restatement of the rule in tests/qber_ref.py.  No GPU compute."""
import os
import subprocess

import numpy as np
import pytest

import qber_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
@pytest.mark.parametrize("name", qber_ref.CODES)
@pytest.mark.parametrize("combo", qber_ref.COMBOS)
def test_counts_host_is_the_rule(q, name, combo):
    code = qber_ref.make_code(q, name)
    var, chk = code.edges()
    D = code.max_cn_degree
    rng = np.random.default_rng(len(name) * 131 + len(combo))
    F = 3
    f = qber_ref.frames(rng, code.N, code.M, F, combo)
    seen = 0
    for i in range(F):
        want = np.array(qber_ref.frame_counts(var, chk, code.N, code.M, D, f, i), np.uint32)
        got = qber_ref.host_counts(q, code, f, i)
        assert got.shape == (D + 1, 2) and (got == want).all(), (name, combo, i)
        seen += int(want[:, 0].sum())
    assert seen > 0
    if combo == "null":      # every VN noisy: every check informative at its own degree
        assert int(got[:, 0].sum()) == code.M and got[0, 0] == 0


def test_known_wins_over_erased_and_over_the_class(q):
    """one check of three VNs: erased + known counts as exact with the value row's bit, whatever the class says"""
    code = q.Code.from_edges(3, 1, [0, 1, 2], [0, 0, 0])
    one = lambda *b: q.pack_bits(np.array(b, np.uint8))
    assert q.qber_counts_host(code, one(1, 0, 0)).tolist() == [[0, 0], [0, 0], [0, 0], [1, 1]]
    assert q.qber_counts_host(code, one(1, 0, 0), erase=one(0, 1, 0)).tolist() == [[0, 0]] * 4      # not informative
    got = q.qber_counts_host(code, one(1, 0, 0), erase=one(0, 1, 0), known=one(0, 1, 0), value=one(0, 1, 0))
    assert got.tolist() == [[0, 0], [0, 0], [1, 0], [0, 0]]                                              # d = 2, u = 1 ^ 1 ^ 0
    got = q.qber_counts_host(code, one(1, 0, 0), vn_class=[0, 2, 1], known=one(0, 1, 0), value=one(0, 0, 0))
    assert got.tolist() == [[0, 0], [1, 1], [0, 0], [0, 0]]                                              # VN 2 pinned, VN 1 known 0
    got = q.qber_counts_host(code, one(1, 0, 0), n_channel=0, syndrome=one(1))
    assert got.tolist() == [[1, 0], [0, 0], [0, 0], [0, 0]]                                              # all shortened: d = 0, u = 1 ^ 1
    with pytest.raises(q.QldpcError):
        q.qber_counts_host(code, one(1, 0, 0), known=one(0, 1, 0))                                       # known without value


@pytest.mark.parametrize("D,n_grid,q_lo,q_hi", [(8, 256, 0.001, 0.25), (12, 2, 0.001, 0.25), (27, 1000, 0.0005, 0.11), (63, 1024, 0.001, 0.25)])
def test_tables_are_the_rounded_logs(q, D, n_grid, q_lo, q_hi):
    L1, L0, qs, llr = q.qber_table_host(D, n_grid, q_lo, q_hi)
    r1, r0, rq = qber_ref.tables(D, n_grid, q_lo, q_hi)
    assert L1.shape == L0.shape == (D + 1, n_grid) and not L1[0].any() and not L0[0].any()
    # +-1: the llround boundary; the double error is far below one unit at scale 2^24
    assert np.abs(L1.astype(np.int64) - np.array(r1, np.int64)).max() <= 1 and np.abs(L0.astype(np.int64) - np.array(r0, np.int64)).max() <= 1
    assert (np.abs(qs.astype(np.float64) - np.array(rq)) <= 1.2e-7 * np.array(rq)).all()      # the double grid rounded to float
    assert abs(float(qs[0]) - q_lo) < 1e-9 and abs(float(qs[-1]) - q_hi) < 1e-7
    assert all(llr[k] == np.float32(q.bsc_llr(float(qs[k]))) for k in range(n_grid))


def test_table_argument_errors(q):
    for bad in [(8, 1, 0.001, 0.25), (8, 1025, 0.001, 0.25), (8, 256, 0.0, 0.25), (8, 256, 0.1, 0.1), (8, 256, 0.001, 0.5), (0, 256, 0.001, 0.25)]:
        with pytest.raises(q.QldpcError) as e:
            q.qber_table_host(*bad)
        assert e.value.status == -1, bad
    with pytest.raises(q.QldpcError) as e:
        q.qber_table_host(64, 256, 0.001, 0.25)
    assert e.value.status == -7


def test_argmax_host_is_the_integer_argmax(q):
    rng = np.random.default_rng(11)
    for D, n_grid in [(8, 256), (12, 2), (27, 1000)]:
        L1, L0, qs, _ = q.qber_table_host(D, n_grid)
        for trial in range(12):
            n = rng.integers(0, [3, 600, 2 ** 20, 2 ** 30][trial % 4], D + 1).astype(np.uint64)
            n[rng.random(D + 1) < 0.4] = 0
            u = (n * rng.uniform(0, 0.5, D + 1)).astype(np.uint64)
            cnt = np.stack([n, u], axis=1)
            assert q.qber_argmax_host(cnt, L1, L0) == qber_ref.argmax(cnt.tolist(), L1.tolist(), L0.tolist()), (D, n_grid, trial)


def test_argmax_host_edge_cases(q):
    D = 8
    L1, L0, qs, _ = q.qber_table_host(D, 256)
    zero = np.zeros((D + 1, 2), np.uint64)
    assert q.qber_argmax_host(zero, L1, L0) == -1
    only0 = zero.copy(); only0[0] = (50, 3)                      # row 0 is diagnostics: the score ignores it
    assert q.qber_argmax_host(only0, L1, L0) == -1
    sat = zero.copy(); sat[6] = (400, 0); sat[7] = (100, 0)      # every check satisfied: the clamp
    assert q.qber_argmax_host(sat, L1, L0) == 0
    half = zero.copy(); half[6] = (400, 200)                     # as bad as it gets: the top of the grid
    assert q.qber_argmax_host(half, L1, L0) == 255
    # ties go to the lowest k: tables with equal columns
    T1, T0 = L1.copy(), L0.copy()
    T1[:, 40:44] = T1[:, 40:41]; T0[:, 40:44] = T0[:, 40:41]
    mid = zero.copy(); mid[6] = (400, int(round(400 * qber_ref.p_d(float(qs[41]), 6))))
    k = q.qber_argmax_host(mid, T1, T0)
    assert k == qber_ref.argmax(mid.tolist(), T1.tolist(), T0.tolist()) and (k == 40 or not 40 < k < 44)
    flat = np.zeros_like(L1)
    assert q.qber_argmax_host(mid, flat, flat) == 0
    with pytest.raises(q.QldpcError):
        bad = zero.copy(); bad[3] = (2, 5)                       # more unsatisfied than counted
        q.qber_argmax_host(bad, L1, L0)


@pytest.mark.parametrize("punctured", [False, True])
def test_pooled_estimate_is_near_the_flip_rate(q, punctured):
    """64 frames of the IRA toy through a BSC at q = 0.02 against Alice's codeword parity (syndrome form of the disclosed parity: parity VNs pinned to
    Alice's bits), plain and with a quarter of the parity punctured and a third of the key shortened.  The pooled estimate lies within 5 sigma plus one
    grid step of the frames' empirical flip rate; sigma from the counts (qber_ref.sigma), 5 covers the mild dependence between checks it ignores."""
    N, K, F, qtrue = 1280, 1024, 64, 0.02
    M = N - K
    code = q.Code.ira(N, K)
    var, chk = code.edges()
    rng = np.random.default_rng(2024 + punctured)
    cls = np.zeros(N, np.uint8); cls[K:] = 1
    nch = np.full(F, K, np.int32)
    if punctured:
        cls[K + np.arange(0, M, 4)] = 2
        nch[:] = K - K // 3
    alice = rng.integers(0, 2, (F, N)).astype(np.uint8)
    alice[:, :K][np.arange(K)[None, :] >= nch[:, None]] = 0            # shortened key bits are known zeros
    # Alice's word need not be a codeword: her syndrome travels instead (syndrome form), so the parity VNs carry her bits exactly
    synd = np.zeros((F, M), np.uint8)
    for v, c in zip(var, chk):
        synd[:, c] ^= alice[:, v]
    flips = (rng.random((F, N)) < qtrue).astype(np.uint8)
    flips[np.arange(N)[None, :] >= nch[:, None]] = 0              # only the noisy VNs: key bits below the frame's length
    bob = alice ^ flips
    pool = np.zeros((code.max_cn_degree + 1, 2), np.uint64)
    for i in range(F):
        pool += q.qber_counts_host(code, q.pack_bits(bob[i]), cls, int(nch[i]), q.pack_bits(synd[i]))
    L1, L0, qs, _ = q.qber_table_host(code.max_cn_degree, 256)
    k = q.qber_argmax_host(pool, L1, L0)
    n_noisy = int(nch.sum())
    emp = flips.sum() / n_noisy
    sig = qber_ref.sigma(pool.tolist(), emp)
    step = float(qs[min(k + 1, 255)] - qs[min(k + 1, 255) - 1])
    print("pooled q = %.5f, empirical %.5f, sigma %.5f, informative checks %d of %d" % (qs[k], emp, sig, int(pool[1:, 0].sum()), F * M))
    assert k >= 0 and int(pool[1:, 0].sum()) > (0.4 if punctured else 0.99) * F * M
    assert abs(float(qs[k]) - emp) <= 5 * sig + step


def test_host_code_under_asan_ubsan(tmp_path):
    """the mirrors as a stand-alone program with exactly sized buffers"""
    csrc = os.path.join(ROOT, "qcrypto-ldpc_amd", "csrc")
    exe = str(tmp_path / "qber_sanitize")
    subprocess.check_call(["gcc", "-std=gnu11", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "c", "qber_sanitize.c"),
                           os.path.join(csrc, "qldpc_qber_host.c"), os.path.join(csrc, "qldpc_graph.c"), "-lm"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "sanitizer pass ok" in r.stdout, r.stdout + r.stderr
