"""CPU suite: the host side of the blind reconciliation rounds of the Monte-Carlo loop -- the schedule (qldpc_mc_blind_next_host, the function
qldpc_mc_blind calls per launch) against the restatement of tests/mc_blind_ref.py over random count vectors and whole simulated runs, and the
efficiency figure (qldpc_mc_blind_efficiency_host) against exact arithmetic.  No GPU compute."""
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import mc_blind_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_next_equals_the_rule_on_random_counts(q):
    rng = np.random.default_rng(1)
    for _ in range(2000):
        R, batch = int(rng.integers(0, 9)), int(rng.integers(1, 70))
        pool = rng.integers(0, 2 * batch, R + 1).astype(np.uint64)
        pool[rng.random(R + 1) < 0.4] = 0
        left = int(rng.choice([0, 1, batch - 1, batch, batch + 1, 10 * batch, 2 ** 40]))
        assert q.mc_blind_next(pool, left, batch) == mc_blind_ref.next_launch([int(x) for x in pool], left, batch), (pool, left, batch)
    assert q.mc_blind_next([7], 0, 4) is None and q.mc_blind_next([7], 9, 4) == (0, 4)                  # max_rounds = 0: pool[0] is not read
    assert q.mc_blind_next([0, 3, 8, 9], 100, 8) == (3, 8) and q.mc_blind_next([0, 3, 7, 2], 5, 8) == (0, 5)
    assert q.mc_blind_next([0, 0, 7, 2], 0, 8) == (2, 7) and q.mc_blind_next(np.zeros(65, np.uint64), 0, 8) is None


@pytest.mark.parametrize("R,batch,n_in,p_open", [(0, 16, 100, 0.5), (1, 16, 333, 0.3), (3, 64, 1000, 0.45), (4, 7, 500, 0.9), (6, 40, 2000, 0.6),
                                                 (5, 1, 60, 0.7), (3, 64, 192, 0.62), (8, 33, 700, 1.0), (2, 50, 49, 0.5)])
def test_whole_runs_agree_launch_for_launch(q, R, batch, n_in, p_open):
    """a simulated run: every frame stays open after a round with probability p_open; the library's schedule and the restatement drive the
    same stacks and must pick the same level and size at every launch, flush included"""
    rng = np.random.default_rng(R * 1000 + batch)
    close = np.full(n_in, -1, np.int64)
    for r in range(R, -1, -1):
        close[rng.random(n_in) >= p_open] = r      # the earliest round that closes the frame is drawn last
    got, peak, drawn = mc_blind_ref.replay(close, R, batch, schedule=lambda pool, left, b: q.mc_blind_next(pool, left, b))
    want, peak_ref, _ = mc_blind_ref.replay(close, R, batch)
    assert [(x["level"], x["frames"]) for x in got] == [(x["level"], x["frames"]) for x in want]
    assert peak == peak_ref and peak < 2 * batch                                  # no pool ever reaches 2 batch
    assert drawn == n_in and sum(len(x["frames"]) for x in got if x["level"] == 0) == n_in
    assert sum(len(x["frames"]) for x in got) == n_in + sum(x["opened"] for x in got if x["level"] < R)      # every frame that went on was decoded again
    for r in range(R + 1):                                                        # every frame was decoded in exactly the rounds up to its closing one
        assert sorted(i for x in got if x["level"] == r for i in x["frames"]) == [i for i in range(n_in) if close[i] < 0 or close[i] >= r]
    ragged = [x for x in got if x["level"] > 0 and len(x["frames"]) < batch]
    assert all(got.index(x) > max(i for i, y in enumerate(got) if y["level"] == 0) for x in ragged)          # ragged launches belong to the flush


def test_a_stopped_input_is_flushed(q):
    close = np.full(300, -1, np.int64)
    close[::3] = 1
    got, _, drawn = mc_blind_ref.replay(close, 2, 32, schedule=lambda pool, left, b: q.mc_blind_next(pool, left, b),
                                        stop=lambda launch: launch["level"] == 2)      # the first launch that ends frames open ends the input
    assert drawn < 300 and drawn % 32 == 0
    assert sorted(i for x in got if x["level"] == 2 for i in x["frames"]) == [i for i in range(drawn) if close[i] != 1]


def test_efficiency_against_exact_arithmetic(q):
    for n_chan, n_par, frames, disclosed, qber in [(504, 504, 192, 2630, 0.26), (1590, 410, 192, 3302, 0.03), (52429, 13107, 4096, 0, 0.02),
                                                   (1, 0, 1, 1, 0.25), (65536, 0, 2 ** 33, 2 ** 40 + 1, 0.11)]:
        h2 = -qber * math.log2(qber) - (1.0 - qber) * math.log2(1.0 - qber)
        want = float(Fraction(n_par) + Fraction(disclosed, frames)) / (n_chan * h2)
        got = q.mc_blind_efficiency(n_chan, n_par, frames, disclosed, qber)
        assert abs(got - want) <= 4 * np.finfo(np.float64).eps * want, (got, want)
    assert q.mc_blind_efficiency(1000, 100, 10, 0, 0.05) == q.mc_blind_efficiency(1000, 0, 10, 1000, 0.05)
    assert abs(q.mc_blind_efficiency(8, 4, 1, 0, 0.11002786443835955) - 1.0) < 1e-12          # h2 = 1/2 there: 4 bits of 8 x 0.5


def test_argument_errors_that_need_no_device(q):
    import ctypes as C
    for pool, left, batch, status in [(np.zeros(66), 0, 4, -6), ([0, 1], 0, 0, -6), ([0, 1], 0, -3, -6), ([], 0, 4, -6)]:
        with pytest.raises(q.QldpcError) as e:
            q.mc_blind_next(pool, left, batch)
        assert e.value.status == status, (pool, batch)
    for args in [(0, 0, 1, 0, 0.1), (10, -1, 1, 0, 0.1), (10, 0, 0, 0, 0.1), (10, 0, 1, 0, 0.0), (10, 0, 1, 0, 0.5), (10, 0, 1, 0, float("nan"))]:
        with pytest.raises(q.QldpcError) as e:
            q.mc_blind_efficiency(*args)
        assert e.value.status == -6, args
    L = q._L
    level, n, f = C.c_int(-5), C.c_int(-5), C.c_double(-5.0)
    pool = np.zeros(3, np.uint64)
    assert L.qldpc_mc_blind_next_host(2, 4, None, 9, C.byref(level), C.byref(n)) == -1
    assert L.qldpc_mc_blind_next_host(2, 4, pool.ctypes.data_as(C.POINTER(C.c_uint64)), 9, None, C.byref(n)) == -1
    assert L.qldpc_mc_blind_efficiency_host(10, 0, 1, 0, 0.1, None) == -1
    assert (level.value, n.value, f.value) == (-5, -5, -5.0)                       # a refused call writes nothing
    cfg, res = q.McBlindCfg(), q.McBlindResult()
    assert L.qldpc_mc_blind(None, C.byref(cfg), C.byref(res)) == -1
    assert L.qldpc_mc_blind_stats(None, None, 0) == -1 and L.qldpc_mc_blind_open(None, None, None, 0) == -1
    assert q.MC_BLIND_MAX_ROUNDS == 64 and q.MC_BLIND_ROUND_STAT.names[-1] == "disclosed" and q.MC_BLIND_ROUND_STAT.itemsize == 80


def test_host_code_under_asan_ubsan(tmp_path):
    """the schedule driven to the end of simulated runs and the efficiency figure as a stand-alone program (nothing loaded into Python is sanitised)"""
    exe = str(tmp_path / "mc_blind_sanitize")
    csrc = os.path.join(ROOT, "qcrypto-ldpc_amd", "csrc")
    subprocess.check_call(["gcc", "-std=gnu11", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                           "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-o", exe, os.path.join(ROOT, "tests", "c", "mc_blind_sanitize.c"),
                           os.path.join(csrc, "qldpc_mc_host.c"), os.path.join(csrc, "qldpc_graph.c"), "-lm"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "sanitizer pass ok" in r.stdout, r.stdout + r.stderr
