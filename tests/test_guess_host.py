"""CPU suite: the host side of the guessing rounds -- the mirrors of the trial rows and of the verdict over the trials (qldpc_guess_trial_host,
qldpc_guess_pick_host, the functions the lanes of qk_guess_expand and qk_guess_pick run) and the schedule of qldpc_mc_guess
(qldpc_mc_guess_next_host, the function it calls per launch) against the restatement of tests/mc_guess_ref.py.  No GPU compute."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import blind_ref
import mc_guess_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def guess_row(rng, N, vns):
    bits = np.zeros(N, np.uint8)
    bits[list(vns)] = 1
    return blind_ref.pack_row(bits), blind_ref.pack_row(rng.integers(0, 2, N))


def cases(rng, N, g):
    """guess sets of N VNs for g bits: random ones of g and of fewer VNs, the empty one, sets in the last (partial) word, sets astride words 63 / 64"""
    W = (N + 31) // 32
    out = [rng.choice(N, g, replace=False) for _ in range(3)]
    out += [rng.choice(N, k, replace=False) for k in sorted({0, g // 2, max(g - 1, 0)})]
    last = np.arange(32 * (W - 1), N)
    out.append(last[-min(g, last.size):] if g else last[:0])
    if W > 64 and g >= 2:
        astride = np.concatenate([np.arange(64 * 32 - (g + 1) // 2, 64 * 32), np.arange(64 * 32, 64 * 32 + g // 2)])
        out += [astride, np.array([63 * 32 + 31, 64 * 32])[:g]]
    return out


@pytest.mark.parametrize("g", [0, 1, 3, 10])
@pytest.mark.parametrize("N", [20, 1008, 8300])
def test_trial_rows_equal_the_restated_rule(q, N, g):
    rng = np.random.default_rng(100 * g + N)
    for vns in cases(rng, N, g):
        weak, hard = guess_row(rng, N, vns)
        known, value = mc_guess_ref.trial_rows(N, g, weak, hard)
        trials = range(1 << g) if g < 10 else [0, 1, 2, 511, 512, 682, 1023] + [int(t) for t in rng.integers(0, 1024, 20)]
        for t in trials:
            k, v = q.guess_trial_host(N, g, t, weak, hard)
            assert (k == known[t]).all() and (v == value[t]).all(), (N, g, t, sorted(vns))
            assert (k == weak).all() and not (v & ~weak).any()
        k0, v0 = q.guess_trial_host(N, g, 0, weak, hard)
        assert (v0 == (hard & weak)).all()                                         # trial 0 pins the frame's own decisions
        if len(vns) < g:                                                           # ranks that do not exist: the bits of t above them are ignored
            low = (1 << len(vns)) - 1
            for t in [int(x) for x in rng.integers(0, 1 << g, 8)]:
                assert (q.guess_trial_host(N, g, t, weak, hard)[1] == q.guess_trial_host(N, g, t & low, weak, hard)[1]).all()


def test_trials_of_a_full_set_are_all_different(q):
    rng = np.random.default_rng(3)
    weak, hard = guess_row(rng, 8300, [5, 2047, 2048, 4000, 8299])
    rows = {tuple(q.guess_trial_host(8300, 5, t, weak, hard)[1]) for t in range(32)}
    assert len(rows) == 32
    bits = blind_ref.unpack_row(q.guess_trial_host(8300, 5, 0b10110, weak, hard)[1] ^ (hard & weak), 8300)
    assert sorted(np.flatnonzero(bits)) == [2047, 2048, 8299]                      # rank j = ascending VN order, bit j of t


@pytest.mark.parametrize("g", [0, 1, 3, 10])
@pytest.mark.parametrize("N", [20, 1008, 8300])
def test_pick_equals_the_restated_rule(q, N, g):
    rng = np.random.default_rng(7 * g + N)
    T, W = 1 << g, (N + 31) // 32
    pad = np.uint32((1 << ((-N) % 32)) - 1)
    for case in range(12):
        base = blind_ref.pack_row(rng.integers(0, 2, N))
        rows = np.tile(base, (T, 1))
        ok = (rng.random(T) < [0.0, 1.0, 0.3, 0.05][case % 4]).astype(np.int32)
        if case == 4:
            ok[:] = 0
            ok[T - 1] = 1
        if case >= 6:                                                              # some trials decode to something else
            for t in rng.choice(T, max(1, T // 3), replace=False):
                rows[t, rng.integers(0, W)] ^= np.uint32(1) << np.uint32(rng.integers(0, 32))
        if case >= 9:                                                              # differences in the padding of the last word alone
            rows = np.tile(base, (T, 1))
            rows[:, W - 1] ^= rng.integers(0, 2 ** 32, T, dtype=np.uint64).astype(np.uint32) & pad
        want = mc_guess_ref.pick(N, ok, rows)
        assert q.guess_pick_host(N, g, ok, rows) == want, (N, g, case)
        if case >= 9:
            assert want[2] == 0
    if g:
        rows = np.tile(blind_ref.pack_row(rng.integers(0, 2, N)), (T, 1))
        ok = np.zeros(T, np.int32)
        ok[[0, T - 1]] = 1
        rows[T - 1, W - 1] ^= np.uint32(1) << np.uint32((-N) % 32)                  # the last valid position
        assert q.guess_pick_host(N, g, ok, rows) == (0, 2, 1)
        rows[0, W - 1] ^= np.uint32(1) << np.uint32((-N) % 32)
        assert q.guess_pick_host(N, g, ok, rows) == (0, 2, 0)


def test_next_equals_the_rule_on_random_counts(q):
    rng = np.random.default_rng(1)
    for _ in range(3000):
        g = int(rng.integers(0, 11))
        batch = int(rng.integers(1 << g, (1 << g) * 9 + 2))
        S = batch >> g
        pool = int(rng.choice([0, 1, S - 1, S, S + 1, S + batch - 1]))
        left = int(rng.choice([0, 1, batch - 1, batch, batch + 1, 10 * batch, 2 ** 40]))
        assert q.mc_guess_next(g, batch, max(pool, 0), left) == mc_guess_ref.next_launch(g, batch, max(pool, 0), left), (g, batch, pool, left)
    assert q.mc_guess_next(3, 40, 5, 10) == (q.MC_GUESS_TRIALS, 5) and q.mc_guess_next(3, 40, 4, 10) == (q.MC_GUESS_FRESH, 10)
    assert q.mc_guess_next(3, 40, 4, 0) == (q.MC_GUESS_TRIALS, 4) and q.mc_guess_next(3, 40, 0, 0) is None
    assert q.mc_guess_next(0, 7, 0, 100) == (q.MC_GUESS_FRESH, 7) and q.mc_guess_next(10, 1024, 1, 5) == (q.MC_GUESS_TRIALS, 1)


@pytest.mark.parametrize("g,batch,n_in,p_fail", [(0, 16, 100, 0.5), (1, 16, 333, 0.3), (3, 64, 1000, 0.45), (3, 40, 500, 0.9), (3, 192, 192, 0.6), (6, 64, 300, 0.2),
                                                 (10, 1024, 3000, 0.01), (2, 4, 60, 1.0), (4, 50, 49, 0.5), (3, 8, 200, 0.7)])
def test_whole_runs_agree_launch_for_launch(q, g, batch, n_in, p_fail):
    """a simulated run: every first decode fails with probability p_fail; the library's schedule and the restatement drive the same stack and must
    pick the same kind and size at every launch, flush included; the pool stays below S + batch"""
    failed = np.random.default_rng(g * 1000 + batch).random(n_in) < p_fail
    got, peak, drawn = mc_guess_ref.replay(failed, g, batch, schedule=q.mc_guess_next)
    want, peak_ref, _ = mc_guess_ref.replay(failed, g, batch)
    assert [(x["kind"], x["frames"]) for x in got] == [(x["kind"], x["frames"]) for x in want]
    S = batch >> g
    assert peak == peak_ref and peak < S + batch and drawn == n_in
    assert sorted(i for x in got if x["kind"] == mc_guess_ref.FRESH for i in x["frames"]) == list(range(n_in))
    tried = sorted(i for x in got if x["kind"] == mc_guess_ref.TRIALS for i in x["frames"])
    assert tried == ([int(i) for i in np.flatnonzero(failed)] if g else [])          # every failed frame got its trials exactly once
    ragged = [x for x in got if x["kind"] == mc_guess_ref.TRIALS and len(x["frames"]) < S]
    assert all(got.index(x) > max(i for i, y in enumerate(got) if y["kind"] == mc_guess_ref.FRESH) for x in ragged)      # ragged trial launches belong to the flush


def test_a_stopped_input_is_flushed(q):
    failed = np.ones(300, bool)
    failed[::3] = False
    seen = [0]

    def stop(launch):
        seen[0] += launch["kind"] == mc_guess_ref.TRIALS
        return seen[0] >= 2                                                        # the second trial launch ends the input

    got, _, drawn = mc_guess_ref.replay(failed, 3, 32, schedule=q.mc_guess_next, stop=stop)
    assert 0 < drawn < 300 and drawn % 32 == 0
    assert sorted(i for x in got if x["kind"] == mc_guess_ref.TRIALS for i in x["frames"]) == [i for i in range(drawn) if failed[i]]
    assert got[-1]["kind"] == mc_guess_ref.TRIALS and len(got[-1]["frames"]) < 4


def test_argument_errors_and_struct_sizes(q):
    weak = np.zeros(2, np.uint32)
    for args, status in [((0, 1, 0), -6), ((40, -1, 0), -6), ((40, 11, 0), -6), ((40, 3, 8), -6), ((40, 3, -1), -6)]:
        with pytest.raises(q.QldpcError) as e:
            q.guess_trial_host(args[0], args[1], args[2], weak, weak)
        assert e.value.status == status, args
    for N, g in [(0, 1), (40, -1), (40, 11)]:
        with pytest.raises(q.QldpcError) as e:
            q.guess_pick_host(N, g, np.zeros(2, np.int32), np.zeros((2, 2), np.uint32))
        assert e.value.status == -6, (N, g)
    for g, batch in [(-1, 8), (11, 4096), (3, 7), (0, 0)]:
        with pytest.raises(q.QldpcError) as e:
            q.mc_guess_next(g, batch, 0, 5)
        assert e.value.status == -6, (g, batch)
    L, up, ip = q._L, C.POINTER(C.c_uint32), C.POINTER(C.c_int)
    known, value = np.full(2, 77, np.uint32), np.full(2, 77, np.uint32)
    ptr = lambda a: a.ctypes.data_as(up)
    assert L.qldpc_guess_trial_host(40, 3, 0, None, ptr(weak), ptr(known), ptr(value)) == -1
    assert L.qldpc_guess_trial_host(40, 3, 0, ptr(weak), None, ptr(known), ptr(value)) == -1
    assert L.qldpc_guess_trial_host(40, 3, 0, ptr(weak), ptr(weak), None, ptr(value)) == -1
    assert L.qldpc_guess_trial_host(40, 3, 0, ptr(weak), ptr(weak), ptr(known), None) == -1
    assert L.qldpc_guess_trial_host(40, 3, 8, ptr(weak), ptr(weak), ptr(known), ptr(value)) == -6
    assert (known == 77).all() and (value == 77).all()                             # a refused call writes nothing
    ok, rows = np.zeros(8, np.int32), np.zeros((8, 2), np.uint32)
    w, n, a = C.c_int(-5), C.c_int(-5), C.c_int(-5)
    assert L.qldpc_guess_pick_host(40, 3, None, ptr(rows), C.byref(w), C.byref(n), C.byref(a)) == -1
    assert L.qldpc_guess_pick_host(40, 3, ok.ctypes.data_as(ip), None, C.byref(w), C.byref(n), C.byref(a)) == -1
    assert L.qldpc_guess_pick_host(40, 3, ok.ctypes.data_as(ip), ptr(rows), None, C.byref(n), C.byref(a)) == -1
    assert L.qldpc_guess_pick_host(40, 3, ok.ctypes.data_as(ip), ptr(rows), C.byref(w), None, C.byref(a)) == -1
    assert L.qldpc_guess_pick_host(40, 3, ok.ctypes.data_as(ip), ptr(rows), C.byref(w), C.byref(n), None) == -1
    assert L.qldpc_guess_pick_host(40, 11, ok.ctypes.data_as(ip), ptr(rows), C.byref(w), C.byref(n), C.byref(a)) == -6
    kind, cnt = C.c_int(-5), C.c_int(-5)
    assert L.qldpc_mc_guess_next_host(3, 40, 5, 10, None, C.byref(cnt)) == -1 and L.qldpc_mc_guess_next_host(3, 40, 5, 10, C.byref(kind), None) == -1
    assert L.qldpc_mc_guess_next_host(3, 7, 5, 10, C.byref(kind), C.byref(cnt)) == -6
    assert (w.value, n.value, a.value, kind.value, cnt.value) == (-5,) * 5
    # the device calls refuse before they touch the device
    for fn, nargs in [(L.qldpc_guess_expand_dev, 4), (L.qldpc_guess_pick_dev, 6)]:
        one = C.c_void_p(64)
        for missing in range(nargs):
            assert fn(40, 3, 1, *[None if i == missing else one for i in range(nargs)], None) == -1, (fn, missing)
        for N, g, n_src in [(0, 3, 1), (40, -1, 1), (40, 11, 1), (40, 3, -1), (40, 10, (1 << 14) + 1)]:
            assert fn(N, g, n_src, *[one] * nargs, None) == -6, (N, g, n_src)
        assert fn(40, 3, 0, *[one] * nargs, None) == 0                             # n_src = 0 queues nothing
    cfg, res = q.McGuessCfg(), q.McGuessResult()
    assert L.qldpc_mc_guess(None, C.byref(cfg), C.byref(res)) == -1
    assert L.qldpc_mc_guess_stats(None, None, 0) == -1 and L.qldpc_mc_guess_open(None, None, None, 0) == -1
    assert q.GUESS_MAX_BITS == 10 and C.sizeof(q.McGuessCfg) == 48 and C.sizeof(q.McGuessResult) == 12 * 8 + 10 * 8


def test_host_code_under_asan_ubsan(tmp_path):
    """the mirrors over random rows against a bit-by-bit restatement in C and the schedule driven to the end of simulated runs, as a stand-alone
    program (nothing loaded into Python is sanitised)"""
    exe = str(tmp_path / "guess_sanitize")
    csrc = os.path.join(ROOT, "qcrypto-ldpc_amd", "csrc")
    subprocess.check_call(["gcc", "-std=gnu11", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                           "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-o", exe, os.path.join(ROOT, "tests", "c", "guess_sanitize.c"),
                           os.path.join(csrc, "qldpc_guess_host.c"), os.path.join(csrc, "qldpc_mc_host.c"), os.path.join(csrc, "qldpc_graph.c"), "-lm"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "sanitizer pass ok" in r.stdout, r.stdout + r.stderr
