"""The deal of the QBER sweep (qldpc_mc_sweep_deal_host), host suite: the C mirror that qldpc_mc_sweep calls per round against the closed-form
numpy restatement of tests/mc_sweep_ref.py, state by state and over whole schedules.  Every comparison is exact equality."""
import os
import subprocess

import numpy as np
import pytest

import mc_sweep_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _states(rng):
    """(label, done, fe, C, S, max_frames, max_fe): the kinds of state the definition distinguishes, a few hundred of each"""
    for _ in range(400):      # more open points than slots: the lowest indices are served
        P, S = int(rng.integers(5, 40)), int(rng.integers(1, 5))
        C, mf = int(rng.integers(1, 20)), int(rng.integers(100, 1000))
        fe, max_fe = rng.integers(0, 50, P), int(rng.integers(1, 60))
        yield "more open than slots", rng.integers(0, mf // 2, P), fe, C, S, mf, max_fe
    for _ in range(400):      # one open point: it takes every slot it needs
        P, S, C, mf = int(rng.integers(1, 12)), int(rng.integers(1, 30)), int(rng.integers(1, 20)), int(rng.integers(50, 2000))
        done = np.full(P, mf)
        done[rng.integers(0, P)] = rng.integers(0, mf)
        yield "one open", done, np.zeros(P, np.int64), C, S, mf, 0
    for _ in range(400):      # every point capped by need: slots are left over
        P, C = int(rng.integers(1, 10)), int(rng.integers(1, 16))
        mf = int(rng.integers(40, 400))
        done = mf - rng.integers(1, 3 * C, P).clip(max=mf)
        yield "capped by need", done, np.zeros(P, np.int64), C, 64, mf, 0
    for _ in range(400):      # max_fe = 0: frame errors close nothing
        P, S, C, mf = int(rng.integers(1, 20)), int(rng.integers(1, 40)), int(rng.integers(1, 33)), int(rng.integers(1, 3000))
        yield "max_fe 0", rng.integers(0, mf + 1, P), rng.integers(0, 10 ** 6, P), C, S, mf, 0
    for _ in range(400):      # done next to max_frames: need = 1 with a ragged chunk
        P, S, C = int(rng.integers(1, 20)), int(rng.integers(1, 40)), int(rng.integers(2, 33))
        mf = int(rng.integers(C, 3000))
        yield "ragged", mf - rng.integers(0, C, P), rng.integers(0, 5, P), C, S, mf, int(rng.integers(0, 6))
    for _ in range(400):      # max_frames above 2^32
        P, S, C = int(rng.integers(1, 20)), int(rng.integers(1, 40)), int(rng.integers(1, 65))
        mf = 2 ** 32 + int(rng.integers(1, 2 ** 40))
        done = np.array([mf - int(rng.integers(0, 100)) if rng.random() < 0.5 else int(rng.integers(0, 2 ** 33)) for _ in range(P)], np.uint64)
        yield "above 2^32", done, rng.integers(0, 9, P), C, S, mf, int(rng.integers(0, 9))
    for _ in range(600):      # anything
        P, S, C, mf = int(rng.integers(1, 50)), int(rng.integers(1, 70)), int(rng.integers(1, 70)), int(rng.integers(1, 5000))
        yield "mixed", rng.integers(0, mf + 1, P), rng.integers(0, 20, P), C, S, mf, int(rng.integers(0, 20))


def test_deal_equals_the_closed_form(q):
    rng = np.random.default_rng(11)
    seen = {}
    for label, done, fe, C, S, mf, max_fe in _states(rng):
        done, fe = np.asarray(done, np.uint64), np.asarray(fe, np.uint64)
        got = q.mc_sweep_deal(done, fe, C, S, mf, max_fe)
        ref = mc_sweep_ref.deal(done, fe, C, S, mf, max_fe)
        need = np.array([min(n, 2 ** 31) for n in mc_sweep_ref.needs(done, fe, C, mf, max_fe)], np.int64)
        assert got.dtype == np.int32 and got.shape == ref.shape and (got == ref).all(), (label, done, fe, C, S, mf, max_fe, got, ref)
        assert got.sum() == min(S, need.sum()) and (got <= need).all()
        seen.setdefault(label, []).append((got, need, S))
    # each kind of state really occurred
    assert any((need > 0).sum() > S and (g[np.nonzero(need)[0][:S]] == 1).all() and g.sum() == S for g, need, S in seen["more open than slots"])
    assert all((need > 0).sum() <= 1 for _, need, _ in seen["one open"]) and any(g.max() > 1 for g, _, _ in seen["one open"])
    assert all((g == need).all() and g.sum() < S for g, need, S in seen["capped by need"])
    assert any((need == 1).all() for _, need, _ in seen["ragged"])
    assert len(seen) == 7 and sum(len(v) for v in seen.values()) == 3000


def _replay(q, fail, C, S, mf, max_fe):
    """the C mirror driven round by round, as qldpc_mc_sweep drives it"""
    P = fail.shape[0]
    done, fe, last = np.zeros(P, np.uint64), np.zeros(P, np.uint64), np.zeros(P, np.int64)
    rounds = 0
    while True:
        give = q.mc_sweep_deal(done, fe, C, S, mf, max_fe)
        if give.sum() == 0:
            break
        assert rounds < P * mf + 1, "the deal does not terminate"
        for p in np.nonzero(give)[0]:
            n = min(int(give[p]) * C, mf - int(done[p]))
            fe[p] += np.uint64(fail[p, int(done[p]):int(done[p]) + n].sum())
            done[p] += np.uint64(n)
            last[p] = rounds
        rounds += 1
    return done, fe, last, rounds


def test_replay_of_whole_schedules(q):
    rng = np.random.default_rng(12)
    reasons = set()
    for case in range(150):
        P, C = int(rng.integers(1, 12)), int(rng.integers(1, 20))
        S, mf = int(rng.integers(1, 14)), int(rng.integers(1, 400))
        max_fe = int(rng.integers(0, 40))
        fail = rng.random((P, mf)) < rng.choice([0.0, 0.02, 0.3, 1.0], (P, 1))
        ref = mc_sweep_ref.schedule(fail, C, S, mf, max_fe)
        done, fe, last, rounds = _replay(q, fail, C, S, mf, max_fe)
        assert (done == ref["frames"]).all() and (fe == ref["frame_errors"]).all() and (last == ref["last_round"]).all() and rounds == ref["rounds"], case
        closed = np.where(done >= mf, mc_sweep_ref.CLOSED_MAX_FRAMES, mc_sweep_ref.CLOSED_MAX_FE)
        assert (closed == ref["closed_by"]).all()
        assert ((done == mf) | ((max_fe > 0) & (fe >= max_fe))).all()          # every point is closed at the end
        reasons |= set(closed.tolist())
    assert reasons == {mc_sweep_ref.CLOSED_MAX_FE, mc_sweep_ref.CLOSED_MAX_FRAMES}


def test_deal_argument_checks(q):
    z = np.zeros(3, np.uint64)
    for kw in (dict(chunk=0), dict(slots=0), dict(max_frames=0), dict(chunk=-1)):
        args = dict(chunk=4, slots=4, max_frames=10)
        args.update(kw)
        with pytest.raises(q.QldpcError) as e:
            q.mc_sweep_deal(z, z, **args)
        assert e.value.status == -6, kw
    for n in (0, q.MC_SWEEP_MAX_POINTS + 1):
        with pytest.raises(q.QldpcError) as e:
            q.mc_sweep_deal(np.zeros(n, np.uint64), np.zeros(n, np.uint64), 4, 4, 10)
        assert e.value.status == -6
    assert q.mc_sweep_deal(np.zeros(q.MC_SWEEP_MAX_POINTS, np.uint64), np.zeros(q.MC_SWEEP_MAX_POINTS, np.uint64), 4, 5, 10).sum() == 5
    assert q._L.qldpc_mc_sweep_deal_host(3, 4, 4, 10, 0, None, None, None) == -1


def test_deal_mirror_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "mc_sweep_sanitize")
    csrc = os.path.join(ROOT, "qcrypto-ldpc_amd", "csrc")
    subprocess.check_call(["gcc", "-std=gnu11", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                           "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-o", exe, os.path.join(ROOT, "tests", "c", "mc_sweep_sanitize.c"),
                           os.path.join(csrc, "qldpc_mc_host.c"), os.path.join(csrc, "qldpc_graph.c"), "-lm"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "sanitizer pass ok" in r.stdout, r.stdout + r.stderr
