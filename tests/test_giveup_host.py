"""The give-up rule of the early-exit run on the host (qldpc_giveup_host, the mirror of csrc/qldpc_giveup_core.h): against the plain Python
restatement of tests/giveup_ref.py on the CPU oracle's syndrome-weight trajectories of the 576 frames the GPU tests decode.  No device."""
import numpy as np
import pytest

import giveup_ref as R


@pytest.mark.parametrize("kind", ["flood", "hlay"])
@pytest.mark.parametrize("depth", [1, 2])
@pytest.mark.parametrize("patience", [1, 6, 30])
def test_host_mirror_equals_the_restated_rule(q, O, kind, depth, patience):
    traj = R.trajectory(q, O, kind)
    T = R.n_tests(traj["layered"])
    seen = np.zeros(3, int)
    for f in range(R.FRAMES):
        w = traj["weight"][f, :T]
        stop, what, _, _ = R.walk(w, patience, depth)
        assert q.giveup_host(w, patience, depth) == (stop, what), f
        seen[what] += 1
    print(kind, depth, patience, seen)
    assert seen[R.CONVERGED] > 0 and (seen[R.GAVE_UP] > 0) == (patience < T)


@pytest.mark.parametrize("kind", ["flood", "hlay"])
@pytest.mark.parametrize("depth", [1, 2])
def test_patience_of_every_test_never_gives_up_and_is_the_oracle_early_exit(q, O, kind, depth):
    traj = R.trajectory(q, O, kind)
    _, og, ogl, _ = R.graphs(q, O)
    T = R.n_tests(traj["layered"])
    ref = O.decode(ogl if traj["layered"] else og, R.llr_of(R.flips()), "NMS", 0.75, R.N_ITE, "hlayered" if traj["layered"] else "flooding", True, depth, n_threads=8)
    for patience in (T, T + 5, 0):
        for f in range(R.FRAMES):
            stop, what = q.giveup_host(traj["weight"][f, :T], patience, depth)
            assert what != R.GAVE_UP
            assert (stop if stop else R.N_ITE) == ref["iters"][f], (f, stop, what)
    exp = R.expected(traj, T, depth)
    assert (exp["iters"] == ref["iters"]).all() and (exp["hard"] == ref["hard"]).all() and (exp["ok"] == ref["synd_ok"]).all() and not exp["gave"].any()


@pytest.mark.parametrize("kind,patience", [("flood", 6), ("flood_i8", 6), ("hlay", 8)])
@pytest.mark.parametrize("F", [R.SMALL, R.LARGE])
def test_the_inputs_hold_every_outcome(q, O, kind, patience, F):
    """what the GPU tests assert before they look at the device"""
    exp = R.expected(R.trajectory(q, O, kind), patience, frames=np.arange(F))
    print(kind, patience, F, R.assert_mix(exp), "false give-ups", int(exp["false"].sum()), "iteration sum", int(exp["iters"].sum()))


def test_argument_checks(q):
    w = np.array([5, 4, 4, 0], np.int32)
    assert q.giveup_host(w, 1) == (3, R.GAVE_UP) and q.giveup_host(w, 2) == (4, R.CONVERGED) and q.giveup_host(w[:3], 0) == (0, R.RAN_OUT)
    assert q.giveup_host([0, 3, 0, 0], 3, 2) == (4, R.CONVERGED) and q.giveup_host([0, 3, 0, 0], 3, 3) == (0, R.RAN_OUT)
    for bad in (dict(weights=w, patience=-1), dict(weights=w[:0], patience=1), dict(weights=w, patience=1, syndrome_depth=0), dict(weights=[3, -1], patience=1)):
        with pytest.raises(q.QldpcError) as e:
            q.giveup_host(**bad)
        assert e.value.status == -1, bad
