"""The CPU oracle's check-node rules against the float64 restatement (tests/check_rules_ref.py), one check update at a time.

No device.  This is where the tolerance of tests/test_check_rules_gpu.py gets its constants: the oracle is an fp32 evaluation of the
restated function, the kernels are another, and the caps K_MAX are twice what the oracle needs on these very inputs -- asserted here, so
the caps cannot hide a failure of the reference.  Run with -s to see the worst K per rule.
"""
import numpy as np
import pytest

import check_rules_ref as R

SCHEDULES = ("flooding", "hlayered")


@pytest.fixture(scope="module")
def inputs():
    return R.input_sets()


def oracle_posts(O, degrees, y, rule, param, sched):
    N, M, var, chk = R.forest(degrees)
    og = O.Graph.from_edges(N, M, var, chk)
    return O.decode(og, y, rule, param, 1, sched, False, 1)["post"]


@pytest.mark.parametrize("rule,param", R.SOFT_RULES)
def test_oracle_within_cap_of_restatement(O, inputs, rule, param):
    """fl32(y + M) of the oracle within tol(K_MAX) of the restatement on every element, both schedules; the only elements left out are the
    LSPA ones where the oracle returns inf through atanhf(1) (the kernels clamp there, the restatement follows the kernels), and at each of
    them the restatement must sit at or beyond the clamp."""
    worst, skipped = 0.0, 0
    for name, (deg, y) in inputs.items():
        for sched in SCHEDULES:
            M = R.messages_cached(rule, param, name, deg, y, sched)
            post = oracle_posts(O, deg, y, rule, param, sched)
            skip = None
            if rule == "LSPA":
                skip = ~np.isfinite(post)
                assert (np.abs(M[skip]) >= 2.0 * np.arctanh(R.CLAMP) - 1e-9).all(), "an inf of the oracle where the restatement is not saturated"
                skipped += int(skip.sum())
            else:
                assert np.isfinite(post).all()
            k, _ = R.worst_k(rule, deg, y, M, post, skip)
            print("oracle %-14s %-8s %-8s worst K = %.3f" % (rule, name, sched, k))
            worst = max(worst, k)
    print("oracle %-14s worst K = %.3f (cap %.3f), %d LSPA-inf elements left out" % (rule, worst, R.K_MAX[rule], skipped))
    assert worst <= R.K_MAX[rule]
    if rule == "LSPA":
        assert skipped > 0, "the inputs no longer reach the documented LSPA-inf class"
    if rule in R.K_MEASURED:      # the min* caps are twice the value measured here: the measured value must stay what the file says
        assert 0.5 * R.K_MAX[rule] == R.K_MEASURED[rule] and worst <= R.K_MEASURED[rule] * 1.0001


def test_forest_isolates_one_check_update(O):
    """post = fl32(y + m): on a forest the oracle's min-sum posterior is the plain two-minimum rule of each check, on both schedules"""
    deg = R.FORESTS["A"]
    y = R.frames(deg, R.SOFT_FAMILIES, seed=1, F=12)[0]
    want = np.empty_like(y)
    for sl in R.check_slices(deg):
        x = y[:, sl]
        a = np.abs(x)
        neg = np.logical_xor(np.logical_xor.reduce(np.signbit(x), axis=1)[:, None], np.signbit(x))
        if x.shape[1] == 1:
            other = np.full_like(a, R.FLT_MAX)
        else:
            srt = np.sort(a, axis=1)
            other = np.where(a == srt[:, :1], srt[:, 1:2], srt[:, :1])
        want[:, sl] = x + np.where(neg, -other, other).astype(np.float32)
    for sched in SCHEDULES:
        assert (oracle_posts(O, deg, y, "MS", 0.0, sched) == want).all()


def test_restatement_known_values():
    clamp = 2.0 * np.arctanh(R.CLAMP)
    for rule in ("SPA", "LSPA"):
        assert R.cn_out(rule, 0.0, [1.5])[0] == clamp                                  # degree 1: the empty product is 1, clamped
        m = R.cn_out(rule, 0.0, [3.0, -2.0])
        assert np.allclose(m, [-2.0, 3.0], rtol=1e-12)                                 # degree 2: each edge gets the other
        x = np.array([0.7, -1.9, 2.6, -0.4])
        t = np.tanh(np.abs(x) / 2)
        want = np.array([2 * np.arctanh(np.prod(np.delete(t, i))) * np.prod(np.sign(np.delete(x, i))) for i in range(4)])
        assert np.allclose(R.cn_out(rule, 0.0, x), want, rtol=1e-12)
    m = R.cn_out("SPA", 0.0, [0.0, 2.6, -2.6])                                         # an erased edge: its own message is the clamp, the others get 0
    assert m[0] == -clamp and (m[1:] == 0).all()
    m = R.cn_out("LSPA", 0.0, [0.0, 2.6, -2.6])                                        # LSPA: the erased edge's term is FLT_MIN, i.e. it counts as certain
    assert np.allclose(m, [-2.0 * np.arctanh(np.tanh(1.3) ** 2), -2.6, 2.6], rtol=1e-9)
    m = R.cn_out("SPA", 0.0, [1e-8, 3.0])                                              # a tiny non-zero input is not an erasure
    assert np.allclose(m, [3.0, 1e-8 * np.tanh(1.5)], rtol=1e-6)
    for rule in ("AMS_MINSTAR", "AMS_MINSTAR_L2"):
        m = R.cn_out(rule, 0.0, [5.0, -0.25, 9.0])
        assert (np.sign(m) == [-1, 1, -1]).all() and abs(m[0]) <= 0.25 and abs(m[1]) <= 5.0


@pytest.mark.parametrize("rule,param", R.SOFT_RULES)
def test_caps_catch_a_dropped_edge(rule, param):
    """a check of degree 6 at |LLR| = 2.6 that loses one edge moves its messages by about 0.15: five orders of magnitude beyond the cap"""
    deg = (6,)
    y = R.frames(deg, ("bsc",), seed=5, F=8)[0]
    M = R.messages(rule, param, deg, y)
    wrong = M.copy()
    wrong[:, :5] = R.messages(rule, param, (5,), y[:, :5])
    k, _ = R.worst_k(rule, deg, y, M, (y + wrong).astype(np.float32))
    assert k > 1e3 * R.K_MAX[rule]
    k0, _ = R.worst_k(rule, deg, y, M, (y + M).astype(np.float32))
    assert k0 == 0.0
