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


# ---------------------------------------------------------------- the syndrome form: a target bit per check ----------

TARGET_SETS = ("A", "B", "C", "W")
HARD_WORD_SETS = ("A-hard", "B-hard")


def u64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("rule,param", R.SOFT_RULES)
def test_target_is_an_exact_sign_flip(rule, param):
    """cn_out with s = 1 is cn_out with s = 0 negated, the clamp message of an erased edge and a zero message included: the shortcut of
    messages_cached() is messages(..., target=) bit for bit"""
    clamp = 2.0 * np.arctanh(R.CLAMP)
    m0, m1 = R.cn_out(rule, param, [0.0, 2.6, -2.6]), R.cn_out(rule, param, [0.0, 2.6, -2.6], 1)
    assert (u64(m1) == u64(-m0)).all()
    if rule == "SPA":
        assert m1[0] == clamp and (m1[1:] == 0).all() and (np.signbit(m1) == [False, False, True]).all()
    assert R.cn_out(rule, param, [1.5], 1)[0] == -R.cn_out(rule, param, [1.5])[0] < 0
    deg, y = R.input_sets()["A"]
    t = R.target_cached("A")
    assert (u64(R.messages(rule, param, deg, y[:12], target=t[:12])) == u64(R.messages_cached(rule, param, "A", deg, y, "hlayered", t)[:12])).all()


def test_targets_are_what_they_say():
    for name in TARGET_SETS + ("A-coded", "B-coded"):
        deg, y = R.input_sets()[name]
        t = R.target_cached(name)
        assert t.shape == (len(y), len(deg)) and t.dtype == np.uint8 and not t[0].any() and t[1].all()
        cons = np.arange(len(y)) % 4 == 2
        assert R.syndrome_matches(deg, np.signbit(y), t)[cons].all()
        rest = ~cons
        rest[:2] = False
        assert 0.4 < t[rest].mean() < 0.6
    assert len(R.FORESTS["W"]) == 70 and sum(R.FORESTS["W"]) == 480      # a target row of three words, the last one ragged


@pytest.mark.parametrize("rule,param", R.SOFT_RULES)
def test_oracle_with_target_within_cap_of_restatement(O, inputs, rule, param):
    """the oracle's coset mode within tol(K_MAX) of the restatement with the same target, both schedules, sets A, B, C, W; frame 0 (target all 0)
    is the oracle's answer without a target, bit for bit.  Left out: the LSPA atanhf(1) elements, as above."""
    worst, skipped = 0.0, 0
    for name in TARGET_SETS:
        deg, y = inputs[name]
        t = R.target_cached(name)
        N, Mc, var, chk = R.forest(deg)
        og = O.Graph.from_edges(N, Mc, var, chk)
        for sched in SCHEDULES:
            M = R.messages_cached(rule, param, name, deg, y, sched, t)
            post = O.decode(og, y, rule, param, 1, sched, False, 1, target=t)["post"]
            assert (post[0].view(np.uint32) == oracle_posts(O, deg, y[:1], rule, param, sched)[0].view(np.uint32)).all()
            skip = None
            if rule == "LSPA":
                skip = ~np.isfinite(post)
                assert (np.abs(M[skip]) >= 2.0 * np.arctanh(R.CLAMP) - 1e-9).all()
                skipped += int(skip.sum())
            else:
                assert np.isfinite(post).all()
            k, _ = R.worst_k(rule, deg, y, M, post, skip)
            print("oracle under a target %-14s %-3s %-8s worst K = %.3f" % (rule, name, sched, k))
            worst = max(worst, k)
    print("oracle under a target %-14s worst K = %.3f (cap %.3f), %d LSPA-inf elements left out" % (rule, worst, R.K_MAX[rule], skipped))
    assert worst <= R.K_MAX[rule]
    if rule == "LSPA":
        assert skipped > 0


def wrong_targets(t):
    """name -> the target bits a faulty kernel body would use in place of t[F, M]"""
    F, Mc = t.shape
    other_lane = np.where(np.arange(F) + 64 < F, np.arange(F) + 64, np.arange(F) - 64)      # the other frame of the lane at 2 or 4 frames per lane
    out = {
        "ignored": np.zeros_like(t),
        "check c + 1": np.roll(t, -1, axis=1),
        "frame f + 1": np.roll(t, -1, axis=0),
        "frame f +- 64": t[other_lane],
        "applied twice": t ^ t,
    }
    if Mc > 32:      # MSB-first words read LSB-first: bit j of a word taken for bit 31 - j
        pad = np.zeros((F, (Mc + 31) // 32 * 32), np.uint8)
        pad[:, :Mc] = t
        out["words read LSB-first"] = pad.reshape(F, -1, 32)[:, :, ::-1].reshape(F, -1)[:, :Mc]
    return out


@pytest.mark.parametrize("rule,param", R.SOFT_RULES)
def test_caps_catch_a_wrong_target(inputs, rule, param):
    """A condition on the inputs: each mistake in where the target bit comes from puts the posterior beyond tol(K_MAX) on every check of degree
    >= 2 in at least one frame (a saturated message hides a flip -- tol grows with sinh |M| -- so not in every frame)"""
    for name in TARGET_SETS:
        deg, y = inputs[name]
        t = R.target_cached(name)
        M = R.messages_cached(rule, param, name, deg, y, "hlayered", t)
        base = R.messages_cached(rule, param, name, deg, y, "hlayered")
        wrongs = wrong_targets(t)
        assert ("words read LSB-first" in wrongs) == (name == "W")
        for what, tw in wrongs.items():
            bad = np.where(R.per_vn(deg, tw) != 0, -base, base)
            with np.errstate(over="ignore"):
                k = R.worst_k(rule, deg, y, M, (y + bad).astype(np.float32))[1]
            seen = np.array([(k[:, sl] > R.K_MAX[rule]).any() for sl in R.check_slices(deg)])
            frames_hit = np.mean([(k[:, sl] > R.K_MAX[rule]).any(axis=1).mean() for sl in R.check_slices(deg) if sl.stop - sl.start >= 2])
            print("wrong target %-14s %-2s %-22s caught on %d of %d checks, in %.0f %% of the frames of a check, worst K = %.3g"
                  % (rule, name, what, seen.sum(), len(deg), 100 * frames_hit, k[np.isfinite(k)].max()))
            assert seen[np.asarray(deg) >= 2].all(), (rule, name, what)


@pytest.mark.parametrize("rule,param", R.SOFT_RULES)
def test_hard_word_exclusions_stay_below_one_percent(inputs, rule, param):
    """the elements whose hard decision the tolerance leaves open (hard_ref) are at most 1 % of each set the device's hard words are compared
    on (tests/test_check_rules_gpu.py, HARD_WORD_SETS)"""
    for name in HARD_WORD_SETS:
        deg, y = R.get_set(name)
        for sched in SCHEDULES:
            M = R.messages_cached(rule, param, name, deg, y, sched, R.target_cached(name))
            skip = R.hard_ref(rule, deg, y, M)[1]
            print("hard word %-14s %-2s %-8s %d of %d elements left out" % (rule, name, sched, skip.sum(), skip.size))
            assert skip.mean() <= 0.01


# ---------------------------------------------------------------- binary16 message storage ----------

F16_SETS = ("A", "B", "C", "tiny", "high")


def f16_post(y, h):
    """fl32(y + fl32(0 + h)): the flooding posterior of a VN whose one stored message is h"""
    with np.errstate(over="ignore"):
        return (np.asarray(y, np.float32) + (np.float32(0.0) + np.asarray(h).astype(np.float32))).astype(np.float32)


def test_accept_f16_known_values():
    y = np.array([1.0, 1.0, 1.0, -0.0, 2.0, 0.5], np.float32)
    lo = np.array([0.5, 0.5, 0.5, 0.0, np.inf, 2.0 ** -24], np.float16)
    hi = np.array([0.5, 0.5, 0.75, 0.0, np.inf, 2.0 ** -24], np.float16)
    post = np.array([1.5, 1.5 + 2.0 ** -12, 1.5 + 2.0 ** -11, 0.0, np.inf, 0.5 + 2.0 ** -24], np.float32)
    assert R.accept_f16(y, post, lo, hi).tolist() == [True, False, True, True, True, True]
    assert not R.accept_f16(y[3:4], np.array([-0.0], np.float32), lo[3:4], hi[3:4])[0]      # -0.0 + (0 + 0) is +0.0
    assert not R.accept_f16(y[:1], np.array([1.5 + 2.0 ** -20], np.float32), lo[:1], hi[2:3])[0]      # y plus an fp32 number that is no binary16 number
    assert (R.rne16(np.array([1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1e-6, 2.0 ** -25, 1e5], np.float32))
            == np.array([1.0, 1.0 + 2.0 ** -9, 17 * 2.0 ** -24, 0.0, np.inf], np.float32)).all()


@pytest.mark.parametrize("rule,param", R.SOFT_RULES)
def test_oracle_with_binary16_storage_passes_accept_f16(O, inputs, rule, param):
    """msg_fp16 on the oracle (stq() rounds every stored message): every posterior is y plus a binary16 number inside [lo16, hi16] of the
    restatement on x16.  Left out: the LSPA atanhf(1) elements only.  A check of degree 1 sends FLT_MAX under the AMS rules, which binary16
    stores as inf: the posterior is +-inf there (as under the min-sum family), and nowhere else"""
    skipped = 0
    for name in F16_SETS:
        deg, y = inputs[name]
        x16, M, lo, hi = R.f16_interval_cached(rule, param, name)
        N, Mc, var, chk = R.forest(deg)
        post = O.decode(O.Graph.from_edges(N, Mc, var, chk), y, rule, param, 1, "flooding", False, 1, msg_fp16=True)["post"]
        ok = R.accept_f16(y, post, lo, hi)
        if rule == "LSPA":
            skip = ~np.isfinite(post) & np.isfinite(lo)
            assert (np.abs(M[skip]) >= 2.0 * np.arctanh(R.CLAMP) - 1e-9).all()
            skipped += int(skip.sum())
            ok |= skip
        d1 = R.per_vn(deg, np.asarray(deg)[None, :] == 1)[0]
        if rule.startswith("AMS"):
            assert np.isinf(post[:, d1]).all() and (np.signbit(post[:, d1]) == np.signbit(M[:, d1])).all()
        assert (np.isinf(post) == np.isinf(lo)).all() or rule == "LSPA"
        assert np.isfinite(post[:, ~d1]).all() or rule == "LSPA"
        sharp = lo == hi
        print("oracle f16 %-14s %-5s sharp share %.3f, %d of %d elements matched only inside a wider interval" % (rule, name, sharp.mean(), (ok & ~sharp).sum(), ok.size))
        assert ok.all(), "%s %s: %d elements fail accept_f16" % (rule, name, (~ok).sum())
    if rule == "LSPA":
        print("oracle f16 LSPA: %d LSPA-inf elements left out" % skipped)
        assert skipped > 0


@pytest.mark.parametrize("rule,param", R.SOFT_RULES)
def test_sharp_share_floors(rule, param):
    """the share of elements at which accept_f16 is a bit-exact comparison (lo16 == hi16) stays above 0.8 of what was measured"""
    for name in ("A", "B", "C"):
        _, _, lo, hi = R.f16_interval_cached(rule, param, name)
        share = float((lo == hi).mean())
        print("sharp share %-14s %s %.4f (measured %.3f)" % (rule, name, share, R.SHARP_MEASURED[rule][name]))
        assert abs(share - R.SHARP_MEASURED[rule][name]) < 0.006, "the measured value next to the constant is stale"
        assert share >= 0.8 * R.SHARP_MEASURED[rule][name]


def f16_mutants(rule, param, name, logu_only=False):
    """name -> (posteriors of a faulty binary16 path, the elements it is judged on)"""
    deg, y = R.input_sets()[name]
    x16, M, lo, hi = R.f16_interval_cached(rule, param, name)
    with np.errstate(over="ignore"):
        h = M.astype(np.float16)
        h_y = R.messages_cached(rule, param, name, deg, y, "flooding").astype(np.float16)
        away = np.abs(h.astype(np.float64)) > np.abs(M)
        h_trunc = np.where(away, np.nextafter(h, np.float16(0.0)), h)
        h_ftz = np.where(np.abs(h) < np.float16(2.0 ** -14), np.copysign(np.float16(0.0), h), h)
    return {
        "inputs not rounded": f16_post(y, h_y),
        "message not rounded": (y + M.astype(np.float32)).astype(np.float32),
        "message truncated": f16_post(y, h_trunc),
        "subnormals flushed": f16_post(y, h_ftz),
    }


@pytest.mark.parametrize("rule,param", R.SOFT_RULES)
def test_accept_f16_catches_a_faulty_binary16_path(rule, param):
    """Each fault fails accept_f16 on at least 20 % of the elements where the comparison is bit-exact: of forest A for the first three; a flush
    of binary16 subnormals to zero is judged where a flush can show at all -- the sharp elements of "tiny" and of A's log-uniform family whose
    message is a non-zero binary16 subnormal"""
    deg, y = R.input_sets()["A"]
    _, M, lo, hi = R.f16_interval_cached(rule, param, "A")
    sharp = lo == hi
    mut = f16_mutants(rule, param, "A")
    with np.errstate(over="ignore"):
        assert R.accept_f16(y, f16_post(y, M.astype(np.float16)), lo, hi).all()      # the faithful path passes
    for what in ("inputs not rounded", "message not rounded", "message truncated"):
        share = float((~R.accept_f16(y, mut[what], lo, hi))[sharp].mean())
        print("f16 fault %-14s %-20s fails on %.3f of the sharp elements of A" % (rule, what, share))
        assert share >= 0.20, (rule, what, share)
    fails, n = 0, 0
    for name in ("tiny", "A"):
        deg, y = R.input_sets()[name]
        _, M, lo, hi = R.f16_interval_cached(rule, param, name)
        with np.errstate(over="ignore"):
            h = M.astype(np.float16)
        judged = (h != 0) & (np.abs(h) < np.float16(2.0 ** -14))
        bad = ~R.accept_f16(y, f16_mutants(rule, param, name)["subnormals flushed"], lo, hi)
        assert not (bad & ~judged).any()
        print("f16 fault %-14s subnormals flushed   fails on %d of %d judged elements of %s" % (rule, (bad & judged).sum(), judged.sum(), name))
        fails, n = fails + int((bad & judged).sum()), n + int(judged.sum())
    assert n >= 50 and fails >= 0.20 * n, (rule, fails, n)
