"""Single-check tests of the eight check-node rules on the device: every kernel body that folds a check, on forests of disjoint checks
where one iteration gives post = fl32(y + m) (tests/check_rules_ref.py).

  soft rules (SPA, LSPA, AMS_MINSTAR, AMS_MINSTAR_L2)   every posterior within tol(K_MAX) of the float64 restatement; no element excluded
  min-sum family (MS, OMS, NMS, AMS_MIN)                posteriors bit-equal to the CPU oracle, special values (+-0.0, denormals, FLT_MAX) included
  coded LLR form                                        load_bits + load_erasures bit-equal to load_llr of the same values, every rule
  under a target (load_syndrome)                        all of the above again with a target bit per (frame, check), forest W (70 checks) added; the ok
                                                        flag against the syndrome of the device's own hard word, the hard word against the reference
  soft rules with binary16 storage                      every posterior y plus a binary16 number inside the restatement's [lo16, hi16] (accept_f16)

The worst K per (rule, engine, schedule) is printed (run with -s); DESIGN.md records the values of one MI355X run.
"""
import numpy as np
import pytest

import check_rules_ref as R
import vlayered_ref

pytestmark = pytest.mark.gpu

EUNSUPPORTED = -7
VS = (1, 2, 4)


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def codes(q, O):
    """name -> (degrees, Code, oracle Graph) of every forest"""
    out = {}
    for name, deg in list(R.FORESTS.items()) + [("high", R.HIGH_DEGREES), ("tiny", R.TINY_DEGREES)]:
        N, M, var, chk = R.forest(deg)
        assert N < 1000
        out[name] = (deg, q.Code.from_edges(N, M, var, chk), O.Graph.from_edges(N, M, var, chk))
    return out


def decoder(q, code, F, rule, param, **kw):
    return q.Decoder(code, code.N, 1, rule=rule, rule_param=param, n_frames=F, enable_syndrome=False, compact="off", **kw)


def words(q, torch, bits):
    """bits[F, n] of 0 / 1 -> the packed MSB-first int32 rows the loaders take, on the device"""
    return torch.from_numpy(np.ascontiguousarray(q.pack_bits(bits)).view(np.int32)).cuda()


def run_llr(torch, dec, y, chunk=None, target=None, q=None):
    """load_llr (-> load_syndrome of target[F, M]) -> run -> fetch_post, `chunk` frames at a time (the edge engine takes 8)"""
    y = np.array(y, np.float32)      # a writable copy: the shared input sets are read-only
    chunk = chunk or len(y)
    post = np.empty(y.shape, np.float32)
    for lo in range(0, len(y), chunk):
        dec.load_llr(torch.from_numpy(y[lo:lo + chunk]).cuda())
        if target is not None:
            dec.load_syndrome(words(q, torch, target[lo:lo + chunk]))
        dec.run()
        post[lo:lo + chunk] = dec.fetch_post().cpu().numpy()
    return post


def bits_equal(a, b):
    return (np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)).all()


# mode -> (engine, schedule, decoder keywords, frames_per_lane values, input sets, frames per load)
ALL = ("A", "B", "C", "A-coded", "B-coded", "C-coded", "tiny")
SOFT_MODES = {
    "frames-flooding": ("frames", "flooding", {}, VS, ALL, None),
    "frames-hlayered": ("frames", "hlayered", {"layer_chain": "off"}, VS, ALL, None),
    "frames-vlayered": ("frames", "vlayered", {}, VS, ALL, None),
    "frames-hlayered-chain": ("frames", "hlayered", {"layer_chain": "on"}, (1,), ("A", "A-coded"), None),      # the one-launch sweep: 64-frame groups, degree <= 40
    "edges-flooding": ("edges", "flooding", {}, (0,), ("A", "B", "A-coded", "B-coded", "tiny"), 8),                # SPA only; check degree <= 64
    "f16-flooding": ("frames", "flooding", {"msg_dtype": "f16"}, VS, ("A", "B", "C", "A-coded", "B-coded", "C-coded", "tiny", "high"), None),      # binary16 storage: held to accept_f16, not to K (below)
}
# the sets each mode runs under a target: A, B, C and W (M = 70: three target words) and the coded sets; the edge engine stops at degree 64, the
# one-launch sweep at 40
TARGET_SETS = {
    "frames-flooding": ("A", "B", "C", "W", "A-coded", "B-coded"),
    "frames-hlayered": ("A", "B", "C", "W", "A-coded", "B-coded"),
    "frames-vlayered": ("A", "B", "C", "W", "A-coded", "B-coded"),
    "frames-hlayered-chain": ("A", "W", "A-coded"),
    "edges-flooding": ("A", "B", "W", "A-coded", "B-coded"),
    "f16-flooding": ("A", "W"),
}


def soft_worst_k(q, torch, codes, rule, param, mode, sets=None, target=False):
    """worst K of `mode` over its input sets; target: every set under R.target_cached(set), loaded through load_syndrome after each load_llr,
    and frame 0 (its target is all 0) must then equal the same decoder's run without load_syndrome bit for bit"""
    engine, sched, kw, vs, names, chunk = SOFT_MODES[mode]
    worst = 0.0
    for name in sets or names:
        if name == "tiny" and rule == "SPA":
            name = "tiny-spa"      # SPA's stated domain is x = 0 or |x| >= 2^-24; test_spa_below_its_domain pins what it does below
        deg, y = R.input_sets()[name]
        code = codes[name.split("-")[0]][1]
        t = R.target_cached(name) if target else None
        M = R.messages_cached(rule, param, name, deg, y, sched, t)
        skip = None
        if sched == "vlayered":      # only the VN of each check that is swept first is updated from the channel values alone (check_rules_ref.py)
            skip = np.broadcast_to(~R.first_swept(deg, code.vlayer_order()[0])[None, :], y.shape)
        for V in vs:
            dec = decoder(q, code, chunk or len(y), rule, param, engine=engine, schedule=sched, frames_per_lane=V, **kw)
            post = run_llr(torch, dec, y, chunk, t, q)
            assert np.isfinite(post).all()
            k, per = R.worst_k(rule, deg, y, M, post, skip)
            if not k <= R.K_MAX[rule]:
                f, v = np.unravel_index(np.argmax(per), per.shape)
                sl = [s for s in R.check_slices(deg) if s.start <= v < s.stop][0]
                print("gpu %-14s %-22s set %-8s V=%d target=%d: K = %.4g at frame %d VN %d (check of degree %d): y = %r, restatement M = %r, posterior %r"
                      % (rule, mode, name, V, target, k, f, v, sl.stop - sl.start, float(y[f, v]), float(M[f, v]), float(post[f, v])))
            worst = max(worst, k)
            if target:
                plain = run_llr(torch, dec, y[:chunk or len(y)], chunk)
                assert bits_equal(post[0], plain[0]), "%s %s set %s V=%d: frame 0, whose target is all 0, differs from the run without a target" % (rule, mode, name, V)
    return worst


# the edge engine runs MS / OMS / NMS / SPA; binary16 storage has its own acceptance rule (below)
SOFT_CASES = [(r, p, m) for r, p in R.SOFT_RULES for m in SOFT_MODES if m != "f16-flooding" and (m != "edges-flooding" or r == "SPA")]


@pytest.mark.parametrize("rule,param,mode", SOFT_CASES)
def test_soft_rules_within_cap_of_restatement(q, torch, codes, rule, param, mode):
    """Every posterior of one check update within tol(K_MAX) of fl32(y + M_ref): forests A, B, C (every register bucket and its first overflow,
    the generic any-degree body), the six input families, the QKD-mix values of the coded sets, inputs of 1e-8 .. 1e-6 (SPA: 2^-24 and 1e-6, its domain), 1 / 2 / 4 frames per
    lane, 130 frames (two full groups and a ragged one).  No element is left out under the flooding and horizontal-layered schedules; under the
    vertical-layered one the comparison is on the VN of each check that is swept first, the only one whose check sees the channel values."""
    k = soft_worst_k(q, torch, codes, rule, param, mode)
    print("gpu %-14s %-22s worst K = %.3f (cap %.3f)" % (rule, mode, k, R.K_MAX[rule]))
    assert k <= R.K_MAX[rule]


@pytest.mark.parametrize("rule,param,mode", SOFT_CASES)
def test_soft_rules_under_a_target(q, torch, codes, rule, param, mode):
    """The syndrome form, one check at a time: the same comparison with a target bit per (frame, check) loaded through load_syndrome -- frame 0
    all 0, frame 1 all 1, every fourth frame consistent with sign(y), the rest coin flips (check_rules_ref.targets) -- on forests A, B, C, on W
    (70 checks: a target row of three words, the last one ragged) and on the coded sets.  The restatement flips the sign of every message of a
    check whose bit is set; tests/test_check_rules_host.py shows that a target that is ignored, taken from the next check, the next frame or
    the other frame of the lane, applied twice or read LSB-first lands beyond the cap on every check of degree >= 2."""
    k = soft_worst_k(q, torch, codes, rule, param, mode, sets=TARGET_SETS[mode], target=True)
    print("gpu %-14s %-22s under a target: worst K = %.3f (cap %.3f)" % (rule, mode, k, R.K_MAX[rule]))
    assert k <= R.K_MAX[rule]


@pytest.mark.parametrize("mode", ["frames-flooding", "frames-hlayered", "edges-flooding"])
def test_spa_below_its_domain(q, torch, codes, mode):
    """Pins what the SPA kernels do with 0 < |x| < 2^-25, outside their stated domain (x = 0 or |x| >= 2^-24): exp(-|x|) rounds to 1 and the edge
    is folded as an ERASED edge that keeps the sign of x -- its own message is the clamp, 16.6 with the sign of the other edges' product, where
    AFF3CT's division form gives the product of the other edges (3.0 for a degree-2 check whose other input is 3.0); what the other edges
    receive is 0 against a true message below 2^-25.  Keeping such inputs apart costs one compare pair and one select per edge, measured at 0.4 %
    of a fixed-iteration SPA step on the benchmark's code, and no channel LLR, pinned bit or erased bit of a QKD frame is
    one, so it is not paid for.  2^-25 itself is a rounding tie: either reading is accepted there."""
    engine, sched, kw, _, _, chunk = SOFT_MODES[mode]
    deg, y = R.input_sets()["tiny"]
    tiny = (np.abs(y) < np.float32(R.SPA_DOMAIN_MIN)) & (y != 0)
    frames_below = tiny.any(axis=1)
    assert 0 < frames_below.sum() < len(y)
    erased = np.where(tiny, np.copysign(np.float32(0.0), y), y).astype(np.float32)
    M_true = R.messages_cached("SPA", 0.0, "tiny", deg, y, "hlayered")
    M_erased = R.messages("SPA", 0.0, deg, erased)
    assert (np.abs(M_erased[tiny]) == 2.0 * np.arctanh(R.CLAMP)).all()
    post = run_llr(torch, decoder(q, codes["tiny"][1], chunk or len(y), "SPA", 0.0, engine=engine, schedule=sched, **kw), y, chunk)
    k_true = R.worst_k("SPA", deg, y, M_true, post)[1]
    k_erased = R.worst_k("SPA", deg, y, M_erased, post)[1]
    tie = (np.abs(y) == np.float32(2.0 ** -25)).any(axis=1)
    strict = frames_below & ~tie
    assert strict.sum() >= 2 * len(R.TINY_DEGREES) and tie.any()
    assert (k_erased[strict] <= R.K_MAX["SPA"]).all()                                       # below the tie: the erased reading
    assert (k_true[strict][tiny[strict]] > 1e3).all()                                        # ... and it IS far from the division form on the edge itself
    assert (np.minimum(k_erased, k_true)[tie] <= R.K_MAX["SPA"]).all()                      # the tie: one of the two
    assert (k_true[~frames_below] <= R.K_MAX["SPA"]).all()                                  # inside the domain: the restatement


# ---------------------------------------------------------------- min-sum family: bit-equal to the oracle ----------

def ms_inputs(name):
    deg = R.FORESTS[name]
    return deg, R.frames(deg, R.MS_FAMILIES, seed=500 + ord(name))[0]


MS_MODES = {
    # mode -> (engine, schedule, oracle schedule, decoder kw, oracle kw, Vs, rules, frames per load)
    "frames-flooding": ("frames", "flooding", "flooding", {}, {}, VS, "all", None),
    "frames-hlayered": ("frames", "hlayered", "hlayered", {}, {}, VS, "all", None),
    "frames-vlayered": ("frames", "vlayered", None, {}, {}, VS, "all", None),            # reference: tests/vlayered_ref.py in the code's class order
    "edges-flooding": ("edges", "flooding", "flooding", {}, {}, (0,), ("MS", "OMS", "NMS"), 8),
    "f16-flooding": ("frames", "flooding", "flooding", {"msg_dtype": "f16"}, {"msg_fp16": True}, VS, "all", None),
    "i8-flooding": ("frames", "flooding", "flooding", {"msg_dtype": "i8"}, {"msg_i8": True, "quant_scale": 8.0}, (0,), ("MS", "OMS", "NMS"), None),
    "i8-hlayered": ("frames", "hlayered", "hlayered", {"msg_dtype": "i8"}, {"msg_i8": True, "quant_scale": 8.0}, (0,), ("MS", "OMS", "NMS"), None),
}


MS_CASES = [(r, p, m) for r, p in R.MS_RULES for m in MS_MODES if MS_MODES[m][6] == "all" or r in MS_MODES[m][6]]


_MS_TARGET = {}


def ms_target(name):
    """the target bits of ms_inputs(name), uint8 [F, M]"""
    if name not in _MS_TARGET:
        deg, y = ms_inputs(name)
        _MS_TARGET[name] = R.targets(deg, y, seed=800 + ord(name))
    return _MS_TARGET[name]


def ms_reference(O, code, og, y, rule, param, mode, t=None):
    """the bit-exact reference posteriors of a min-sum mode, under the target t[F, M] if given.  A forest's checks share no VN, so the order
    in which the horizontal-layered sweep takes them does not matter and the target goes to the oracle unpermuted
    (test_hlayered_check_order_does_not_matter_on_a_forest)"""
    sched, osched, okw = MS_MODES[mode][1], MS_MODES[mode][2], MS_MODES[mode][4]
    if sched == "vlayered":      # later VNs of a check see inputs rebuilt from posteriors: the schedule's own fp32 reference
        order, ptr, _ = code.vlayer_order()
        with np.errstate(over="ignore"):      # FLT_MAX + FLT_MAX is inf on both sides
            return vlayered_ref.decode(og.export(), y, rule, param, 1, "vlayered", order=order, class_ptr=ptr, enable_syndrome=False, target=t)["post"]
    return O.decode(og, y, rule, param, 1, osched, False, 1, target=t, **okw)["post"]


def ms_compare(q, O, torch, codes, rule, param, mode, forests, freeze=False, vs=None, target=False):
    engine, sched, osched, kw, okw, mode_vs, rules, chunk = MS_MODES[mode]
    vs = vs or mode_vs
    n = 0
    for name in forests:
        if engine == "edges" and name == "C":
            continue      # check degree <= 64
        deg, y = ms_inputs(name)
        _, code, og = codes[name]
        t = ms_target(name) if target else None
        ref = ms_reference(O, code, og, y, rule, param, mode, t)
        for V in vs:
            extra = dict(kw)
            if freeze:
                extra["freeze_messages"] = True
            dec = decoder(q, code, chunk or len(y), rule, param, engine=engine, schedule=sched, frames_per_lane=V, **extra)
            post = run_llr(torch, dec, y, chunk, t, q)
            bad = np.ascontiguousarray(post).view(np.uint32) != np.ascontiguousarray(ref).view(np.uint32)
            if bad.any():
                f, v = np.argwhere(bad)[0]
                sl = [s for s in R.check_slices(deg) if s.start <= v < s.stop][0]
                c = [i for i, s in enumerate(R.check_slices(deg)) if s.start <= v < s.stop][0]
                raise AssertionError("%s %s forest %s V=%d freeze=%d target=%s: %d posteriors differ from the oracle, first at frame %d VN %d (check %d of degree %d): "
                                     "y = %r, oracle %r, device %r" % (rule, mode, name, V, freeze, "none" if t is None else int(t[f, c]), int(bad.sum()), f, v, c,
                                                                       sl.stop - sl.start, y[f, sl].tolist(), float(ref[f, v]), float(post[f, v])))
            n += 1
    return n


@pytest.mark.parametrize("rule,param,mode", MS_CASES)
def test_min_sum_family_bit_equal_to_oracle(q, O, torch, codes, rule, param, mode):
    """MS / OMS / NMS / AMS_MIN on forests A, B, C with +-0.0, fp32 denormals and FLT_MAX among the inputs (domain: finite inputs): the
    posteriors of one check update equal the oracle's bit for bit -- fp32 on every schedule and both engines, binary16 storage on flooding with
    1 / 2 / 4 frames per lane, 8-bit messages on flooding and horizontal layered (against the oracle's integer decoder)."""
    assert ms_compare(q, O, torch, codes, rule, param, mode, ("A", "B", "C")) > 0


@pytest.mark.parametrize("mode", ["frames-flooding", "frames-hlayered", "frames-vlayered", "f16-flooding"])
@pytest.mark.parametrize("rule,param", R.MS_RULES)
def test_min_sum_family_bit_equal_with_freeze_messages(q, O, torch, codes, rule, param, mode):
    """freeze_messages on: the host takes the layered sweeps off the compressed check state and hands the kernels the freeze flag; no frame is
    frozen in a run without the syndrome test, so the answer is the one above"""
    assert ms_compare(q, O, torch, codes, rule, param, mode, ("A", "B"), freeze=True, vs=(1, 2)) > 0


@pytest.mark.parametrize("cst,rec", [("1", "1"), ("0", "1"), ("1", "0"), ("0", "0")])
@pytest.mark.parametrize("rule,param", R.MS_RULES)
def test_min_sum_family_layered_state_forms(q, O, torch, codes, monkeypatch, rule, param, cst, rec):
    """forest A on the horizontal-layered sweep with the compressed check state on and off (QLDPC_LAYER_CST) and with layer records on and off
    (QLDPC_LAYER_REC): four forms of the same sweep, one answer"""
    monkeypatch.setenv("QLDPC_LAYER_CST", cst)
    monkeypatch.setenv("QLDPC_LAYER_REC", rec)
    assert ms_compare(q, O, torch, codes, rule, param, "frames-hlayered", ("A",)) > 0


def test_hlayered_check_order_does_not_matter_on_a_forest(q, O, codes):
    """what lets ms_reference() hand the oracle the target unpermuted: the oracle on the graph in the sweep's check order with the permuted
    target gives the posteriors of the oracle on the graph as built, bit for bit (forest W, float and 8-bit messages)"""
    deg, y = ms_inputs("W")
    _, code, og = codes["W"]
    t = ms_target("W")
    order, _, _ = code.layer_order()
    var, chk = og.edges()
    inv = np.empty(code.M, np.int32)
    inv[order] = np.arange(code.M, dtype=np.int32)
    newc = inv[chk]
    idx = np.argsort(newc, kind="stable")
    og2 = O.Graph.from_edges(code.N, code.M, var[idx], newc[idx])
    for okw in ({}, {"msg_i8": True, "quant_scale": 8.0}):
        for rule, param in (("NMS", 0.75), ("OMS", 0.35)):
            a = O.decode(og, y, rule, param, 1, "hlayered", False, 1, target=t, **okw)["post"]
            b = O.decode(og2, y, rule, param, 1, "hlayered", False, 1, target=t[:, order], **okw)["post"]
            assert bits_equal(a, b)
    assert t.any(axis=0).all() and not t.all(axis=0).any()


@pytest.mark.parametrize("rule,param,mode", MS_CASES)
def test_min_sum_family_under_a_target(q, O, torch, codes, rule, param, mode):
    """MS / OMS / NMS / AMS_MIN with a target bit per (frame, check) on forests A, B, C and W (70 checks, three target words): posteriors
    bit-equal to the oracle's coset mode (tests/vlayered_ref.py for the vertical-layered sweep) -- fp32 on three schedules, the edge engine,
    binary16 storage at 1 / 2 / 4 frames per lane (2: the packed check pass, target bits at 15 and 31 of a dword), 8-bit messages on both of
    their schedules"""
    assert ms_compare(q, O, torch, codes, rule, param, mode, ("A", "B", "C", "W"), target=True) > 0


@pytest.mark.parametrize("mode", ["frames-flooding", "frames-hlayered", "frames-vlayered", "f16-flooding"])
@pytest.mark.parametrize("rule,param", R.MS_RULES)
def test_min_sum_family_under_a_target_with_freeze_messages(q, O, torch, codes, rule, param, mode):
    assert ms_compare(q, O, torch, codes, rule, param, mode, ("A", "W"), freeze=True, vs=(1, 2), target=True) > 0


@pytest.mark.parametrize("cst,rec", [("1", "1"), ("0", "1"), ("1", "0"), ("0", "0")])
@pytest.mark.parametrize("rule,param", R.MS_RULES)
def test_min_sum_family_layered_state_forms_under_a_target(q, O, torch, codes, monkeypatch, rule, param, cst, rec):
    """the four forms of the horizontal-layered sweep (compressed check state, layer records) each start the sign product from the target"""
    monkeypatch.setenv("QLDPC_LAYER_CST", cst)
    monkeypatch.setenv("QLDPC_LAYER_REC", rec)
    assert ms_compare(q, O, torch, codes, rule, param, "frames-hlayered", ("A",), target=True) > 0


# ---------------------------------------------------------------- coded LLR form ----------

CODED_MODES = {
    "frames-flooding": ("frames", "flooding", {}, VS, None),
    "f16-flooding": ("frames", "flooding", {"msg_dtype": "f16"}, VS, None),
    "frames-hlayered": ("frames", "hlayered", {}, (1,), None),
    "frames-vlayered": ("frames", "vlayered", {}, (1,), None),
    "edges-flooding": ("edges", "flooding", {}, (0,), 8),
}


CODED_CASES = [(r, p, m) for r, p in R.MS_RULES + R.SOFT_RULES for m in CODED_MODES if m != "edges-flooding" or r in ("MS", "OMS", "NMS", "SPA")]


def coded_compare(q, torch, codes, rule, param, mode, forests, target=False):
    engine, sched, kw, vs, chunk = CODED_MODES[mode]
    n = 0
    for i, name in enumerate(R.FORESTS):
        if name not in forests or (engine == "edges" and name == "C"):
            continue
        deg = R.FORESTS[name]
        y, bits, mag, cls, erase = R.qkd_frames(deg, seed=200 + i)
        assert bits_equal(y, R.input_sets()[name + "-coded"][1])
        t = R.target_cached(name + "-coded") if target else None
        code = codes[name][1]
        for V in vs:
            step = chunk or len(y)
            dec = decoder(q, code, step, rule, param, engine=engine, schedule=sched, frames_per_lane=V, **kw)
            want = run_llr(torch, dec, y, chunk, t, q)
            got = np.empty_like(want)
            for lo in range(0, len(y), step):
                dec.load_bits(torch.from_numpy(q.pack_bits(bits[lo:lo + step]).view(np.int32)).cuda(), torch.from_numpy(mag[lo:lo + step]).cuda(),
                              torch.from_numpy(cls).cuda())
                dec.load_erasures(torch.from_numpy(q.pack_bits(erase[lo:lo + step]).view(np.int32)).cuda())
                if target:
                    dec.load_syndrome(words(q, torch, t[lo:lo + step]))
                dec.run()
                got[lo:lo + step] = dec.fetch_post().cpu().numpy()
            assert bits_equal(got, want), "%s %s forest %s V=%d target=%d: %d posteriors differ between the coded form and the LLR array" % (
                rule, mode, name, V, target, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
            if target:      # ... and the target was not lost on both sides: it moves the posteriors
                assert not bits_equal(got, run_llr(torch, dec, y, chunk))
            n += 1
    return n


@pytest.mark.parametrize("rule,param,mode", CODED_CASES)
def test_coded_llr_form_bit_equal_to_llr_array(q, torch, codes, rule, param, mode):
    """The QKD mix through load_bits + load_erasures -- the class map (channel / pinned / punctured), a magnitude per frame, erasure rows --
    against load_llr of the same floats: bit-equal posteriors for every rule (the CODED kernels are separate instantiations; binary16
    storage with every rule, the soft ones included)."""
    assert ("SPA", 0.0, "f16-flooding") in CODED_CASES and ("AMS_MINSTAR_L2", 0.0, "f16-flooding") in CODED_CASES
    assert coded_compare(q, torch, codes, rule, param, mode, tuple(R.FORESTS)) > 0


@pytest.mark.parametrize("rule,param,mode", CODED_CASES)
def test_coded_llr_form_under_a_target(q, torch, codes, rule, param, mode):
    """the same with load_syndrome on both sides, forests A and W: the CODED instantiations start the sign product from the target too"""
    assert coded_compare(q, torch, codes, rule, param, mode, ("A", "W"), target=True) > 0


# ---------------------------------------------------------------- check degrees of 128 and more ----------

@pytest.mark.parametrize("sched", ["flooding", "hlayered", "vlayered"])
def test_spa_refused_from_check_degree_128(q, codes, sched):
    """The SPA fold keeps prod (1 + e_j) <= 2^dc in fp32: from degree 128 on it overflows (130 inputs of |x| = 0.01 give inf, then NaN, then
    the clamp: +-16.6 where the message is 1e-297).  Such a code is refused with the remedy named, not decoded wrongly."""
    deg, code, _ = codes["high"]
    with pytest.raises(q.QldpcError) as e:
        decoder(q, code, 8, "SPA", 0.0, schedule=sched, engine="frames")
    assert e.value.status == EUNSUPPORTED
    assert "LSPA" in str(e.value) and "128" in str(e.value)
    with pytest.raises(q.QldpcError) as e:
        decoder(q, code, 8, "SPA", 0.0, schedule=sched)
    assert e.value.status == EUNSUPPORTED
    decoder(q, codes["C"][1], 8, "SPA", 0.0, schedule=sched, engine="frames")      # degree 127 is served


@pytest.mark.parametrize("sched", ["flooding", "hlayered", "vlayered"])
@pytest.mark.parametrize("rule,param", [r for r in R.SOFT_RULES if r[0] != "SPA"])
def test_rules_without_a_product_serve_check_degrees_128_to_200(q, torch, codes, rule, param, sched):
    """LSPA (the remedy the refusal names) and the AMS rules on checks of degree 128, 129, 130 and 200: |x| = 0.01 throughout and the
    log-uniform family, within the same caps"""
    deg, y = R.input_sets()["high"]
    M = R.messages_cached(rule, param, "high", deg, y, sched)
    skip = np.broadcast_to(~R.first_swept(deg, codes["high"][1].vlayer_order()[0])[None, :], y.shape) if sched == "vlayered" else None
    worst = 0.0
    for V in VS:
        post = run_llr(torch, decoder(q, codes["high"][1], len(y), rule, param, schedule=sched, frames_per_lane=V, engine="frames"), y)
        worst = max(worst, R.worst_k(rule, deg, y, M, post, skip)[0])
    print("gpu %-14s frames-%-9s degrees 128..200 worst K = %.3f (cap %.3f)" % (rule, sched, worst, R.K_MAX[rule]))
    assert worst <= R.K_MAX[rule]


# ---------------------------------------------------------------- flags and hard words under a target ----------

HARD_WORD_SETS = ("A-hard", "B-hard")      # tests/test_check_rules_host.py: at most 1 % of their elements have a hard decision the tolerance leaves open
FLAG_SETS = HARD_WORD_SETS + ("W-hard",)


@pytest.mark.parametrize("sched", ["flooding", "hlayered"])
@pytest.mark.parametrize("rule,param", R.MS_RULES + R.SOFT_RULES)
def test_flags_and_hard_words_under_a_target(q, O, torch, codes, rule, param, sched):
    """With a target loaded, 1 / 2 / 4 frames per lane: fetch_status says ok exactly where the syndrome of the device's own hard word is the
    target (computed in numpy from fetch_packed, nothing left out), and the hard word is !(ref >= 0) of the reference posterior -- the
    oracle's for the min-sum family (forests A, B and W, every element), the restatement's for the soft rules, where the elements within
    tol(K_MAX) of a sign change are left out (check_rules_ref.hard_ref; forests A and B, at most 1 % of the elements).  Frames whose target is
    consistent with sign(y) come out ok, frame 1 (all ones) mostly does not."""
    soft = (rule, param) in R.SOFT_RULES
    mode = "frames-" + sched
    frame1, n_runs = 0, 0
    for name in FLAG_SETS:
        deg, y = R.get_set(name)
        t = R.target_cached(name)
        if soft:
            want, skip = R.hard_ref(rule, deg, y, R.messages_cached(rule, param, name, deg, y, sched, t))
            if name not in HARD_WORD_SETS:
                want = None
            else:
                assert skip.mean() <= 0.01
        else:
            _, code, og = codes[name.split("-")[0]]
            want, skip = (~(ms_reference(O, code, og, y, rule, param, mode, t) >= 0)).astype(np.uint8), np.zeros(y.shape, bool)
        code = codes[name.split("-")[0]][1]
        consistent = (np.arange(len(y)) % 4 == 2) & ~(y == 0).any(axis=1)
        assert consistent.sum() >= 10
        for V in VS:
            dec = decoder(q, code, len(y), rule, param, engine="frames", schedule=sched, frames_per_lane=V)
            run_llr(torch, dec, y, None, t, q)
            hard = q.unpack_bits(dec.fetch_packed().cpu().numpy().view(np.uint32), code.N)
            ok = dec.fetch_status()[1].cpu().numpy()
            assert set(np.unique(ok)) == {0, 1}, "%s %s set %s V=%d: flags %r" % (rule, mode, name, V, np.unique(ok))
            mine = R.syndrome_matches(deg, hard, t)
            assert ((ok == 1) == mine).all(), "%s %s set %s V=%d: the flag of frames %r is not what the syndrome of the device's own hard word says" % (
                rule, mode, name, V, np.flatnonzero((ok == 1) != mine)[:8].tolist())
            assert (ok[consistent] == 1).all(), "%s %s set %s V=%d: consistent frames %r are not ok" % (rule, mode, name, V, np.flatnonzero(consistent & (ok != 1))[:8].tolist())
            if want is not None:
                bad = (hard != want) & ~skip
                if bad.any():
                    f, v = np.argwhere(bad)[0]
                    raise AssertionError("%s %s set %s V=%d: %d hard decisions differ from the reference, first at frame %d VN %d: y = %r, device posterior %r"
                                         % (rule, mode, name, V, int(bad.sum()), f, v, float(y[f, v]), float(dec.fetch_post().cpu().numpy()[f, v])))
            frame1 += int(ok[1])
            n_runs += 1
    assert 2 * frame1 < n_runs, "frame 1, whose target is all ones, comes out ok in %d of %d runs" % (frame1, n_runs)


# ---------------------------------------------------------------- soft rules with binary16 message storage ----------

F16_STATS = {}


def f16_check(q, torch, codes, rule, param, name, target=False):
    """every posterior of the f16-flooding mode on one input set passes accept_f16; returns (elements, sharp elements, elements matched only
    inside a wider interval)"""
    engine, sched, kw, vs, _, _ = SOFT_MODES["f16-flooding"]
    deg, y = R.input_sets()[name]
    code = codes[name.split("-")[0]][1]
    x16, M, lo, hi = R.f16_interval_cached(rule, param, name, target)
    t = R.target_cached(name) if target else None
    sharp = lo == hi
    for V in vs:
        dec = decoder(q, code, len(y), rule, param, engine=engine, schedule=sched, frames_per_lane=V, **kw)
        post = run_llr(torch, dec, y, None, t, q)
        ok = R.accept_f16(y, post, lo, hi) & (np.isinf(post) == np.isinf(lo))      # +-inf exactly where the restatement's message is beyond binary16
        if not ok.all():
            for f, v in np.argwhere(~ok)[:8]:
                print("gpu f16 %-14s set %-8s V=%d target=%d frame %d VN %d: y = %r, x16 = %r, M = %r, lo16 = %r, hi16 = %r, device %r"
                      % (rule, name, V, target, f, v, float(y[f, v]), float(x16[f, v]), float(M[f, v]), float(lo[f, v]), float(hi[f, v]), float(post[f, v])))
        assert ok.all(), "%s f16-flooding set %s V=%d target=%d: %d of %d posteriors fail accept_f16" % (rule, name, V, target, int((~ok).sum()), ok.size)
        if target:
            assert bits_equal(post[0], run_llr(torch, dec, y, None)[0])
    return ok.size, int(sharp.sum()), int((~sharp).sum())


@pytest.mark.parametrize("rule,param", R.SOFT_RULES)
def test_soft_rules_with_binary16_storage(q, torch, codes, rule, param):
    """msg_dtype = "f16" with a soft rule (the __half instantiations of the soft check bodies, the __half VN passes, qk_first_v2c to binary16):
    every posterior is y plus a binary16 number inside [lo16, hi16] of the restatement on the rounded inputs (check_rules_ref.accept_f16) --
    bit-exact where lo16 == hi16 -- on forests A, B, C, the coded sets, inputs of 1e-8 .. 1e-6 (after the rounding every one of them is 0 or
    >= 2^-24, inside SPA's domain too) and, for the rules without a product, degrees 128 .. 200.  A check of degree 1 sends FLT_MAX under
    the AMS rules, which binary16 stores as inf: the posterior is +-inf there and nowhere else."""
    n = s = w = 0
    for name in SOFT_MODES["f16-flooding"][4]:
        if name == "high" and rule == "SPA":
            with pytest.raises(q.QldpcError) as e:      # refused as with fp32 messages (test_spa_refused_from_check_degree_128)
                decoder(q, codes["high"][1], 8, "SPA", 0.0, engine="frames", schedule="flooding", msg_dtype="f16")
            assert e.value.status == EUNSUPPORTED and "LSPA" in str(e.value)
            continue
        a, b, c = f16_check(q, torch, codes, rule, param, name)
        n, s, w = n + a, s + b, w + c
    print("gpu f16 %-14s %d elements: %.3f compared bit-exactly (lo16 == hi16), %d matched inside a wider interval" % (rule, n, s / n, w))


@pytest.mark.parametrize("rule,param", R.SOFT_RULES)
def test_soft_rules_with_binary16_storage_under_a_target(q, torch, codes, rule, param):
    """the soft __half bodies with a target bit, forests A and W"""
    for name in TARGET_SETS["f16-flooding"]:
        f16_check(q, torch, codes, rule, param, name, target=True)


@pytest.mark.parametrize("sched", ["hlayered", "vlayered"])
def test_binary16_storage_refused_off_the_flooding_schedule(q, codes, sched):
    with pytest.raises(q.QldpcError) as e:
        decoder(q, codes["A"][1], 8, "LSPA", 0.0, engine="frames", schedule=sched, msg_dtype="f16")
    assert e.value.status == EUNSUPPORTED
    assert ("fp16 message storage is implemented for the flooding schedule" in str(e.value)) or ("vertical-layered schedule runs on the FRAMES engine with fp32 messages" in str(e.value))
