"""Single-VN tests of the variable-node update on the device: every kernel body that sums a VN's messages, on stars (one centre VN of degree d,
d checks of degree 2, d leaves) where every posterior shows one VN update and nothing else, and on a fan (an IRA code with information VNs of
degree 0 .. 13 and 16) for the posterior form of the flooding run.  References: tests/vn_rules_ref.py -- the star formulas, flood() -- and the CPU
oracle where the restatement does not reach (binary16 and 8-bit messages, two layered sweeps); tests/test_vn_rules_host.py holds the restatement
to the oracle and the inputs to their sensitivity conditions.  Every comparison is on bit patterns.

Every decoder runs without the syndrome test and with compaction off.  The body each test runs is listed in DESIGN.md section 4, "Variable-node
updates, one VN at a time".
"""
import numpy as np
import pytest

import blind_ref
import vlayered_ref
import vn_rules_ref as R

pytestmark = pytest.mark.gpu

EUNSUPPORTED = -7
VS = (1, 2, 4)
EDGE_RULES = [r for r in R.MS_RULES if r[0] != "AMS_MIN"]      # the edge engine and the 8-bit form run MS / OMS / NMS
EDGE_LOAD = 8
PINNED_LLR = 23.025850929840455


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


class StarCode:
    def __init__(self, q, O, profile):
        self.st = R.stars(list(profile), list(profile.values()))
        st = self.st
        self.code = q.Code.from_edges(st.N, st.M, st.var, st.chk)
        self.og = O.Graph.from_edges(st.N, st.M, st.var, st.chk)
        self.ex = self.og.export()
        st.bind(self.ex)
        self.ogl, self.layer_order = blind_ref.layered_graph(O, self.code, self.og)      # the oracle's graph with the checks in the device's sweep order
        self._y = {}

    def frames(self, families, rule, param):
        key = (families, rule)
        if key not in self._y:
            y, fam = R.frames(self.st, families, seed=11, rule=rule, param=param)
            y.setflags(write=False)
            self._y[key] = (y, fam)
        return self._y[key]


@pytest.fixture(scope="module")
def sets(q, O):
    return {"A": StarCode(q, O, R.SET_A), "edge": StarCode(q, O, R.SET_EDGE), "33": StarCode(q, O, R.SET_33), "256": StarCode(q, O, R.SET_256),
            "257": StarCode(q, O, R.SET_257)}


def decoder(q, code, F, rule, param, n_ite, **kw):
    return q.Decoder(code, code.N, n_ite, rule=rule, rule_param=param, n_frames=F, enable_syndrome=False, compact="off", **kw)


def run_llr(torch, dec, y, chunk=None):
    """load_llr -> run -> fetch_post, `chunk` frames at a time"""
    y = np.array(y, np.float32)
    chunk = chunk or len(y)
    post = np.empty(y.shape, np.float32)
    for lo in range(0, len(y), chunk):
        dec.load_llr(torch.from_numpy(y[lo:lo + chunk]).cuda())
        dec.run()
        post[lo:lo + chunk] = dec.fetch_post().cpu().numpy()
    return post


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_on_stars(sc, y, got, ref, what):
    """bit-equal posteriors, or a message that names the star degree and the first differing frame and VN with its inputs"""
    bad = bits(got) != bits(ref)
    if not bad.any():
        return
    f, v = (int(x) for x in np.argwhere(bad)[0])
    d, cen, leaves = sc.st.members(v)
    raise AssertionError("%s: %d posteriors differ, first at frame %d VN %d (%s of a star of degree %d): reference %r, device %r; Y_centre = %r, Y_leaves in slot order = %r"
                         % (what, int(bad.sum()), f, v, "centre" if v == cen else "leaf, slot %d" % int(np.nonzero(leaves == v)[0][0]), d,
                            float(ref[f, v]), float(got[f, v]), float(y[f, cen]), y[f, leaves].tolist()))


# ---------------------------------------------------------------- a1: frames engine, flooding, fp32 ----------

@pytest.mark.parametrize("n_ite", [1, 2])
@pytest.mark.parametrize("rule,param", R.MS_RULES)
def test_flooding_fp32_equals_the_restatement(q, torch, sets, rule, param, n_ite):
    """qk_vn_flood<POST> (n_ite = 1) and qk_vn_flood<NORMAL> (n_ite = 2), caps 4, 12 and the generic body, 1 / 2 / 4 frames per lane"""
    sc = sets["A"]
    y, _ = sc.frames(R.FLOOD_FAMILIES, rule, param)
    ref = R.star_flooding(sc.st, y, rule, param, n_ite)
    for V in VS:
        dec = decoder(q, sc.code, len(y), rule, param, n_ite, engine="frames", frames_per_lane=V)
        assert not dec.flood_post
        same_on_stars(sc, y, run_llr(torch, dec, y), ref, "%s frames-flooding n_ite=%d V=%d" % (rule, n_ite, V))


# ---------------------------------------------------------------- a2: edge engine ----------

@pytest.mark.parametrize("n_ite", [1, 2])
@pytest.mark.parametrize("rule,param", EDGE_RULES)
def test_edge_engine_equals_the_restatement(q, torch, sets, rule, param, n_ite):
    """the edge engine's VN pass (each lane sums its VN's slots in order), the degrees of set A up to its limit of 32 and that limit, 8 frames per load"""
    sc = sets["edge"]
    y, _ = sc.frames(R.FLOOD_FAMILIES, rule, param)
    ref = R.star_flooding(sc.st, y, rule, param, n_ite)
    dec = decoder(q, sc.code, EDGE_LOAD, rule, param, n_ite, engine="edges")
    same_on_stars(sc, y, run_llr(torch, dec, y, EDGE_LOAD), ref, "%s edges-flooding n_ite=%d" % (rule, n_ite))


@pytest.mark.parametrize("name,dv", [("33", 33), ("A", 65)])
def test_edge_engine_refuses_vn_degrees_above_32(q, sets, name, dv):
    """512 VNs x max_dv messages have to fit 64 KiB of LDS: degree 33 is the first excess, and the refusal names the limit (it said 64 once, and
    refused 33 and 64 under that wording)"""
    assert sets["edge"].code.max_vn_degree == R.EDGE_MAX_DV and sets[name].code.max_vn_degree == dv
    with pytest.raises(q.QldpcError) as e:
        decoder(q, sets[name].code, EDGE_LOAD, "NMS", 0.75, 2, engine="edges")
    assert e.value.status == EUNSUPPORTED
    assert "edge-parallel engine needs flooding, MS/OMS/NMS/SPA, check degree <= 64 (have 2) and VN degree <= 32 (have %d)" % dv in str(e.value)
    assert decoder(q, sets[name].code, EDGE_LOAD, "NMS", 0.75, 2, engine="auto").flood_post is False      # auto: served by the frames engine


# ---------------------------------------------------------------- a3: binary16 messages ----------

@pytest.mark.parametrize("n_ite", [1, 2])
@pytest.mark.parametrize("rule,param", R.MS_RULES)
def test_flooding_f16_equals_the_oracle(q, O, torch, sets, rule, param, n_ite):
    """the binary16 instantiations of qk_vn_flood: fp32 sum of the widened messages, the extrinsic outputs rounded to binary16"""
    sc = sets["A"]
    y, _ = sc.frames(R.FLOOD_FAMILIES, rule, param)
    ref = O.decode(sc.og, y, rule, param, n_ite, "flooding", False, 1, msg_fp16=True)["post"]
    for V in VS:
        dec = decoder(q, sc.code, len(y), rule, param, n_ite, engine="frames", frames_per_lane=V, msg_dtype="f16")
        same_on_stars(sc, y, run_llr(torch, dec, y), ref, "%s f16-flooding n_ite=%d V=%d" % (rule, n_ite, V))


# ---------------------------------------------------------------- a4: 8-bit messages ----------

def i8_inputs(sc, rule, param):
    return np.concatenate([sc.frames(R.FLOOD_FAMILIES, rule, param)[0], R.saturated_frames(sc.st)])


@pytest.mark.parametrize("sched", ["flooding", "hlayered"])
@pytest.mark.parametrize("rule,param", EDGE_RULES)
def test_i8_equals_the_oracle(q, O, torch, sets, rule, param, sched):
    """qi_vn_flood (a 16-bit posterior) and the 8-bit layered sweep against the oracle's integer decoder at scale 8: set A with the general
    families and with every input at +-127 / scale, and the degree-256 star with every input saturated -- both signs, alternating signs, the
    centre against its leaves: 127 + 256 x 127 = 32 639 is the last sum a 16-bit posterior holds"""
    for name in ("A", "256"):
        sc = sets[name]
        y = i8_inputs(sc, rule, param) if name == "A" else R.saturated_frames(sc.st)
        for n_ite in (1, 2):
            ref = O.decode(sc.og if sched == "flooding" else sc.ogl, y, rule, param, n_ite, sched, False, 1, msg_i8=True, quant_scale=R.I8_SCALE)["post"]
            if name == "256" and sched == "flooding" and n_ite == 1 and rule == "MS":
                assert ref[0, sc.st.centre[0]] == 32639.0 and ref[1, sc.st.centre[0]] == -32639.0
            dec = decoder(q, sc.code, len(y), rule, param, n_ite, schedule=sched, msg_dtype="i8", quant_scale=R.I8_SCALE)
            same_on_stars(sc, y, run_llr(torch, dec, y), ref, "%s i8-%s set %s n_ite=%d" % (rule, sched, name, n_ite))


@pytest.mark.parametrize("sched", ["flooding", "hlayered"])
def test_i8_refuses_vn_degree_257(q, sets, sched):
    with pytest.raises(q.QldpcError) as e:
        decoder(q, sets["257"].code, 8, "NMS", 0.75, 2, schedule=sched, msg_dtype="i8", quant_scale=R.I8_SCALE)
    assert e.value.status == EUNSUPPORTED
    assert "256" in str(e.value) and "257" in str(e.value)


# ---------------------------------------------------------------- a5: horizontal layered ----------

def hlayered_compare(q, O, torch, sc, rule, param, what, vs, **kw):
    y, _ = sc.frames(R.LAYER_FAMILIES, rule, param)
    refs = {1: R.star_hlayered(sc.st, y, rule, param, order=sc.layer_order),
            2: O.decode(sc.ogl, y, rule, param, 2, "hlayered", False, 1)["post"]}
    for n_ite, ref in refs.items():
        for V in vs:
            dec = decoder(q, sc.code, len(y), rule, param, n_ite, engine="frames", schedule="hlayered", frames_per_lane=V, **kw)
            same_on_stars(sc, y, run_llr(torch, dec, y), ref, "%s hlayered %s n_ite=%d V=%d" % (rule, what, n_ite, V))


@pytest.mark.parametrize("chain", ["on", "off"])
@pytest.mark.parametrize("rule,param", R.MS_RULES)
def test_hlayered_equals_the_restatement(q, O, torch, sets, rule, param, chain):
    """the centre's running posterior over its checks in sweep order, -0.0 inputs included (the sweep forms y - 0 and keeps the sign): one sweep
    against the restatement, two against the oracle; the one-launch sweep (V = 1) and the launch per layer (V = 1, 2, 4)"""
    hlayered_compare(q, O, torch, sets["A"], rule, param, "layer_chain=" + chain, (1,) if chain == "on" else VS, layer_chain=chain)


@pytest.mark.parametrize("cst,rec", [("1", "1"), ("0", "1"), ("1", "0"), ("0", "0")])
@pytest.mark.parametrize("rule,param", R.MS_RULES)
def test_hlayered_state_forms(q, O, torch, sets, monkeypatch, rule, param, cst, rec):
    """the compressed check state and the layer records on and off: four forms of one sweep, one answer"""
    monkeypatch.setenv("QLDPC_LAYER_CST", cst)
    monkeypatch.setenv("QLDPC_LAYER_REC", rec)
    hlayered_compare(q, O, torch, sets["A"], rule, param, "CST=%s REC=%s" % (cst, rec), (1,))


# ---------------------------------------------------------------- a6: vertical layered ----------

@pytest.mark.parametrize("rule,param", R.MS_RULES)
def test_vlayered_equals_its_reference(q, torch, sets, rule, param):
    """qk_vn_vlayer against tests/vlayered_ref.py in the code's class order, one and two sweeps"""
    sc = sets["A"]
    y, _ = sc.frames(R.LAYER_FAMILIES, rule, param)
    order, ptr, _ = sc.code.vlayer_order()
    for n_ite in (1, 2):
        ref = vlayered_ref.decode(sc.ex, y, rule, param, n_ite, "vlayered", order=order, class_ptr=ptr, enable_syndrome=False)["post"]
        for V in VS:
            dec = decoder(q, sc.code, len(y), rule, param, n_ite, engine="frames", schedule="vlayered", frames_per_lane=V)
            same_on_stars(sc, y, run_llr(torch, dec, y), ref, "%s vlayered n_ite=%d V=%d" % (rule, n_ite, V))


# ---------------------------------------------------------------- a7: coded LLR form ----------

CODED_MODES = {
    "frames-flooding": ("A", {"engine": "frames"}, VS, None),
    "f16-flooding": ("A", {"engine": "frames", "msg_dtype": "f16"}, VS, None),
    "edges-flooding": ("edge", {"engine": "edges"}, (0,), EDGE_LOAD),
    "frames-hlayered": ("A", {"engine": "frames", "schedule": "hlayered"}, (1,), None),
    "frames-vlayered": ("A", {"engine": "frames", "schedule": "vlayered"}, (1,), None),
}
CODED_CASES = [(r, p, m) for r, p in R.MS_RULES for m in CODED_MODES if m != "edges-flooding" or r != "AMS_MIN"]


@pytest.mark.parametrize("rule,param,mode", CODED_CASES)
def test_coded_llr_form_equals_the_llr_array(q, torch, sets, rule, param, mode):
    """two iterations, so the CODED instantiations of qk_vn_flood<NORMAL> (fp32 and binary16) and of the other VN passes run: the QKD mix through
    load_bits + load_erasures (class map, a magnitude per frame, erasure rows) gives the bits of load_llr of the same floats, and on the fp32
    flooding engines those of the restatement"""
    name, kw, vs, chunk = CODED_MODES[mode]
    sc = sets[name]
    y, bts, mag, cls, erase = R.qkd_frames(sc.st.N, seed=21)
    step = chunk or len(y)
    for V in vs:
        dec = decoder(q, sc.code, step, rule, param, 2, frames_per_lane=V, **kw)
        want = run_llr(torch, dec, y, chunk)
        if mode in ("frames-flooding", "edges-flooding"):
            same_on_stars(sc, y, want, R.star_flooding(sc.st, y, rule, param, 2), "%s %s V=%d, LLR array" % (rule, mode, V))
        got = np.empty_like(want)
        for lo in range(0, len(y), step):
            dec.load_bits(torch.from_numpy(q.pack_bits(bts[lo:lo + step]).view(np.int32)).cuda(), torch.from_numpy(mag[lo:lo + step]).cuda(), torch.from_numpy(cls).cuda())
            dec.load_erasures(torch.from_numpy(q.pack_bits(erase[lo:lo + step]).view(np.int32)).cuda())
            dec.run()
            got[lo:lo + step] = dec.fetch_post().cpu().numpy()
        same_on_stars(sc, y, got, want, "%s %s V=%d, coded form against the LLR array" % (rule, mode, V))


# ---------------------------------------------------------------- a8: the two ballots ----------

@pytest.mark.parametrize("sched", ["flooding", "hlayered"])
@pytest.mark.parametrize("rule,param", R.MS_RULES)
def test_ballots(q, torch, sets, rule, param, sched):
    """hard = !(tmp >= 0) is what fetch_packed returns, sgn = signbit(tmp) is what the syndrome test reads: posteriors that cancel to exactly +0.0
    (both ballots 0) and, under the layered sweep, stars that stay at -0.0 (sgn 1, hard 0).  The success flag is the syndrome of the hard word;
    on a star a centre at -0.0 has every leaf at -0.0, so the syndrome of the sign bits is the same flag, and both are asserted.  Frames 0 and 1
    are made all positive and all -0.0 so that the flag is not 0 throughout"""
    sc = sets["A"]
    fams = R.FLOOD_FAMILIES if sched == "flooding" else R.LAYER_FAMILIES
    y, fam = sc.frames(fams, rule, param)
    y = np.array(y)
    y[0] = np.abs(y[0]) + np.float32(1.0)
    y[1] = np.float32(-0.0)
    ref = R.star_flooding(sc.st, y, rule, param, 1) if sched == "flooding" else R.star_hlayered(sc.st, y, rule, param, order=sc.layer_order)
    cancel = fam == fams.index("cancel")
    cancel[:2] = False
    assert (bits(ref[:, sc.st.centre][cancel]) == 0).all() or (sched == "hlayered" and rule == "OMS")
    if sched == "hlayered":
        assert (bits(ref[1]) == 0x80000000).all() and (bits(ref[:, sc.st.centre][2:][R.all_negzero(fam, fams)[2:]]) == 0x80000000).all()
    hard = (~(ref >= 0)).astype(np.uint8)
    ok_hard = R.vlayered_syndrome(sc.ex, hard)
    ok_sgn = R.vlayered_syndrome(sc.ex, np.signbit(ref))
    assert (ok_hard == ok_sgn).all() and ok_hard[0] == 1 and ok_hard[1] == 1 and 0 < ok_hard.sum() < len(y)
    for V in VS:
        dec = decoder(q, sc.code, len(y), rule, param, 1, engine="frames", schedule=sched, frames_per_lane=V)
        dec.load_llr(torch.from_numpy(y).cuda())
        dec.run()
        got = q.unpack_bits(dec.fetch_packed().cpu().numpy().view(np.uint32), sc.st.N)
        it, ok = dec.fetch_status()
        what = "%s %s V=%d" % (rule, sched, V)
        same_on_stars(sc, y, got.astype(np.float32), hard.astype(np.float32), what + ", hard words")
        assert (ok.cpu().numpy() == ok_sgn).all() and (it.cpu().numpy() == 1).all(), what
        same_on_stars(sc, y, dec.fetch_post().cpu().numpy(), ref, what)


# ---------------------------------------------------------------- b: the posterior form on the fan ----------

FAN_FRAMES = (3, 64, 130)
FAN_ITES = (1, 2, 3, 5)


@pytest.fixture(scope="module")
def the_fan(q, O):
    N, M, var, chk, deg = R.fan()
    code = q.Code.from_edges(N, M, var, chk)
    og = O.Graph.from_edges(N, M, var, chk)
    assert code.is_ira
    return code, og.export(), deg, R.general_frames(N, seed=77)


def knobs(monkeypatch, post, post_vn):
    for name, on in (("QLDPC_FLOOD_POST", post), ("QLDPC_FLOOD_POST_VN", post_vn)):
        if on:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, "0")


def results(dec):
    it, ok = dec.fetch_status()
    return dict(hard=dec.fetch_packed().cpu().numpy().view(np.uint32).copy(), iters=it.cpu().numpy(), ok=ok.cpu().numpy(), post=bits(dec.fetch_post().cpu().numpy()).copy())


def record_bytes(deg, F):
    """what the records of qk_vn_fpost add to the moved bytes of one in-between pass (tests/test_flood_post_vn_gpu.py): {v, row[0 .. D)} padded to
    16 bytes per VN of degree <= 12, read once per 64-frame group"""
    return sum(((int(d) + 1 + 3) // 4) * 16.0 for d in deg if d <= 12) * (F / 64.0)


def fan_same(q, got, ref, F, N, deg, y, what):
    bad = got["post"] != bits(ref["post"][:F])
    if bad.any():
        f, v = (int(x) for x in np.argwhere(bad)[0])
        raise AssertionError("%s: %d posteriors differ from flood(), first at frame %d VN %d (%s): reference %r, device %r, Y = %r"
                             % (what, int(bad.sum()), f, v, "information VN of degree %d" % deg[v] if v < len(deg) else "chain VN",
                                float(ref["post"][f, v]), float(got["post"][f, v].view(np.float32)), float(y[f, v])))
    assert (q.unpack_bits(got["hard"], N) == ref["hard"][:F]).all(), what
    assert (got["iters"] == ref["iters"][:F]).all() and (got["ok"] == ref["synd_ok"][:F]).all(), what


@pytest.mark.parametrize("rule,param", EDGE_RULES)
def test_posterior_form_on_the_fan(q, torch, the_fan, monkeypatch, rule, param):
    """qk_vn_fpost with a body per degree 0 .. 12 (13 degree classes: four launches), degrees 13 and 16 on qk_vn_flood<POST> inside the posterior form,
    the closing pass and qk_fpost_close, against flood(); the same with the in-between pass on qk_vn_flood (QLDPC_FLOOD_POST_VN=0) and on explicit
    messages (QLDPC_FLOOD_POST=0)"""
    code, ex, deg, y = the_fan
    for n_ite in FAN_ITES:
        ref = R.flood(ex, y, rule, param, n_ite)
        for F in FAN_FRAMES:
            out = []
            for post, post_vn, want_fp in ((True, True, True), (True, False, True), (False, True, False)):
                knobs(monkeypatch, post, post_vn)
                dec = decoder(q, code, F, rule, param, n_ite, engine="frames", frames_per_lane=1)
                assert dec.flood_post == want_fp
                dec.profile(True)
                dec.load_llr(torch.from_numpy(y[:F].copy()).cuda())
                dec.run()
                got = results(dec)
                fan_same(q, got, ref, F, code.N, deg, y, "%s n_ite=%d F=%d FLOOD_POST=%d FLOOD_POST_VN=%d" % (rule, n_ite, F, post, post_vn))
                out.append({s["name"]: s for s in dec.profile_read()})
            # a pass is one vn_update record whichever kernels run it: n_ite - 1 in between, the closing pair, the pair of fetch_post
            st, st1 = out[0], out[1]
            assert st["vn_update"]["launches"] == st1["vn_update"]["launches"] == n_ite + 1 + 2
            assert st["cn_update"]["launches"] == st1["cn_update"]["launches"] == n_ite
            extra = st["vn_update"]["moved_bytes"] - st1["vn_update"]["moved_bytes"]
            assert extra == pytest.approx((n_ite - 1) * record_bytes(deg, F), rel=1e-9, abs=1e-6), (n_ite, F)


def test_posterior_form_on_the_fan_from_bits(q, torch, the_fan, monkeypatch):
    """coded LLRs as the benchmark loads them -- received bits, a magnitude per frame, every parity VN pinned -- against the same run on the LLR
    array, against flood(), and with the in-between pass on qk_vn_flood"""
    code, ex, deg, _ = the_fan
    K, F, n_ite = len(deg), 130, 3
    rng = np.random.default_rng(17)
    bts = rng.integers(0, 2, (F, code.N)).astype(np.uint8)
    mag = rng.uniform(1.0, 4.0, F).astype(np.float32)
    cls = np.zeros(code.N, np.uint8)
    cls[K:] = q.VN_PINNED
    m = np.where(cls[None, :] == q.VN_PINNED, np.float32(PINNED_LLR), mag[:, None]).astype(np.float32)
    y = np.where(bts == 1, -m, m).astype(np.float32)
    ref = R.flood(ex, y, "NMS", 0.75, n_ite)
    for post_vn in (True, False):
        knobs(monkeypatch, True, post_vn)
        dec = decoder(q, code, F, "NMS", 0.75, n_ite, engine="frames", frames_per_lane=1)
        assert dec.flood_post
        dec.load_bits(torch.from_numpy(q.pack_bits(bts).view(np.int32)).cuda(), torch.from_numpy(mag).cuda(), torch.from_numpy(cls).cuda())
        dec.run()
        fan_same(q, results(dec), ref, F, code.N, deg, y, "NMS from bits, FLOOD_POST_VN=%d" % post_vn)
        dec.load_llr(torch.from_numpy(y).cuda())
        dec.run()
        fan_same(q, results(dec), ref, F, code.N, deg, y, "NMS from the LLR array, FLOOD_POST_VN=%d" % post_vn)
