"""Active-frame compaction on the horizontal-layered schedule (qldpc_decoder_cfg.compact = 1, csrc/qldpc_kernels_compact.h) -- GPU parity (-m gpu).

The layered decoder with the per-sweep syndrome exit keeps a converged frame in its lane until the slowest frame of its group is done;
with compact="on" the frames still running are dealt into fewer, full groups: the posteriors are gathered, the first sweep afterwards reads
the check's messages (or its compressed state) of the old generation through the slot map.  None of that may be visible to a caller: hard
decisions, iteration counts and success flags stay those of the oracle given H in the layer order (and of the uncompacted decoder), in the
caller's frame order, for explicit messages and the compressed check state, every frames-per-lane value, LLR and bit loads, the syndrome
form, syndrome_depth > 1 and per-frame erasures.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def layer_graph(O, code, og):
    """the oracle's graph with the checks in the code's layer order (the order the GPU sweeps them in), and that order"""
    order, _, _ = code.layer_order()
    var, chk = og.edges()
    inv = np.empty(code.M, np.int32)
    inv[order] = np.arange(code.M, dtype=np.int32)
    newc = inv[chk]
    idx = np.argsort(newc, kind="stable")
    return O.Graph.from_edges(code.N, code.M, var[idx], newc[idx]), order


@pytest.fixture(scope="module")
def peg(q, O, gold):
    p = os.path.join(gold, "PEGReg504x1008.alist")
    code = q.Code.from_alist(p)
    ogl, order = layer_graph(O, code, O.Graph.from_alist(p))
    return code, ogl, order


def i32(a):
    return np.ascontiguousarray(a).view(np.int32)


def frames(rng, F, N, lo=0.03, hi=0.075):
    """per-frame crossover probabilities spread over the waterfall, so the sweep counts are spread too (and some frames fail)"""
    p = rng.uniform(lo, hi, F)
    y = (rng.random((F, N)) < p[:, None]).astype(np.uint8)
    return y, p


def run(q, torch, dec, llr=None, bits=None, mag=None, cls=None, synd=None, erase=None):
    if llr is not None:
        dec.load_llr(torch.from_numpy(llr).cuda())
    else:
        dec.load_bits(torch.from_numpy(i32(q.pack_bits(bits))).cuda(), torch.from_numpy(mag).cuda(), None if cls is None else torch.from_numpy(cls).cuda())
    if erase is not None:
        dec.load_erasures(torch.from_numpy(i32(q.pack_bits(erase))).cuda())
    if synd is not None:
        dec.load_syndrome(torch.from_numpy(i32(q.pack_bits(synd))).cuda())
    dec.run()
    hard = q.unpack_bits(dec.fetch_packed().cpu().numpy().view(np.uint32), dec.N)
    it, ok = dec.fetch_status()
    return hard, it.cpu().numpy(), ok.cpu().numpy()


def same_as(ref, hard, it, ok):
    return bool((hard == ref["hard"]).all() and (it == ref["iters"]).all() and (ok == ref["synd_ok"]).all())


def layered(q, code, n_ite, F, **kw):
    kw.setdefault("rule", "NMS")
    kw.setdefault("rule_param", 0.75)
    return q.Decoder(code, code.N, n_ite, n_frames=F, schedule="hlayered", **kw)


# ---- 1. parity against the oracle and against compact="off" ------------------------------------------------------------------------

@pytest.mark.parametrize("V", [1, 2, 4])      # 1: compressed check state (qk_cn_layer_cst), 2 / 4: explicit messages (qk_cn_layer)
@pytest.mark.parametrize("form", ["llr", "bits"])
def test_compacted_layered_run_equals_oracle_and_uncompacted_run(q, O, torch, peg, V, form):
    code, ogl, _ = peg
    rng = np.random.default_rng(40 + V)
    F, N, n_ite = 1100, 1008, 30
    y, p = frames(rng, F, N)
    mag = np.full(F, 2.6, np.float32)
    llr = np.where(y == 1, -mag[:, None], mag[:, None]).astype(np.float32)
    ref = O.decode(ogl, llr, "NMS", 0.75, n_ite, "hlayered", True, 1, n_threads=8)
    assert len(np.unique(ref["iters"])) >= 6 and 0 < (ref["synd_ok"] == 0).sum() < F // 2      # a spread of sweep counts, both outcomes
    kw = dict(llr=llr) if form == "llr" else dict(bits=y, mag=mag)
    out = {}
    for mode in ("off", "on"):
        dec = layered(q, code, n_ite, F, frames_per_lane=V, compact=mode)
        hard, it, ok = run(q, torch, dec, **kw)
        st = dec.last_run_stats()
        print("V=%d %s compact=%s: %s, device bytes %d" % (V, form, mode, st, dec.device_bytes))
        assert (hard == ref["hard"]).all(), mode
        assert (it == ref["iters"]).all(), mode
        assert (ok == ref["synd_ok"]).all(), mode
        out[mode] = st
        if mode == "on":
            assert st["compactions"] >= (1 if V == 4 else 2), st
            with pytest.raises(q.QldpcError) as e:
                dec.fetch_post()
            assert e.value.status == -7
            # the decoder is reusable: the same batch again (no reload), then a smaller one
            dec.run()
            assert (q.unpack_bits(dec.fetch_packed().cpu().numpy().view(np.uint32), N) == ref["hard"]).all()
            it1, ok1 = dec.fetch_status()
            assert (it1.cpu().numpy() == ref["iters"]).all() and (ok1.cpu().numpy() == ref["synd_ok"]).all()
            h2, it2, ok2 = run(q, torch, dec, **({"llr": llr[:333]} if form == "llr" else {"bits": y[:333], "mag": mag[:333]}))
            assert (h2 == ref["hard"][:333]).all() and (it2 == ref["iters"][:333]).all() and (ok2 == ref["synd_ok"][:333]).all()
    # compaction is what it is for: fewer lane-sweeps for the same frames
    assert out["on"]["lane_iterations"] < out["off"]["lane_iterations"], out
    assert out["off"]["compactions"] == 0


# ---- 2. the rules on explicit messages, 64-frame groups ----------------------------------------------------------------------------

@pytest.mark.parametrize("rule,param,cst", [("SPA", 0.0, None), ("AMS_MIN", 0.0, "0"), ("AMS_MIN", 0.0, None), ("NMS", 0.75, "0"), ("OMS", 0.3, "0")])
def test_rules_at_one_frame_per_lane(q, O, torch, peg, monkeypatch, rule, param, cst):
    """frames are independent lanes: moving one to another lane changes nothing in its arithmetic, so "on" equals "off" bit for bit for
    every rule.  QLDPC_LAYER_CST=0 keeps the explicit messages for the min-sum / AMS rules, which otherwise run on the compressed state."""
    code, ogl, _ = peg
    if cst is not None:
        monkeypatch.setenv("QLDPC_LAYER_CST", cst)
    rng = np.random.default_rng(41)
    F, N, n_ite = 1100, 1008, 30
    y, _ = frames(rng, F, N)
    llr = np.where(y == 1, -2.6, 2.6).astype(np.float32)
    ref = O.decode(ogl, llr, rule, param, n_ite, "hlayered", True, 1, n_threads=8)
    assert len(np.unique(ref["iters"])) >= 6 and 0 < (ref["synd_ok"] == 0).sum() < F // 2
    res = {}
    for mode in ("off", "on"):
        dec = layered(q, code, n_ite, F, rule=rule, rule_param=param, frames_per_lane=1, compact=mode)
        res[mode] = run(q, torch, dec, llr=llr) + (dec.last_run_stats(),)
    assert res["off"][3]["compactions"] == 0 and res["on"][3]["compactions"] >= 2, (res["off"][3], res["on"][3])
    for a, b in zip(res["off"][:3], res["on"][:3]):
        assert (a == b).all()
    hard, it, ok, _ = res["on"]
    if rule != "SPA":
        assert same_as(ref, hard, it, ok)
    else:
        # the tolerance tests/test_parity_gpu.py states for the transcendental rules (device exp / log differ from glibc's in the last ulp): of the
        # frames the oracle converges on >= 99 % get the identical word, and the FER lies within 3 binomial sigma of the oracle's
        conv_ref = ref["synd_ok"] == 1
        same = (hard == ref["hard"]).all(axis=1)
        assert same[conv_ref].mean() >= 0.99, same[conv_ref].mean()
        fer_ref, fer_gpu = 1.0 - conv_ref.mean(), 1.0 - (ok == 1).mean()
        sigma = max(np.sqrt(fer_ref * (1 - fer_ref) / F), 1.0 / F)
        assert abs(fer_gpu - fer_ref) <= 3 * sigma, (fer_gpu, fer_ref, sigma)


# ---- 3. the other forms -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("V", [1, 2])
def test_syndrome_form_targets_move_with_their_frames(q, O, torch, peg, V):
    """random cosets: every frame has its own target syndrome (the oracle takes it in the layer order), re-dealt with the frame"""
    code, ogl, order = peg
    rng = np.random.default_rng(60 + V)
    F, N, n_ite = 900, 1008, 30
    e, _ = frames(rng, F, N)
    x = rng.integers(0, 2, (F, N)).astype(np.uint8)
    y = x ^ e
    og = O.Graph.from_alist(os.path.join(os.path.dirname(__file__), "golden", "PEGReg504x1008.alist"))
    s = np.stack([og.syndrome(xx)[1] for xx in x])
    mag = np.full(F, 2.6, np.float32)
    llr = np.where(y == 1, -2.6, 2.6).astype(np.float32)
    ref = O.decode(ogl, llr, "NMS", 0.75, n_ite, "hlayered", True, 1, n_threads=8, target=s[:, order])
    assert len(np.unique(ref["iters"])) >= 6 and 0 < (ref["synd_ok"] == 0).sum() < F // 2
    for mode in ("off", "on"):
        dec = layered(q, code, n_ite, F, frames_per_lane=V, compact=mode)
        hard, it, ok = run(q, torch, dec, bits=y, mag=mag, synd=s)
        assert same_as(ref, hard, it, ok), mode
        assert (dec.last_run_stats()["compactions"] >= 2) == (mode == "on")


@pytest.mark.parametrize("V", [1, 4])
def test_syndrome_depth_counters_move_with_their_frames(q, O, torch, peg, V):
    """syndrome_depth = 2: a frame dealt into another group between its first and its second zero syndrome takes its count along"""
    code, ogl, _ = peg
    rng = np.random.default_rng(52)
    F, N = 700, 1008
    y, _ = frames(rng, F, N)
    llr = np.where(y == 1, -2.6, 2.6).astype(np.float32)
    ref = O.decode(ogl, llr, "NMS", 0.75, 30, "hlayered", True, 2, n_threads=8)
    assert len(np.unique(ref["iters"])) >= 6
    dec = layered(q, code, 30, F, syndrome_depth=2, frames_per_lane=V, compact="on")
    hard, it, ok = run(q, torch, dec, llr=llr)
    assert dec.last_run_stats()["compactions"] >= 1
    assert same_as(ref, hard, it, ok)


@pytest.mark.parametrize("V", [1, 2])
def test_per_frame_erasures(q, O, torch, peg, V):
    """per-frame erasures are written into the channel rows at load time; a layered run never reads those again, so they stay where they are"""
    code, ogl, _ = peg
    rng = np.random.default_rng(70 + V)
    F, N, n_ite = 800, 1008, 30
    y, _ = frames(rng, F, N, 0.02, 0.06)
    erase = (rng.random((F, N)) < rng.uniform(0.0, 0.06, (F, 1))).astype(np.uint8)
    mag = np.full(F, 2.6, np.float32)
    llr = np.where(y == 1, -2.6, 2.6).astype(np.float32)
    llr[erase == 1] = 0.0
    ref = O.decode(ogl, llr, "NMS", 0.75, n_ite, "hlayered", True, 1, n_threads=8)
    assert len(np.unique(ref["iters"])) >= 6
    for mode in ("off", "on"):
        dec = layered(q, code, n_ite, F, frames_per_lane=V, compact=mode)
        hard, it, ok = run(q, torch, dec, bits=y, mag=mag, erase=erase)
        assert same_as(ref, hard, it, ok), mode
        assert (dec.last_run_stats()["compactions"] >= 1) == (mode == "on")


def test_fetch_info_and_decode_siho_after_compaction(q, O, torch, peg):
    """decode_siho's output (one int per information bit at info_bits_pos) is gathered from every generation"""
    code, ogl, _ = peg
    rng = np.random.default_rng(77)
    F, N = 500, 1008
    y, _ = frames(rng, F, N)
    llr = np.where(y == 1, -2.6, 2.6).astype(np.float32)
    pos = np.arange(504, 1008)[::-1].copy()
    ref = O.decode(ogl, llr, "OMS", 0.3, 25, "hlayered", True, 1, n_threads=8)
    assert len(np.unique(ref["iters"])) >= 6
    dec = q.Decoder(code, 504, 25, info_bits_pos=pos, rule="OMS", rule_param=0.3, n_frames=F, schedule="hlayered", compact="on")
    V = dec.decode_siho(llr)
    assert dec.last_run_stats()["compactions"] >= 1
    assert (V == ref["hard"][:, pos]).all()
    assert (dec.fetch_info().cpu().numpy() == ref["hard"][:, pos]).all()


# ---- 4. what must not compact -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw", [dict(compact="auto"), dict(compact="on", freeze_messages=True), dict(compact="on", enable_syndrome=False),
                                dict(compact="on", layer_chain="on"), dict(compact="on", msg_dtype="i8")],
                         ids=["auto", "freeze", "fixed", "chain", "i8"])
def test_cases_that_do_not_compact(q, O, torch, peg, kw):
    code, ogl, _ = peg
    rng = np.random.default_rng(90)
    F, N, n_ite = 1100, 1008, 12
    y, _ = frames(rng, F, N)
    llr = np.where(y == 1, -2.6, 2.6).astype(np.float32)
    synd = kw.get("enable_syndrome", True)
    ref = O.decode(ogl, llr, "NMS", 0.75, n_ite, "hlayered", synd, 1, n_threads=8, msg_i8=(kw.get("msg_dtype") == "i8"))
    dec = layered(q, code, n_ite, F, **kw)
    hard, it, ok = run(q, torch, dec, llr=llr)
    assert dec.last_run_stats()["compactions"] == 0
    assert same_as(ref, hard, it, ok)
    if kw.get("msg_dtype") != "i8":
        dec.fetch_post()      # not refused: nothing moved


def test_vertical_layered_keeps_refusing(q, peg):
    code, _, _ = peg
    with pytest.raises(q.QldpcError) as e:
        q.Decoder(code, 1008, 8, rule="NMS", rule_param=0.75, n_frames=600, schedule="vlayered", compact="on")
    assert e.value.status == -7


# ---- 5. a session-shaped batch on the headline code ----------------------------------------------------------------------------------

def test_mixed_qber_batch_on_the_headline_code(q, O, torch):
    """every block of a reconciliation batch has its own QBER and the gaps sit close to the threshold: 512 frames of the headline code with
    per-frame QBER U[2 %, 3 %], parity VNs pinned.  Uncompacted, the useful share of the lane-sweeps of such a batch is about 0.37."""
    code = q.Code.ira(65536, 52429, 0.125, 11, 3, 7)
    enc = q.Encoder(code, "IRA")
    K, N = enc.K, code.N
    var, chk = code.edges()
    ogl, _ = layer_graph(O, code, O.Graph.from_edges(N, code.M, var, chk))
    rng = np.random.default_rng(2)
    F, n_ite = 512, 50
    qber = rng.uniform(0.02, 0.03, F)
    cw = enc.encode(rng.integers(0, 2, (F, K)).astype(np.uint8))
    noisy = cw.copy()
    noisy[:, :K] ^= rng.random((F, K)) < qber[:, None]
    mag = np.array([q.bsc_llr(float(p)) for p in qber], np.float32)
    llr = np.where(noisy == 1, -mag[:, None], mag[:, None]).astype(np.float32)
    llr[:, K:] = np.where(cw[:, K:] == 1, -np.float32(q.CONFIRMED_BIT_LLR), np.float32(q.CONFIRMED_BIT_LLR))
    ref = O.decode(ogl, llr, "NMS", 0.75, n_ite, "hlayered", True, 1, n_threads=min(16, os.cpu_count() or 8))
    its = ref["iters"]
    groups = its.reshape(-1, 64)
    print("oracle: sweeps %d..%d, mean %.2f, %d failures, useful lane-sweeps uncompacted %.3f"
          % (its.min(), its.max(), its.mean(), int((ref["synd_ok"] == 0).sum()), its.sum() / (64.0 * groups.max(axis=1).sum())))
    assert len(np.unique(its)) >= 6 and (ref["synd_ok"] == 1).sum() > F // 2      # a spread of sweep counts, most frames converge
    st = {}
    for mode in ("off", "on"):
        dec = q.Decoder(code, N, n_ite, rule="NMS", rule_param=0.75, n_frames=F, schedule="hlayered", compact=mode)
        hard, it, ok = run(q, torch, dec, llr=llr)
        st[mode] = dec.last_run_stats()
        print("compact=%s: %s, useful %.3f" % (mode, st[mode], its.sum() / max(1, st[mode]["lane_iterations"])))
        assert same_as(ref, hard, it, ok), mode
    assert st["off"]["compactions"] == 0 and st["on"]["compactions"] >= 1, st
    assert st["on"]["lane_iterations"] < st["off"]["lane_iterations"], st
