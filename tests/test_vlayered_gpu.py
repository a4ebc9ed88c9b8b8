"""GPU suite (-m gpu): the vertical-layered schedule (QLDPC_SCHED_VLAYERED, csrc/qldpc_kernels_vl.h) through the C ABI.

Bar: MS / OMS / NMS / AMS<min> fp32 -- identical hard decisions, iteration counts, success flags and (with freeze_messages) posteriors
bit for bit on every frame, against tests/vlayered_ref.py.  That reference is a restatement of Decoder_LDPC_BP_vertical_layered in the
terms of the oracle's horizontal decoder (parity UNPINNED against AFF3CT: its source is not in the reference tree); its shared fold and
bookkeeping are pinned to the CPU oracle in tests/test_vlayered_host.py.  SPA / LSPA / min*: the tolerance the project states for these
rules (test_transcendental_rules_tolerance): of the frames the reference converges on, >= 99 % identical words.
"""
import json
import os

import numpy as np
import pytest

import vlayered_ref as R
from mc_oracle import ROOT, sim_rows

pytestmark = pytest.mark.gpu

EXACT = [("MS", 0.0), ("OMS", 0.35), ("NMS", 0.75), ("AMS_MIN", 0.0)]
SOFT = [("SPA", 0.0), ("LSPA", 0.0), ("AMS_MINSTAR", 0.0), ("AMS_MINSTAR_L2", 0.0)]


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def kat(gold):
    return json.load(open(os.path.join(gold, "kat_peg504x1008.json")))


@pytest.fixture(scope="module")
def peg(q, O, gold):
    """(code, oracle graph, its export, the code's vlayer order and class bounds): the order is the natural level schedule here, i.e. the
    reference worked through class by class is the sequential v = 0..N-1 sweep (test_vlayered_host.py checks both statements)"""
    p = os.path.join(gold, "PEGReg504x1008.alist")
    code, og = q.Code.from_alist(p), O.Graph.from_alist(p)
    order, ptr, natural = code.vlayer_order()
    assert natural
    return code, og, og.export(), order, ptr


def bsc_frames(rng, F, N, p, mag):
    return np.where(rng.random((F, N)) < p, -mag, mag).astype(np.float32)


def i32(words):
    return words.astype(np.int64).astype(np.uint32).view(np.int32)


def fetch(q, dec, want_post=True):
    hard = q.unpack_bits(dec.fetch_packed().cpu().numpy().view(np.uint32), dec.N)
    it, ok = dec.fetch_status()
    post = dec.fetch_post().cpu().numpy() if want_post else None
    return hard, it.cpu().numpy(), ok.cpu().numpy(), post


def staged(q, torch, dec, llr, want_post=True):
    dec.load_llr(torch.from_numpy(llr).cuda())
    dec.run()
    return fetch(q, dec, want_post)


def same_as(ref, hard, it, ok, post=None):
    assert (hard == ref["hard"]).all()
    assert (it == ref["iters"]).all()
    assert (ok == ref["synd_ok"]).all()
    if post is not None:
        assert (post.view(np.uint32) == ref["post"].view(np.uint32)).all()     # bit-exact floats


@pytest.mark.parametrize("rule,param", EXACT)
@pytest.mark.parametrize("V", [1, 2, 4])
def test_vlayered_minsum_family_bit_exact(q, torch, peg, rule, param, V):
    code, _, ex, order, ptr = peg
    F = 300                                                     # ragged: not a multiple of 64*V
    llr = bsc_frames(np.random.default_rng(10 + V), F, 1008, 0.065 if rule in ("NMS", "OMS") else 0.045, 2.6)
    ref = R.decode(ex, llr, rule, param, 25, "vlayered", order=order, class_ptr=ptr)
    dec = q.Decoder(code, 1008, 25, rule=rule, rule_param=param, n_frames=F, schedule="vlayered", frames_per_lane=V, freeze_messages=True)
    same_as(ref, *staged(q, torch, dec, llr))
    fails = int((ref["synd_ok"] == 0).sum())
    print("vlayered %s V=%d: %d of %d frames fail in the reference, mean iterations %.2f" % (rule, V, fails, F, ref["iters"].mean()))
    if rule in ("NMS", "OMS"):
        assert 0 < fails < F                                    # both outcomes are exercised


def test_vlayered_natural_order_qc_code(q, O, torch, gold):
    """NR_1_7_30.qc: 27 levels in natural order; messages not frozen -- words, iterations and flags are exact"""
    p = os.path.join(gold, "NR_1_7_30.qc")
    code, og = q.Code.from_qc(p), O.Graph.from_qc(p)
    order, ptr, natural = code.vlayer_order()
    assert natural and code.n_vlayers == 27
    F = 100
    llr = bsc_frames(np.random.default_rng(31), F, code.N, 0.12, 2.0)
    ref = R.decode(og.export(), llr, "NMS", 0.75, 10, "vlayered", order=order, class_ptr=ptr)
    dec = q.Decoder(code, code.N, 10, rule="NMS", rule_param=0.75, n_frames=F, schedule="vlayered")
    same_as(ref, *staged(q, torch, dec, llr, want_post=False))
    assert (ref["synd_ok"] == 1).any() and ref["iters"].max() > ref["iters"].min()


@pytest.mark.parametrize("rule,param,V", [("NMS", 0.75, 1), ("AMS_MIN", 0.0, 2)])
def test_vlayered_coloured_order_ira_code(q, O, torch, rule, param, V):
    """an IRA code has no level parallelism on the VN side: the sweep runs in the exported coloured order, and so does the reference"""
    code = q.Code.ira(4096, 3277)
    var, chk = code.edges()
    og = O.Graph.from_edges(code.N, code.M, var, chk)
    order, ptr, natural = code.vlayer_order()
    assert not natural
    F = 130
    llr = bsc_frames(np.random.default_rng(32), F, code.N, 0.012, 4.4)
    ref = R.decode(og.export(), llr, rule, param, 10, "vlayered", order=order, class_ptr=ptr)
    dec = q.Decoder(code, code.N, 10, rule=rule, rule_param=param, n_frames=F, schedule="vlayered", frames_per_lane=V)
    same_as(ref, *staged(q, torch, dec, llr, want_post=False))
    assert (ref["synd_ok"] == 1).any()


def test_vlayered_fixed_iterations_no_syndrome(q, torch, peg):
    code, _, ex, order, ptr = peg
    llr = bsc_frames(np.random.default_rng(5), 130, 1008, 0.06, 2.75)
    ref = R.decode(ex, llr, "OMS", 0.35, 12, "vlayered", order=order, class_ptr=ptr, enable_syndrome=False)
    dec = q.Decoder(code, 1008, 12, rule="OMS", rule_param=0.35, n_frames=130, schedule="vlayered", enable_syndrome=False)
    hard, it, ok, post = staged(q, torch, dec, llr)
    assert (it == 12).all() and dec.last_run_iterations == 12
    same_as(ref, hard, it, ok, post)


def test_vlayered_syndrome_depth(q, torch, peg):
    code, _, ex, order, ptr = peg
    llr = bsc_frames(np.random.default_rng(6), 64, 1008, 0.05, 2.9)
    ref = R.decode(ex, llr, "NMS", 0.75, 30, "vlayered", order=order, class_ptr=ptr, syndrome_depth=2)
    one = R.decode(ex, llr, "NMS", 0.75, 30, "vlayered", order=order, class_ptr=ptr)
    assert (ref["iters"] != one["iters"]).any()                 # the depth is seen
    dec = q.Decoder(code, 1008, 30, rule="NMS", rule_param=0.75, n_frames=64, schedule="vlayered", syndrome_depth=2, freeze_messages=True)
    same_as(ref, *staged(q, torch, dec, llr))


def test_vlayered_syndrome_form(q, torch, peg):
    """coset decoding: the fold of check c starts at sign (-1)^s_c (as orc_decode_coset), the stop test and the flag are H x = s"""
    code, og, ex, order, ptr = peg
    rng = np.random.default_rng(151)
    F = 150
    x = rng.integers(0, 2, (F, 1008)).astype(np.uint8)
    s = np.stack([og.syndrome(xx)[1] for xx in x])
    y = x ^ (rng.random((F, 1008)) < 0.045)
    mag = np.float32(q.bsc_llr(0.045))
    llr = np.where(y == 1, -mag, mag).astype(np.float32)
    ref = R.decode(ex, llr, "NMS", 0.75, 30, "vlayered", order=order, class_ptr=ptr, target=s)
    dec = q.Decoder(code, 1008, 30, rule="NMS", rule_param=0.75, n_frames=F, schedule="vlayered", frames_per_lane=2, freeze_messages=True)
    dec.load_bits(torch.from_numpy(i32(q.pack_bits(y))).cuda(), torch.full((F,), float(mag), device="cuda"))
    dec.load_syndrome(torch.from_numpy(i32(q.pack_bits(s))).cuda())
    dec.run()
    hard, it, ok, post = fetch(q, dec)
    same_as(ref, hard, it, ok, post)
    good = ok == 1
    assert good.mean() > 0.8 and (hard[good] == x[good]).all()      # Bob ends with Alice's key


def test_vlayered_frame_formation_and_per_frame_erasures(q, O, torch):
    """qldpc_load_bits_* (channel bits, pinned and punctured classes) and qldpc_load_erasures_dev in front of the vertical sweep: what the
    reference gives on the LLRs those calls stand for"""
    rng = np.random.default_rng(21)
    code = q.Code.ira(2048, 1536, 0.2, 8, 3, 11)
    var, chk = code.edges()
    og = O.Graph.from_edges(code.N, code.M, var, chk)
    order, ptr, _ = code.vlayer_order()
    N, K, F = code.N, 1536, 130
    enc = q.Encoder(code, "IRA")
    info = rng.integers(0, 2, (F, K)).astype(np.uint8)
    cw = q.unpack_bits(enc.encode_packed(torch.from_numpy(q.pack_bits(info).view(np.int32)).cuda()).cpu().numpy().view(np.uint32), N)
    qber = rng.uniform(0.005, 0.03, F).astype(np.float32)
    y = cw.copy()
    y[:, :K] ^= (rng.random((F, K)) < qber[:, None]).astype(np.uint8)
    mag = np.array([q.bsc_llr(float(p)) for p in qber], np.float32)
    cls = np.zeros(N, np.uint8)
    cls[K:] = q.VN_PINNED
    cls[K:K + 30] = q.VN_PUNCTURED
    erase = np.zeros((F, N), np.uint8)
    for f in range(F):                                            # a different number of evenly spaced punctured parity VNs per frame
        p = int(rng.integers(0, 150))
        j = np.arange(N - K, dtype=np.int64)
        erase[f, K:] = ((j + 1) * p // (N - K) > j * p // (N - K))
    llr = np.where(y == 1, -mag[:, None], mag[:, None]).astype(np.float32)
    llr[:, K:] = np.where(cw[:, K:] == 1, -np.float32(q.CONFIRMED_BIT_LLR), np.float32(q.CONFIRMED_BIT_LLR))
    llr[:, K:K + 30] = 0.0
    plain = R.decode(og.export(), llr, "NMS", 0.75, 20, "vlayered", order=order, class_ptr=ptr)
    dec = q.Decoder(code, N, 20, rule="NMS", rule_param=0.75, n_frames=F, schedule="vlayered", freeze_messages=True)
    bits = torch.from_numpy(q.pack_bits(y).view(np.int32)).cuda()
    dec.load_bits(bits, torch.from_numpy(mag).cuda(), torch.from_numpy(cls).cuda())
    dec.run()
    same_as(plain, *fetch(q, dec))
    llr[erase == 1] = 0.0
    erased = R.decode(og.export(), llr, "NMS", 0.75, 20, "vlayered", order=order, class_ptr=ptr)
    dec.load_bits(bits, torch.from_numpy(mag).cuda(), torch.from_numpy(cls).cuda())
    dec.load_erasures(torch.from_numpy(q.pack_bits(erase).view(np.int32)).cuda())
    dec.run()
    same_as(erased, *fetch(q, dec))
    assert (erased["synd_ok"] == 1).mean() > 0.5 and (erased["post"] != plain["post"]).any()


@pytest.mark.parametrize("rule,param", SOFT)
def test_vlayered_transcendental_rules_tolerance(q, torch, peg, rule, param):
    code, _, ex, order, ptr = peg
    F = 256
    llr = bsc_frames(np.random.default_rng(7), F, 1008, 0.07, 2.59)
    ref = R.decode(ex, llr, rule, param, 20, "vlayered", order=order, class_ptr=ptr)
    dec = q.Decoder(code, 1008, 20, rule=rule, rule_param=param, n_frames=F, schedule="vlayered", freeze_messages=True)
    hard, it, ok, _ = staged(q, torch, dec, llr, want_post=False)
    same = (hard == ref["hard"]).all(axis=1)
    conv_ref = ref["synd_ok"] == 1
    print("vlayered %s: reference converges on %d of %d, identical words on %.4f of those, GPU converges on %d" % (rule, conv_ref.sum(), F, same[conv_ref].mean(), (ok == 1).sum()))
    assert conv_ref.sum() > F // 2
    assert same[conv_ref].mean() >= 0.99, same[conv_ref].mean()


def test_vlayered_kat_through_decode_siho(q, peg, kat):
    code = peg[0]
    dec = q.Decoder(code, 504, 10, info_bits_pos=np.arange(504, 1008), rule="SPA", n_frames=1, schedule="vlayered")
    V = dec.decode_siho(np.array(kat["llrs"], np.float32))
    assert (V[0] == np.array(kat["decoded"])).all()
    it, ok = dec.fetch_status()
    assert ok.item() == 1 and 0 < it.item() < 10                 # the reference takes 4 sweeps
    dec.reset()
    V2 = dec.decode_siho(np.array(kat["llrs"], np.float32))     # reset() -> same answer again
    assert (V2 == V).all()


def test_vlayered_profile_stats(q, torch, peg):
    code, _, ex, _, _ = peg
    F, ite = 128, 6
    dec = q.Decoder(code, 1008, ite, rule="NMS", rule_param=0.75, n_frames=F, schedule="vlayered", enable_syndrome=False)
    dec.profile(True)
    staged(q, torch, dec, bsc_frames(np.random.default_rng(2), F, 1008, 0.05, 2.9), want_post=False)
    st = {s["name"]: s for s in dec.profile_read()}
    assert "vn_vlayer" in st and "layer_update" not in st and st["vn_vlayer"]["launches"] == ite
    dc = np.diff(ex["cn_ptr"]).astype(np.int64)
    rows = 2 * int((dc ** 2).sum()) + 2 * code.N                 # read 2 sum dc^2 - E + N, written E + N
    assert st["vn_vlayer"]["moved_bytes"] == pytest.approx(rows * 4.0 * F * ite)
    assert st["vn_vlayer"]["alg_bytes"] == pytest.approx(4.0 * code.E * 4.0 * F * ite)


@pytest.mark.parametrize("kw", [dict(engine="edges"), dict(msg_dtype="f16"), dict(msg_dtype="i8"), dict(layer_chain="on"), dict(compact="on")])
def test_vlayered_refused_combinations(q, O, torch, peg, kw):
    code, og, _, _, _ = peg
    with pytest.raises(q.QldpcError) as e:
        q.Decoder(code, 1008, 10, rule="NMS", rule_param=0.75, n_frames=8, schedule="vlayered", **kw)
    assert e.value.status == -7 and "vertical-layered" in str(e.value)
    with pytest.raises(q.QldpcError) as e:
        q.Recon(max_blocks=16, schedule="vlayered")
    assert e.value.status == -1 and "recon_create" in str(e.value)
    # nothing shared was disturbed: a horizontal and a flooding decoder created afterwards on the same code still match the oracle
    llr = bsc_frames(np.random.default_rng(9), 70, 1008, 0.06, 2.6)
    order, _, nat = code.layer_order()
    assert nat                                                   # natural layer order: the oracle's c = 0..M-1 sweep
    for sched in ("hlayered", "flooding"):
        ref = O.decode(og, llr, "NMS", 0.75, 20, sched, True, 1, n_threads=8)
        dec = q.Decoder(code, 1008, 20, rule="NMS", rule_param=0.75, n_frames=70, schedule=sched, freeze_messages=True)
        same_as(ref, *staged(q, torch, dec, llr))


def test_c_harness_vertical_layered_runs():
    """host/qldpc_sim -v on the arguments of test_alist_layered_minsum_runs, with that test's own bound (the numpy reference gives 0
    failures in 2 000 such frames, mean 2.0 iterations, so the bound hides nothing)"""
    rows, text = sim_rows(["-a", os.path.join(ROOT, "tests", "golden", "PEGReg504x1008.alist"), "-r", "NMS", "-p", "0.75", "-v", "-i", "20", "-f", "200", "-b", "100",
                           "-s", "0.02:0.02:0.01"], timeout=600)
    assert len(rows) == 1 and int(rows[0][1]) == 200 and int(rows[0][3]) <= 2
    assert "vertical_layered" in text and "Info. bits (K) = 504" in text
