"""GPU suite (-m gpu): the posterior form of the fixed-iteration flooding min-sum run (qldpc_kernels_fpost.h) against the CPU oracle and
against the same decoder on explicit messages (QLDPC_FLOOD_POST=0): hard words, iteration counts, success flags and posteriors as bit
patterns.  The oracle is computed once per (code, rule, iteration count) for the largest batch; smaller batches are its first frames."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PIN = np.float32(23.025850929840455)
RULES = [("MS", 0.0), ("OMS", 0.35), ("NMS", 0.75)]
CODES = {"r08": (4096, 3277), "r05": (2048, 1024)}      # check degree 17 / 18 (bucket 20) and 6 (bucket 8, state outside the var_to_chk allocation)
FRAMES = (3, 64, 130)                                  # partial group, full group, three groups
ITES = (1, 2, 5)                                       # first pass only; state read once; both parities of the ping-pong


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def codes(q, O):
    out = {}
    for name, (n, k) in CODES.items():
        c = q.Code.ira(n, k, 0.125, 11, 3, 7)
        var, chk = c.edges()
        out[name] = (c, O.Graph.from_edges(c.N, c.M, var, chk))
    return out


def i32(words):
    return words.astype(np.int64).astype(np.uint32).view(np.int32)


def results(dec, N):
    it, ok = dec.fetch_status()
    return dict(hard=dec.fetch_packed().cpu().numpy().view(np.uint32).copy(), iters=it.cpu().numpy(), ok=ok.cpu().numpy(),
                post=dec.fetch_post().cpu().numpy().view(np.uint32).copy())


def same(a, b):
    return all((a[k] == b[k]).all() for k in ("hard", "iters", "ok", "post"))


def against_oracle(q, got, ref, F, N):
    assert (q.unpack_bits(got["hard"], N) == ref["hard"][:F]).all()
    assert (got["iters"] == ref["iters"][:F]).all() and (got["ok"] == ref["synd_ok"][:F]).all()
    assert (got["post"] == ref["post"][:F].view(np.uint32)).all()


def llr_frames(rng, F, N):
    """real-valued LLRs with random signs; frame 1 all zero (every message +-0.0); frame 2 on a coarse grid (ties min1 == min2 in most checks)"""
    llr = (rng.normal(1.2, 1.5, (F, N)) * np.where(rng.random((F, N)) < 0.5, -1.0, 1.0)).astype(np.float32)
    llr[1] = 0.0
    llr[2] = np.round(llr[2] * 2.0) / 2.0
    return llr


def run_llr(q, torch, code, rule, param, n_ite, llr, synd=None, **kw):
    dec = q.Decoder(code, code.N, n_ite, rule=rule, rule_param=param, n_frames=llr.shape[0], engine="frames", enable_syndrome=kw.pop("enable_syndrome", False), **kw)
    dec.profile(True)
    dec.load_llr(torch.from_numpy(llr).cuda())
    if synd is not None:
        dec.load_syndrome(torch.from_numpy(i32(q.pack_bits(synd))).cuda())
    dec.run()
    return dec, results(dec, code.N)


@pytest.mark.parametrize("rule,param", RULES)
@pytest.mark.parametrize("name", list(CODES))
def test_llr_arrays_bit_exact(q, O, torch, codes, monkeypatch, name, rule, param):
    code, og = codes[name]
    llr = llr_frames(np.random.default_rng(5), max(FRAMES), code.N)
    for n_ite in ITES:
        ref = O.decode(og, llr, rule, param, n_ite, "flooding", False, 1, n_threads=8)
        for F in FRAMES:
            monkeypatch.delenv("QLDPC_FLOOD_POST", raising=False)
            dec, got = run_llr(q, torch, code, rule, param, n_ite, llr[:F])
            assert dec.flood_post and dec.last_run_iterations == n_ite
            against_oracle(q, got, ref, F, code.N)
            monkeypatch.setenv("QLDPC_FLOOD_POST", "0")
            dec0, got0 = run_llr(q, torch, code, rule, param, n_ite, llr[:F])
            assert not dec0.flood_post and same(got, got0), (n_ite, F)


def coded_case(q, rng, code, F):
    """load_bits frames: pinned and punctured VNs among the information AND the chain VNs (the rest of the chain are channel VNs), a shortening
    length per frame, per-frame erasures; returns what is loaded and the LLR array it stands for"""
    N, K = code.N, code.N - code.M
    cls = np.zeros(N, np.uint8)
    cls[rng.random(N) < 0.10] = 1                      # pinned
    cls[(rng.random(N) < 0.05) & (cls == 0)] = 2       # punctured
    assert (cls[K:] == 0).sum() > code.M // 2 and (cls[K:] == 1).any() and (cls[K:] == 2).any()
    bits = rng.integers(0, 2, (F, N)).astype(np.uint8)
    mag = rng.uniform(1.0, 4.0, F).astype(np.float32)
    nch = rng.integers(K // 2, N + 1, F).astype(np.int32)
    era = (rng.random((F, N)) < 0.02).astype(np.uint8)
    v = np.arange(N)[None, :]
    m = np.where(cls[None, :] == 0, np.where(v < nch[:, None], mag[:, None], PIN), np.where(cls[None, :] == 1, PIN, np.float32(0.0))).astype(np.float32)
    m[era == 1] = 0.0
    llr = np.where(bits == 1, -m, m).astype(np.float32)
    return dict(bits=bits, mag=mag, cls=cls, nch=nch, era=era, llr=llr)


def run_coded(q, torch, code, rule, param, n_ite, cs, F, synd=None):
    dec = q.Decoder(code, code.N, n_ite, rule=rule, rule_param=param, n_frames=F, engine="frames", enable_syndrome=False)
    dec.profile(True)
    dec.load_bits(torch.from_numpy(i32(q.pack_bits(cs["bits"][:F]))).cuda(), torch.from_numpy(cs["mag"][:F]).cuda(), torch.from_numpy(cs["cls"]).cuda(),
                  torch.from_numpy(cs["nch"][:F]).cuda())
    dec.load_erasures(torch.from_numpy(i32(q.pack_bits(cs["era"][:F]))).cuda())
    if synd is not None:
        dec.load_syndrome(torch.from_numpy(i32(q.pack_bits(synd[:F]))).cuda())
    dec.run()
    return dec, results(dec, code.N)


@pytest.mark.parametrize("rule,param", RULES)
@pytest.mark.parametrize("name", list(CODES))
def test_load_bits_with_pinned_shortened_erased_vns_bit_exact(q, O, torch, codes, monkeypatch, name, rule, param):
    code, og = codes[name]
    cs = coded_case(q, np.random.default_rng(9), code, max(FRAMES))
    for n_ite in ITES:
        ref = O.decode(og, cs["llr"], rule, param, n_ite, "flooding", False, 1, n_threads=8)
        for F in FRAMES:
            monkeypatch.delenv("QLDPC_FLOOD_POST", raising=False)
            dec, got = run_coded(q, torch, code, rule, param, n_ite, cs, F)
            assert dec.flood_post
            against_oracle(q, got, ref, F, code.N)
            monkeypatch.setenv("QLDPC_FLOOD_POST", "0")
            dec0, got0 = run_coded(q, torch, code, rule, param, n_ite, cs, F)
            assert not dec0.flood_post and same(got, got0), (n_ite, F)


@pytest.mark.parametrize("name", list(CODES))
def test_target_syndrome_bit_exact(q, O, torch, codes, monkeypatch, name):
    code, og = codes[name]
    rng = np.random.default_rng(13)
    F = max(FRAMES)
    x = rng.integers(0, 2, (F, code.N)).astype(np.uint8)
    s = np.stack([og.syndrome(xx)[1] for xx in x])
    assert s.any()
    cs = coded_case(q, rng, code, F)
    cs["bits"] = x ^ (rng.random((F, code.N)) < 0.03)
    llr_mag = np.abs(cs["llr"])
    cs["llr"] = np.where(cs["bits"] == 1, -llr_mag, llr_mag).astype(np.float32)
    llr = llr_frames(rng, F, code.N)
    monkeypatch.delenv("QLDPC_FLOOD_POST", raising=False)
    for n_ite in ITES:
        ref = O.decode(og, cs["llr"], "NMS", 0.75, n_ite, "flooding", False, 1, n_threads=8, target=s)
        ref_llr = O.decode(og, llr, "OMS", 0.35, n_ite, "flooding", False, 1, n_threads=8, target=s)
        for Fx in FRAMES:
            dec, got = run_coded(q, torch, code, "NMS", 0.75, n_ite, cs, Fx, synd=s)
            assert dec.flood_post
            against_oracle(q, got, ref, Fx, code.N)
            dec, got = run_llr(q, torch, code, "OMS", 0.35, n_ite, llr[:Fx], synd=s[:Fx])
            assert dec.flood_post
            against_oracle(q, got, ref_llr, Fx, code.N)


def stats(dec):
    return {s["name"]: s for s in dec.profile_read()}


def test_the_form_really_ran_and_moves_fewer_bytes(q, O, torch, codes, monkeypatch):
    """profile: a variable-node pass of the posterior form moves less than 0.7 of what a var_to_chk-writing pass is priced at (2 E + N rows);
    with the knob off the passes move what they always did"""
    code, og = codes["r08"]
    F, n_ite = 130, 5
    llr = llr_frames(np.random.default_rng(5), F, code.N)
    normal = (2.0 * code.E + code.N) * 4.0 * F
    monkeypatch.delenv("QLDPC_FLOOD_POST", raising=False)
    dec, _ = run_llr(q, torch, code, "NMS", 0.75, n_ite, llr)
    st = stats(dec)
    print("posterior form", {k: (v["launches"], v["alg_bytes"], v["moved_bytes"]) for k, v in st.items()})
    assert dec.flood_post
    # run: n_ite check passes, n_ite - 1 posterior passes + the closing pair; fetch_post: one more pair
    assert st["cn_update"]["launches"] == n_ite and st["vn_update"]["launches"] == n_ite + 1 + 2
    assert st["vn_update"]["moved_bytes"] / st["vn_update"]["launches"] < 0.7 * normal
    # a check pass is priced at 2 E rows and moves, per information edge, a posterior row in and a message row out, its own three state rows in and out
    # and the channel rows of its chain VNs (the first pass: channel rows of all VNs in, no state in) -- MORE than 2 E; the saving is the VN pass's
    Ei, M = code.E - (2 * code.M - 1), code.M
    assert st["cn_update"]["alg_bytes"] == n_ite * 2.0 * code.E * 4.0 * F
    assert st["cn_update"]["moved_bytes"] == ((Ei + 3 * M + code.N) + (n_ite - 1) * (2 * Ei + 6 * M + M)) * 4.0 * F
    assert set(st) <= {"cn_update", "vn_update", "syndrome", "status", "load", "fetch"}
    monkeypatch.setenv("QLDPC_FLOOD_POST", "0")
    dec0, _ = run_llr(q, torch, code, "NMS", 0.75, n_ite, llr)
    st0 = stats(dec0)
    assert not dec0.flood_post
    assert st0["cn_update"]["moved_bytes"] == st0["cn_update"]["alg_bytes"] == n_ite * 2.0 * code.E * 4.0 * F
    # FIRST + (n_ite - 1) NORMAL + POST, and the POST of fetch_post
    assert st0["vn_update"]["launches"] == n_ite + 2
    assert st0["vn_update"]["moved_bytes"] == st0["vn_update"]["alg_bytes"] == ((n_ite - 1) * normal + 3 * (code.E + code.N) * 4.0 * F)


def explicit_messages(st, E, F):
    """the check passes of the explicit-message form move what they are priced at: E rows read, E written"""
    return st["cn_update"]["moved_bytes"] == st["cn_update"]["alg_bytes"] == st["cn_update"]["launches"] * 2.0 * E * 4.0 * F


def test_ineligible_decoders_fall_back_and_stay_exact(q, O, torch, codes, gold, monkeypatch):
    monkeypatch.delenv("QLDPC_FLOOD_POST", raising=False)
    code, og = codes["r08"]
    F, n_ite = 130, 5
    llr = llr_frames(np.random.default_rng(5), F, code.N)
    # early exit: needs the ballots of every VN after every iteration
    ref = O.decode(og, llr, "NMS", 0.75, n_ite, "flooding", True, 1, n_threads=8)
    dec, got = run_llr(q, torch, code, "NMS", 0.75, n_ite, llr, enable_syndrome=True, freeze_messages=True)
    assert not dec.flood_post and explicit_messages(stats(dec), code.E, F)
    against_oracle(q, got, ref, F, code.N)
    # two frames per lane
    ref = O.decode(og, llr, "NMS", 0.75, n_ite, "flooding", False, 1, n_threads=8)
    dec, got = run_llr(q, torch, code, "NMS", 0.75, n_ite, llr, frames_per_lane=2)
    assert not dec.flood_post and explicit_messages(stats(dec), code.E, F)
    against_oracle(q, got, ref, F, code.N)
    # SPA is tolerance class here (hardware exp / log against libm: converged-word agreement, not bit patterns), so: BSC frames at a QBER the code
    # corrects in a few iterations, the words of every frame the oracle sees converge, and bit for bit the run with the knob off
    rng = np.random.default_rng(21)
    mag = np.float32(q.bsc_llr(0.01))
    bsc = np.where(rng.random((F, code.N)) < 0.01, -mag, mag).astype(np.float32)
    ref = O.decode(og, bsc, "SPA", 0.0, 8, "flooding", False, 1, n_threads=8)
    dec, got = run_llr(q, torch, code, "SPA", 0.0, 8, bsc)
    assert not dec.flood_post and explicit_messages(stats(dec), code.E, F)
    conv = ref["synd_ok"] == 1
    assert conv.mean() > 0.5 and (got["ok"][conv] == 1).all() and (q.unpack_bits(got["hard"], code.N)[conv] == ref["hard"][conv]).all()
    monkeypatch.setenv("QLDPC_FLOOD_POST", "0")
    dec0, got0 = run_llr(q, torch, code, "SPA", 0.0, 8, bsc)
    monkeypatch.delenv("QLDPC_FLOOD_POST", raising=False)
    assert not dec0.flood_post and same(got, got0)
    # a graph without the chain
    p = os.path.join(gold, "PEGReg504x1008.alist")
    peg, opeg = q.Code.from_alist(p), O.Graph.from_alist(p)
    llr = llr_frames(np.random.default_rng(6), F, peg.N)
    ref = O.decode(opeg, llr, "NMS", 0.75, n_ite, "flooding", False, 1, n_threads=8)
    dec, got = run_llr(q, torch, peg, "NMS", 0.75, n_ite, llr)
    assert not dec.flood_post and explicit_messages(stats(dec), peg.E, F)
    against_oracle(q, got, ref, F, peg.N)
