"""GPU suite (-m gpu): the check passes of the posterior form after their loads were reordered (qldpc_kernels_fpost.h: the first pass fetches a
check's channel words with lanes as edges, a steady pass asks for its chain VNs' words in front of the gathers, the closing pass likewise).
Hard words, iteration counts, success flags and posteriors of all N VNs as bit patterns, against the CPU oracle, against the same decoder on
explicit messages (QLDPC_FLOOD_POST=0) and against the posterior form with qk_vn_flood in between (QLDPC_FLOOD_POST_VN=0).

Coded loads (load_bits, the benchmark's path) carry what the reordered loads read: per-frame magnitudes, pinned parity, pinned and punctured
information VNs, a shortening length on some frames, and erasures on a few frames -- information VNs, a chain VN, the last chain VN (degree 1)
and one frame erased altogether (every message +-0.0, -0.0 where the received bit is set) -- once loaded and once not (no erasure array).
The oracle is computed once per (code, rule, iteration count) for the largest batch; smaller batches are its first frames."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PIN = np.float32(23.025850929840455)
RULES = [("MS", 0.0), ("OMS", 0.35), ("NMS", 0.75)]
# check degree 17 / 18 (bucket 20), 6 (bucket 8) and 24 / 25 (the QK_FP_DCMAX instance)
CODES = {"r08": (4096, 3277), "r05": (2048, 1024), "r085": (2048, 1741)}
FRAMES = (3, 64, 130)      # partial group, full group, a last group with 62 padding lanes
ITES = (1, 2, 3)           # the first pass followed directly by the closing passes; both parities of the state
KNOBS = ("QLDPC_FLOOD_POST", "QLDPC_FLOOD_POST_VN")


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


def test_the_high_degree_code_runs_the_widest_instance(codes):
    code, _ = codes["r085"]
    _, chk = code.edges()
    deg = np.bincount(chk, minlength=code.M)
    assert 21 <= deg.max() <= 27, deg.max()


def i32(words):
    return words.astype(np.int64).astype(np.uint32).view(np.int32)


def results(dec):
    it, ok = dec.fetch_status()
    return dict(hard=dec.fetch_packed().cpu().numpy().view(np.uint32).copy(), iters=it.cpu().numpy(), ok=ok.cpu().numpy(),
                post=dec.fetch_post().cpu().numpy().view(np.uint32).copy())


def same(a, b):
    return all((a[k] == b[k]).all() for k in ("hard", "iters", "ok", "post"))


def against_oracle(q, got, ref, F, N):
    assert got["post"].shape == (F, N)
    assert (q.unpack_bits(got["hard"], N) == ref["hard"][:F]).all()
    assert (got["iters"] == ref["iters"][:F]).all() and (got["ok"] == ref["synd_ok"][:F]).all()
    assert (got["post"] == ref["post"][:F].view(np.uint32)).all()


def coded_case(rng, code, F):
    """what load_bits / load_erasures get, and the two LLR arrays it stands for (erasures loaded or not)"""
    N, K = code.N, code.N - code.M
    cls = np.zeros(N, np.uint8)
    cls[K:] = 1                                             # parity disclosed: pinned
    cls[:K][rng.random(K) < 0.08] = 1                       # pinned information VNs
    cls[:K][(rng.random(K) < 0.06) & (cls[:K] == 0)] = 2    # punctured ones
    assert (cls[:K] == 1).any() and (cls[:K] == 2).any() and (cls[:K] == 0).sum() > K // 2
    bits = rng.integers(0, 2, (F, N)).astype(np.uint8)
    mag = rng.uniform(1.0, 4.0, F).astype(np.float32)
    nch = np.full(F, N, np.int32)
    short = rng.random(F) < 0.3
    short[0] = True
    nch[short] = rng.integers(K // 2, K, int(short.sum()))
    era = np.zeros((F, N), np.uint8)
    for f in (0, 2, 70, F - 1):                             # a few frames: information VNs, a chain VN, the last chain VN
        era[f, rng.choice(K, 40, replace=False)] = 1
        era[f, K + 5] = era[f, N - 1] = 1
    era[1] = 1                                              # every channel bit of frame 1 erased
    v = np.arange(N)[None, :]
    m = np.where(cls[None, :] == 0, np.where(v < nch[:, None], mag[:, None], PIN), np.where(cls[None, :] == 1, PIN, np.float32(0.0))).astype(np.float32)
    me = m.copy()
    me[era == 1] = 0.0
    # -m keeps the sign where m is 0: a set bit at magnitude 0 is -0.0, as the kernels form it
    return dict(bits=bits, mag=mag, cls=cls, nch=nch, era=era,
                llr={True: np.where(bits == 1, -me, me).astype(np.float32), False: np.where(bits == 1, -m, m).astype(np.float32)})


def run_coded(q, torch, code, rule, param, n_ite, cs, F, erasures):
    dec = q.Decoder(code, code.N, n_ite, rule=rule, rule_param=param, n_frames=F, engine="frames", enable_syndrome=False)
    dec.load_bits(torch.from_numpy(i32(q.pack_bits(cs["bits"][:F]))).cuda(), torch.from_numpy(cs["mag"][:F]).cuda(), torch.from_numpy(cs["cls"]).cuda(),
                  torch.from_numpy(cs["nch"][:F]).cuda())
    if erasures:
        dec.load_erasures(torch.from_numpy(i32(q.pack_bits(cs["era"][:F]))).cuda())
    dec.run()
    return dec, results(dec)


def run_llr(q, torch, code, rule, param, n_ite, llr):
    dec = q.Decoder(code, code.N, n_ite, rule=rule, rule_param=param, n_frames=llr.shape[0], engine="frames", enable_syndrome=False)
    dec.load_llr(torch.from_numpy(llr).cuda())
    dec.run()
    return dec, results(dec)


def three_ways(q, monkeypatch, run, ref, F, N, tag):
    """the default run against the oracle, then the same run with each knob off against the default run"""
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    dec, got = run()
    assert dec.flood_post, tag
    against_oracle(q, got, ref, F, N)
    monkeypatch.setenv("QLDPC_FLOOD_POST", "0")
    dec0, got0 = run()
    assert not dec0.flood_post and same(got, got0), tag
    monkeypatch.delenv("QLDPC_FLOOD_POST")
    monkeypatch.setenv("QLDPC_FLOOD_POST_VN", "0")
    dec1, got1 = run()
    assert dec1.flood_post and same(got, got1), tag
    monkeypatch.delenv("QLDPC_FLOOD_POST_VN")


@pytest.mark.parametrize("rule,param", RULES)
@pytest.mark.parametrize("name", list(CODES))
def test_coded_loads_bit_exact(q, O, torch, codes, monkeypatch, name, rule, param):
    code, og = codes[name]
    cs = coded_case(np.random.default_rng(17), code, max(FRAMES))
    assert (cs["llr"][True][1] == 0.0).all() and np.signbit(cs["llr"][True][1]).any()
    for n_ite in ITES:
        for erasures in (True, False):
            ref = O.decode(og, cs["llr"][erasures], rule, param, n_ite, "flooding", False, 1, n_threads=8)
            for F in FRAMES:
                three_ways(q, monkeypatch, lambda: run_coded(q, torch, code, rule, param, n_ite, cs, F, erasures), ref, F, code.N, (n_ite, erasures, F))


def llr_frames(rng, F, N):
    """real-valued LLRs with random signs; frame 1 all zero (every message +-0.0); frame 2 on a coarse grid (ties min1 == min2 in most checks)"""
    llr = (rng.normal(1.2, 1.5, (F, N)) * np.where(rng.random((F, N)) < 0.5, -1.0, 1.0)).astype(np.float32)
    llr[1] = 0.0
    llr[2] = np.round(llr[2] * 2.0) / 2.0
    return llr


@pytest.mark.parametrize("rule,param", RULES)
@pytest.mark.parametrize("name", list(CODES))
def test_llr_arrays_with_ties_bit_exact(q, O, torch, codes, monkeypatch, name, rule, param):
    code, og = codes[name]
    llr = llr_frames(np.random.default_rng(5), max(FRAMES), code.N)
    for n_ite in ITES:
        ref = O.decode(og, llr, rule, param, n_ite, "flooding", False, 1, n_threads=8)
        for F in FRAMES:
            three_ways(q, monkeypatch, lambda: run_llr(q, torch, code, rule, param, n_ite, llr[:F]), ref, F, code.N, (n_ite, F))
