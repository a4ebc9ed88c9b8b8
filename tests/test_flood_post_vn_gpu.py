"""GPU suite (-m gpu): the posterior pass between two iterations of the posterior form as its own kernel (qk_vn_fpost, qldpc_kernels_fpost.h:
one launch for all degree classes, one record per VN) against the CPU oracle, against the same decoder with QLDPC_FLOOD_POST_VN=0 (the pass on
qk_vn_flood, a launch per bucket) and with QLDPC_FLOOD_POST=0 (explicit messages): hard words, iteration counts, success flags and posteriors
as bit patterns.  The oracle is computed once per (code, rule, iteration count) for the largest batch; smaller batches are its first frames."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RULES = [("MS", 0.0), ("OMS", 0.35), ("NMS", 0.75)]
CODES = {"r08": (4096, 3277), "r05": (2048, 1024)}
FRAMES = (3, 64, 130)                                  # partial group, full group, three groups (the last one with 62 padding lanes)
ITES = (1, 2, 5)                                       # no in-between pass at all; one; both parities of the check state
# the VNs a wave of qk_vn_fpost takes from a class of degree <= 4 / above (QK_FPV_UN, qldpc_kernels_fpost.h) and the waves of a workgroup (QK_WAVES)
UN_A, UN_B, WAVES = 4, 2, 4


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
        out[name] = (c, O.Graph.from_edges(c.N, c.M, var, chk), np.bincount(var, minlength=c.N)[:k])
    return out


def i32(words):
    return words.astype(np.int64).astype(np.uint32).view(np.int32)


def results(dec):
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


def stats(dec):
    return {s["name"]: s for s in dec.profile_read()}


def run_llr(q, torch, code, rule, param, n_ite, llr):
    dec = q.Decoder(code, code.N, n_ite, rule=rule, rule_param=param, n_frames=llr.shape[0], engine="frames", enable_syndrome=False)
    dec.profile(True)
    dec.load_llr(torch.from_numpy(llr).cuda())
    dec.run()
    return dec, results(dec)


def knobs(monkeypatch, post, post_vn):
    for name, on in (("QLDPC_FLOOD_POST", post), ("QLDPC_FLOOD_POST_VN", post_vn)):
        if on:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, "0")


def classes(deg):
    """the degree classes of qk_vn_fpost: {degree: VN count}"""
    d, n = np.unique(deg, return_counts=True)
    assert d.max() <= 12
    return dict(zip(d.tolist(), n.tolist()))


def record_bytes(deg, F):
    """what the records of qk_vn_fpost add to the moved bytes of ONE in-between pass: {v, row[0 .. D)} padded to 16 bytes, read once per 64-frame group"""
    return sum(n * ((d + 1 + 3) // 4) * 16.0 for d, n in classes(deg).items()) * (F / 64.0)


def test_the_lists_have_tails(codes):
    """in at least one code no degree class fills its last wave or its last workgroup (UN and UN x QK_WAVES entries), so the tail path of the
    kernel (repeat entry i0) and a last workgroup with idle waves both run in every class; the cap-4 bucket of that code is not uniform either"""
    tails = []
    for name, (code, og, deg) in codes.items():
        cl = classes(deg)
        print(name, cl)
        assert {3, 11} <= set(cl)
        tails.append(all(n % (UN_A if d <= 4 else UN_B) != 0 and n % ((UN_A if d <= 4 else UN_B) * WAVES) != 0 for d, n in cl.items()) and len(cl) > 2)
    assert any(tails)


@pytest.mark.parametrize("rule,param", RULES)
@pytest.mark.parametrize("name", list(CODES))
def test_llr_arrays_bit_exact(q, O, torch, codes, monkeypatch, name, rule, param):
    code, og, deg = codes[name]
    llr = llr_frames(np.random.default_rng(5), max(FRAMES), code.N)
    for n_ite in ITES:
        ref = O.decode(og, llr, rule, param, n_ite, "flooding", False, 1, n_threads=8)
        for F in FRAMES:
            knobs(monkeypatch, True, True)
            dec, got = run_llr(q, torch, code, rule, param, n_ite, llr[:F])
            assert dec.flood_post and dec.last_run_iterations == n_ite
            against_oracle(q, got, ref, F, code.N)
            knobs(monkeypatch, True, False)
            dec1, got1 = run_llr(q, torch, code, rule, param, n_ite, llr[:F])
            assert dec1.flood_post and same(got, got1), (n_ite, F)
            knobs(monkeypatch, False, True)
            dec0, got0 = run_llr(q, torch, code, rule, param, n_ite, llr[:F])
            assert not dec0.flood_post and same(got, got0), (n_ite, F)
            # a pass is one vn_update record whichever kernel runs it: n_ite - 1 in between, the closing pair, the pair of fetch_post;
            # the new kernel shows in the record bytes it moves on top of what the pass on qk_vn_flood moves
            st, st1 = stats(dec), stats(dec1)
            assert st["vn_update"]["launches"] == st1["vn_update"]["launches"] == n_ite + 1 + 2
            assert st["cn_update"]["launches"] == st1["cn_update"]["launches"] == n_ite
            assert st["vn_update"]["alg_bytes"] == st1["vn_update"]["alg_bytes"]
            extra = st["vn_update"]["moved_bytes"] - st1["vn_update"]["moved_bytes"]
            assert extra == pytest.approx((n_ite - 1) * record_bytes(deg, F), rel=1e-9, abs=1e-6), (n_ite, F)


def test_load_bits_with_pinned_parity_vns(q, torch, codes, monkeypatch):
    """coded LLRs as the benchmark loads them (received bits, one magnitude per frame, every parity VN pinned) against the same run with the
    in-between pass on qk_vn_flood"""
    code, og, deg = codes["r08"]
    K, F, n_ite = code.N - code.M, 130, 5
    rng = np.random.default_rng(17)
    bits = rng.integers(0, 2, (F, code.N)).astype(np.uint8)
    mag = rng.uniform(1.0, 4.0, F).astype(np.float32)
    cls = np.zeros(code.N, np.uint8)
    cls[K:] = q.VN_PINNED
    out = []
    for post_vn in (True, False):
        knobs(monkeypatch, True, post_vn)
        dec = q.Decoder(code, code.N, n_ite, rule="NMS", rule_param=0.75, n_frames=F, engine="frames", enable_syndrome=False)
        dec.profile(True)
        dec.load_bits(torch.from_numpy(i32(q.pack_bits(bits))).cuda(), torch.from_numpy(mag).cuda(), torch.from_numpy(cls).cuda())
        dec.run()
        assert dec.flood_post
        out.append((results(dec), stats(dec)))
    (got, st), (got1, st1) = out
    assert same(got, got1)
    assert st["vn_update"]["launches"] == st1["vn_update"]["launches"] == n_ite + 1 + 2
    assert st["vn_update"]["moved_bytes"] - st1["vn_update"]["moved_bytes"] == pytest.approx((n_ite - 1) * record_bytes(deg, F), rel=1e-9)
