"""GPU suite: the syndrome-weight QBER estimate on the device (qldpc_qber_estimate_dev: counting and argmax kernels) against its host mirrors, the
chain estimate -> load -> run without a host round trip, and the sessions' qldpc_recon_estimate_blocks."""
import numpy as np
import pytest

import qber_ref
from qber_ref import CODES, host_counts, make_code

pytestmark = pytest.mark.gpu

FRAMES = (1, 63, 64, 65, 200)
GRIDS = (2, 256, 1000)


def dev_rows(q, torch, a):
    return None if a is None else torch.from_numpy(q.pack_bits(a).astype(np.uint32).view(np.int32)).cuda()


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.mark.parametrize("name", CODES)
@pytest.mark.parametrize("combo", qber_ref.COMBOS)
def test_device_equals_the_host_mirror(q, torch, monkeypatch, name, combo):
    """counts, index, estimate and |LLR| of every frame, pooled counts and pooled index: exactly the mirror's, for 1 .. 200 frames, checks_per_block auto
    and 64 (several partial histograms per frame), three grid sizes, and both the LDS-staged and the memory-gather path of the counting kernel"""
    code = make_code(q, name)
    D, Fmax = code.max_cn_degree, max(FRAMES)
    rng = np.random.default_rng(len(name) * 977 + len(combo))
    f = qber_ref.frames(rng, code.N, code.M, Fmax, combo)
    want_counts = np.stack([host_counts(q, code, f, i) for i in range(Fmax)])
    t = {k: dev_rows(q, torch, f[k]) for k in ("bits", "synd", "erase", "known", "value")}
    cls = None if f["cls"] is None else torch.from_numpy(f["cls"]).cuda()
    nch = None if f["nch"] is None else torch.from_numpy(f["nch"]).cuda()
    tables = {g: q.qber_table_host(D, g) for g in GRIDS}
    want_index = {g: np.array([q.qber_argmax_host(want_counts[i], tables[g][0], tables[g][1]) for i in range(Fmax)], np.int32) for g in GRIDS}
    assert (want_index[256] >= 0).any()
    for staged in (True, False):
        if not staged:
            monkeypatch.setenv("QLDPC_QBER_STAGE", "0")
        for cpb in (0, 64):
            for g in GRIDS:
                est = q.QberEstimator(code, Fmax, n_grid=g, checks_per_block=cpb)
                L1, L0, qs, llr = tables[g]
                assert (est.q == qs).all() and (est.llr == llr).all()
                for F in FRAMES:
                    cut = lambda x: None if x is None else x[:F].contiguous()
                    out = est.estimate(cut(t["bits"]), cls, cut(nch), cut(t["synd"]), cut(t["erase"]), cut(t["known"]), cut(t["value"]))
                    torch.cuda.synchronize()
                    where = (name, combo, staged, cpb, g, F)
                    counts = out["counts"].cpu().numpy().view(np.uint32)
                    assert (counts == want_counts[:F]).all(), where
                    k = out["index"].cpu().numpy()
                    assert (k == want_index[g][:F]).all(), where
                    ok = k >= 0
                    got_q, got_m = out["qber"].cpu().numpy(), out["llr_mag"].cpu().numpy()
                    assert (got_q[ok] == qs[k[ok]]).all() and (got_m[ok] == llr[k[ok]]).all() and not got_q[~ok].any() and not got_m[~ok].any(), where
                    pool = out["pool_counts"].cpu().numpy().astype(np.uint64)
                    assert (pool == want_counts[:F].astype(np.uint64).sum(axis=0)).all(), where
                    assert int(out["pool_index"].cpu()[0]) == q.qber_argmax_host(pool, L1, L0), where


def test_outputs_are_optional_and_sizes_are_checked(q, torch):
    code = make_code(q, "toy45")
    est = q.QberEstimator(code, 4)
    assert est.device_bytes() > 0
    bits = torch.zeros((5, 2), dtype=torch.int32, device="cuda")
    with pytest.raises(q.QldpcError) as e:
        est.estimate(bits)                                        # more frames than the estimator was made for
    assert e.value.status == -1
    for bad in (dict(n_grid=1), dict(n_grid=1025), dict(q_lo=0.3), dict(q_hi=0.5)):
        with pytest.raises(q.QldpcError) as e:
            q.QberEstimator(code, 4, **bad)
        assert e.value.status == -1, bad
    wide = q.Code.from_edges(70, 1, np.arange(70), np.zeros(70, np.int32))      # one check of degree 70 > 63
    with pytest.raises(q.QldpcError) as e:
        q.QberEstimator(wide, 4)
    assert e.value.status == -7
    # only the per-frame magnitudes asked for (every other output NULL): the all-zero word satisfies every check -> the clamp, k = 0
    mag = torch.full((4,), -1.0, dtype=torch.float32, device="cuda")
    rc = q._L.qldpc_qber_estimate_dev(est._h, q._vp(bits.data_ptr()), None, None, None, None, None, None, 4, None, None, None, q._vp(mag.data_ptr()), None, None)
    torch.cuda.synchronize()
    assert rc == 0 and (mag.cpu().numpy() == est.llr[0]).all()


def test_estimate_feeds_the_load_without_a_host_round_trip(q, torch, gold):
    """estimate -> load_bits with the estimator's device magnitudes -> run, nothing read back in between: hard decisions, iteration counts and flags
    equal those of a decoder loaded with the mirror's magnitudes (PEGReg504x1008, SPA, 65 frames)"""
    code = make_code(q, "peg504")
    F, N = 65, code.N
    rng = np.random.default_rng(65)
    bob = (rng.random((F, N)) < rng.uniform(0.01, 0.07, (F, 1))).astype(np.uint8)      # the zero codeword through a BSC, a QBER per frame
    words = q.pack_bits(bob).astype(np.uint32)
    bits = torch.from_numpy(words.view(np.int32)).cuda()
    est = q.QberEstimator(code, F)
    chained = q.Decoder(code, 504, 30, rule="SPA", n_frames=F)
    out = est.estimate(bits)
    chained.load_bits(bits, out["llr_mag"])
    chained.run()
    got = (chained.fetch_packed().cpu().numpy(), *[x.cpu().numpy() for x in chained.fetch_status()])
    L1, L0, qs, llr = q.qber_table_host(code.max_cn_degree, 256)
    k = np.array([q.qber_argmax_host(q.qber_counts_host(code, words[i]), L1, L0) for i in range(F)])
    assert (k >= 0).all() and len(set(k.tolist())) > 8
    plain = q.Decoder(code, 504, 30, rule="SPA", n_frames=F)
    plain.load_bits(bits, torch.from_numpy(llr[k]).cuda())
    plain.run()
    want = (plain.fetch_packed().cpu().numpy(), *[x.cpu().numpy() for x in plain.fetch_status()])
    for a, b in zip(got, want):
        assert (a == b).all()
    assert want[2].sum() > F // 2                                  # most frames decode: the run is not trivially all failures


def informative_checks(M, n_punct):
    """checks of an IRA mother code whose parity neighbours are both disclosed: check c touches parity VNs c - 1 and c of the accumulator, and position j is
    punctured iff floor((j + 1) p / M) > floor(j p / M) (the punct_at rule of csrc/qldpc_recon.hip)"""
    at = lambda j: (j + 1) * n_punct // M > j * n_punct // M
    return sum(1 for c in range(M) if not at(c) and (c == 0 or not at(c - 1)))


def test_sessions_estimate_blocks(q, torch):
    """qldpc_recon_estimate_blocks on blocks of mixed lengths and rates (three batches in the largest group: the third reuses the first one's staging set): a block's estimate and counts alone and in the
    mix, the number of informative checks from (M, n_punct), the pooled estimate against the true flip rate, keys untouched, the decode unchanged"""
    qtrue = 0.02
    rng = np.random.default_rng(404)
    spec = [(14500, 0.015)] * 5 + [(15000, 0.05), (3000, 0.02), (14337, 0.014), (14900, 0.016), (14999, 0.015), (15360, 0.015), (14800, 0.048), (15100, 0.015)] + [(14500, 0.015)] * 8
    r = q.Recon(max_blocks=8)
    keys, bobs, msgs, pars, flips = [], [], [], [], 0
    for kb, plan_q in spec:
        alice = rng.integers(0, 2, kb).astype(np.uint8)
        bob = alice ^ (rng.random(kb) < qtrue)
        flips += int((alice != bob).sum())
        m, par = r.encode(q.pack_bits(alice), kb, plan_q)
        keys.append(q.pack_bits(alice)); bobs.append(q.pack_bits(bob)); msgs.append(m); pars.append(par)
    kbs = [s[0] for s in spec]
    assert len({(m.code_k, m.code_m) for m in msgs}) >= 3 and sum(1 for m in msgs if (m.code_k, m.code_m) == (msgs[0].code_k, msgs[0].code_m)) > 16
    assert any(m.n_punct for m in msgs)
    before = [b.copy() for b in bobs]
    qb, counts, pool_q = r.estimate_blocks(bobs, kbs, msgs, pars)
    assert all((a == b).all() for a, b in zip(bobs, before))
    L1, L0, qs, _ = q.qber_table_host(q.QBER_MAX_DEGREE, 256)
    for i, m in enumerate(msgs):
        assert int(counts[i, :, 0].sum()) == informative_checks(int(m.code_m), int(m.n_punct)), i
        assert counts[i, 0, 0] == 0 and qb[i] == qs[q.qber_argmax_host(counts[i], L1, L0)], i
    for i in (0, 5, 6, len(spec) - 1):                             # alone: its own batch, its own place in it
        q1, c1, p1 = r.estimate_blocks([bobs[i]], [kbs[i]], [msgs[i]], [pars[i]])
        assert q1[0] == qb[i] and (c1[0] == counts[i]).all() and p1 == qb[i], i
    pool = counts.astype(np.uint64).sum(axis=0)
    k = q.qber_argmax_host(pool, L1, L0)
    emp = flips / sum(kbs)
    sig = qber_ref.sigma(pool.tolist(), emp)
    step = float(qs[k + 1] - qs[k])
    print("pooled q = %.5f, empirical %.5f, sigma %.5f; per block %s" % (pool_q, emp, sig, np.round(qb, 4)))
    assert pool_q == qs[k] and abs(pool_q - emp) <= 5 * sig + step
    # a header that does not match its block is left out, the others are estimated
    bad = [q.ReconMsg.from_buffer_copy(m) for m in msgs[:3]]
    bad[1].code_m += 32
    q3, c3, _ = r.estimate_blocks(bobs[:3], kbs[:3], bad, pars[:3])
    assert q3[1] == 0 and not c3[1].any() and q3[0] == qb[0] and q3[2] == qb[2]
    # the decode that follows is the decode without the call
    plan_q = [s[1] for s in spec]
    st, fixed, co, it = r.decode_blocks(bobs, kbs, plan_q, msgs, pars)
    st2, fixed2, co2, it2 = q.Recon(max_blocks=8).decode_blocks(bobs, kbs, plan_q, msgs, pars)
    assert (st == st2).all() and (co == co2).all() and (it == it2).all() and all((a == b).all() for a, b in zip(fixed, fixed2))
    # and the estimates serve as its `qber`
    st3, fixed3, _, _ = r.decode_blocks(bobs, kbs, qb, msgs, pars)
    for i in np.flatnonzero(st3 == 0):
        assert (q.unpack_bits(fixed3[i], kbs[i]) == q.unpack_bits(keys[i], kbs[i])).all()
