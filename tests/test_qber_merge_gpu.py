"""GPU suite: the merged form of the syndrome-weight QBER estimate on the device (qldpc_qber_set_merge: qk_qber_count_merged) against its host mirror,
merging off against what the estimator gave before, and the sessions' qldpc_recon_estimate_blocks_merged on blocks whose plans puncture half of the
parity and more."""
import numpy as np
import pytest

import qber_merge_ref as mref
import qber_ref

pytestmark = pytest.mark.gpu

FRAMES = (1, 3, 70)
# M = 256: one pass of 256 threads; M = 1 024: four passes, and 16 chunks with checks_per_block = 64 -- runs cross lane-64, pass and chunk boundaries
MERGE_CODES = ((1280, 1024), (5120, 4096))


def dev_rows(q, torch, a):
    return None if a is None else torch.from_numpy(q.pack_bits(a).astype(np.uint32).view(np.int32)).cuda()


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def device_inputs(q, torch, f):
    t = {k: dev_rows(q, torch, f[k]) for k in ("bits", "synd", "erase", "known", "value")}
    t["cls"] = None if f["cls"] is None else torch.from_numpy(f["cls"]).cuda()
    t["nch"] = None if f["nch"] is None else torch.from_numpy(f["nch"]).cuda()
    return t


def run(est, t, F):
    cut = lambda x: None if x is None else x[:F].contiguous()
    return est.estimate(cut(t["bits"]), t["cls"], cut(t["nch"]), cut(t["synd"]), cut(t["erase"]), cut(t["known"]), cut(t["value"]))


def assert_equals_mirror(q, torch, out, want_counts, want_index, tables, F, where):
    L1, L0, qs, llr = tables
    torch.cuda.synchronize()
    counts = out["counts"].cpu().numpy().view(np.uint32)
    assert counts.shape == want_counts[:F].shape and (counts == want_counts[:F]).all(), where
    k = out["index"].cpu().numpy()
    assert (k == want_index[:F]).all(), where
    ok = k >= 0
    got_q, got_m = out["qber"].cpu().numpy(), out["llr_mag"].cpu().numpy()
    assert (got_q[ok] == qs[k[ok]]).all() and (got_m[ok] == llr[k[ok]]).all() and not got_q[~ok].any() and not got_m[~ok].any(), where
    pool = out["pool_counts"].cpu().numpy().astype(np.uint64)
    assert (pool == want_counts[:F].astype(np.uint64).sum(axis=0)).all(), where
    assert int(out["pool_index"].cpu()[0]) == q.qber_argmax_host(pool, L1, L0), where


@pytest.mark.parametrize("shape", MERGE_CODES)
@pytest.mark.parametrize("combo", qber_ref.COMBOS)
def test_merged_device_equals_the_host_mirror(q, torch, monkeypatch, shape, combo):
    """counts, index, estimate and |LLR| of every frame, pooled counts and pooled index: exactly the merged mirror's, for 1 / 3 / 70 frames whose parity is
    erased evenly spaced, at random and in the constructed cases of the CPU suite, checks_per_block auto and 64, staged and memory-gather path"""
    code = q.Code.ira(*shape)
    var, chk = code.edges()
    N, M, Fmax = code.N, code.M, max(FRAMES)
    rng = np.random.default_rng(N * 13 + len(combo))
    f, names = mref.overlay(rng, var, chk, N, M, qber_ref.frames(rng, N, M, Fmax, combo), combo not in ("null", "class"))
    want_counts = np.stack([mref.host_counts(q, code, f, i) for i in range(Fmax)])
    tables = q.qber_table_host(q.QBER_MAX_DEGREE, 256)
    want_index = np.array([q.qber_argmax_host(want_counts[i], tables[0], tables[1]) for i in range(Fmax)], np.int32)
    assert (want_index >= 0).any()
    if combo not in ("class", "all"):      # (their class maps erase a sixth of the information VNs: hardly a run survives)
        assert want_counts[:, code.max_cn_degree + 1:, 0].any()      # merged runs above the code's own largest degree
    t = device_inputs(q, torch, f)
    for staged in (True, False):
        if not staged:
            monkeypatch.setenv("QLDPC_QBER_STAGE", "0")
        for cpb in (0, 64):
            est = q.QberEstimator(code, Fmax, checks_per_block=cpb, merge=True)
            assert est.rows == q.QBER_MAX_DEGREE + 1
            for F in FRAMES:
                assert_equals_mirror(q, torch, run(est, t, F), want_counts, want_index, tables, F, (shape, combo, staged, cpb, F))


def test_merge_off_is_the_estimator_as_it_was(q, torch):
    """merge=False, and merging turned on and off again (the score tables and count rows were replaced by wider ones meanwhile): the unmerged mirror's
    results, D + 1 rows; then on again: the merged mirror's"""
    code = q.Code.ira(*MERGE_CODES[0])
    var, chk = code.edges()
    N, M, D, F = code.N, code.M, code.max_cn_degree, 70
    rng = np.random.default_rng(99)
    f, _ = mref.overlay(rng, var, chk, N, M, qber_ref.frames(rng, N, M, F, "erase_known"), True)
    t = device_inputs(q, torch, f)
    plain_tables, wide_tables = q.qber_table_host(D, 256), q.qber_table_host(q.QBER_MAX_DEGREE, 256)
    plain = np.stack([qber_ref.host_counts(q, code, f, i) for i in range(F)])
    merged = np.stack([mref.host_counts(q, code, f, i) for i in range(F)])
    plain_index = np.array([q.qber_argmax_host(plain[i], plain_tables[0], plain_tables[1]) for i in range(F)], np.int32)
    merged_index = np.array([q.qber_argmax_host(merged[i], wide_tables[0], wide_tables[1]) for i in range(F)], np.int32)
    assert (plain_index != merged_index).any()
    off = q.QberEstimator(code, F)
    assert off.rows == D + 1
    assert_equals_mirror(q, torch, run(off, t, F), plain, plain_index, plain_tables, F, "never merged")
    est = q.QberEstimator(code, F, merge=True)
    est.set_merge(False)
    assert est.rows == D + 1
    assert_equals_mirror(q, torch, run(est, t, F), plain, plain_index, plain_tables, F, "merged, then off")
    est.set_merge(True)
    assert_equals_mirror(q, torch, run(est, t, F), merged, merged_index, wide_tables, F, "on again")


def test_non_chain_codes_are_refused_on_the_device(q, torch):
    for name in ("toy45", "peg504"):
        code = qber_ref.make_code(q, name)
        with pytest.raises(q.QldpcError) as e:
            q.QberEstimator(code, 4, merge=True)
        assert e.value.status == -7 and "chain" in str(e.value), name
        est = q.QberEstimator(code, 4)
        with pytest.raises(q.QldpcError):
            est.set_merge(True)
        assert est.rows == code.max_cn_degree + 1      # and it goes on unmerged
        out = est.estimate(torch.zeros((4, (code.N + 31) // 32), dtype=torch.int32, device="cuda"))
        torch.cuda.synchronize()
        assert (out["index"].cpu().numpy() == 0).all()


# (key bits, planning QBER = the block's true QBER): plans that puncture half of the parity and more -- just above the QBER at which the plan
# falls back to the next lower mother rate -- on three mother codes, a short block at the 65 % cap, and ordinary blocks, 20 of one code (three batches of 8)
HEAVY = [(14500, 0.006), (14337, 0.0055), (14500, 0.023), (14500, 0.055), (15000, 0.052), (3000, 0.02)]
ORDINARY = [(14500, 0.015)] * 14 + [(14900, 0.016), (15360, 0.014), (14800, 0.03), (14999, 0.075)]


def test_sessions_estimate_blocks_merged(q, torch):
    """qldpc_recon_estimate_blocks_merged on a mix of heavily punctured and ordinary blocks: the plain call has nothing to stand on for the former; the
    merged one counts the runs the plan and the code's degrees predict, its estimates are the argmax of its counts, lie within 5 sigma + one grid step
    of each block's own empirical flip rate, are the same for a block alone, touch no key and leave the decode as it was"""
    rng = np.random.default_rng(2026)
    spec = HEAVY[:3] + ORDINARY[:10] + HEAVY[3:] + ORDINARY[10:]
    heavy = [i for i, s in enumerate(spec) if s in HEAVY]
    r = q.Recon(max_blocks=8)
    keys, bobs, msgs, pars, emp = [], [], [], [], []
    for kb, plan_q in spec:
        alice = rng.integers(0, 2, kb).astype(np.uint8)
        bob = alice ^ (rng.random(kb) < plan_q)
        emp.append(float((alice != bob).mean()))
        m, par = r.encode(q.pack_bits(alice), kb, plan_q)
        keys.append(q.pack_bits(alice)); bobs.append(q.pack_bits(bob)); msgs.append(m); pars.append(par)
    kbs = [s[0] for s in spec]
    for i in heavy:
        assert 2 * int(msgs[i].n_punct) >= int(msgs[i].code_m), (spec[i], int(msgs[i].code_m), int(msgs[i].n_punct))
    shapes = [(int(m.code_k), int(m.code_m)) for m in msgs]
    assert len(set(shapes)) >= 3 and max(shapes.count(s) for s in set(shapes)) > 16
    L1, L0, qs, _ = q.qber_table_host(q.QBER_MAX_DEGREE, 256)
    before = [b.copy() for b in bobs]
    qb, counts, _ = r.estimate_blocks(bobs, kbs, msgs, pars)
    for i in heavy:      # as today: one informative check at most, so nothing, the clamp, or whatever one unsatisfied check says
        assert int(counts[i, :, 0].sum()) <= 1 and (qb[i] == 0 or qb[i] == qs[q.qber_argmax_host(counts[i], L1, L0)]), i
        assert qb[i] == 0 or qb[i] == qs[0] or int(counts[i, :, 1].sum()) == 1, i
    qm, cm, pool_q = r.estimate_blocks(bobs, kbs, msgs, pars, merge=True)
    assert all((a == b).all() for a, b in zip(bobs, before))
    edges, want_runs = {}, {}
    for i, m in enumerate(msgs):
        K, M, p = shapes[i][0], shapes[i][1], int(m.n_punct)
        if (K, M) not in edges:
            edges[(K, M)] = q.Code.ira_peg(K + M, K).edges()
        if (K, M, p, kbs[i]) not in want_runs:
            want_runs[(K, M, p, kbs[i])] = mref.session_runs(*edges[(K, M)], K, M, p, kbs[i])
        assert int(cm[i, :, 0].sum()) == want_runs[(K, M, p, kbs[i])], (i, spec[i])
        k = q.qber_argmax_host(cm[i], L1, L0)
        assert k >= 0 and qm[i] == qs[k], i
        sig = qber_ref.sigma(cm[i].tolist(), emp[i])
        step = float(qs[min(k + 1, 255)] - qs[min(k + 1, 255) - 1])
        print("block %2d %s: punctured %.2f, merged q = %.5f, plain %.5f, empirical %.5f, sigma %.5f, step %.5f, runs %d" %
              (i, spec[i], p / M, qm[i], qb[i], emp[i], sig, step, int(cm[i, :, 0].sum())))
        assert abs(float(qm[i]) - emp[i]) <= 5 * sig + step, (i, spec[i])
    assert pool_q == qs[q.qber_argmax_host(cm.astype(np.uint64).sum(axis=0), L1, L0)]
    for i in (heavy[0], heavy[3], heavy[5], 4, len(spec) - 1):      # alone: its own batch, its own place in it
        q1, c1, p1 = r.estimate_blocks([bobs[i]], [kbs[i]], [msgs[i]], [pars[i]], merge=True)
        assert q1[0] == qm[i] and (c1[0] == cm[i]).all() and p1 == qm[i], i
    # the plain call after the merged one is the plain call before it
    qb2, counts2, _ = r.estimate_blocks(bobs, kbs, msgs, pars)
    assert (qb2 == qb).all() and (counts2 == counts).all()
    # the decode that follows is the decode without the calls
    plan_q = [s[1] for s in spec]
    st, fixed, co, it = r.decode_blocks(bobs, kbs, plan_q, msgs, pars)
    st2, fixed2, co2, it2 = q.Recon(max_blocks=8).decode_blocks(bobs, kbs, plan_q, msgs, pars)
    assert (st == st2).all() and (co == co2).all() and (it == it2).all() and all((a == b).all() for a, b in zip(fixed, fixed2))
    # and the merged estimates serve as its `qber`
    st3, fixed3, _, _ = r.decode_blocks(bobs, kbs, qm, msgs, pars)
    assert (st3 == 0).sum() > len(spec) // 2
    for i in np.flatnonzero(st3 == 0):
        assert (q.unpack_bits(fixed3[i], kbs[i]) == q.unpack_bits(keys[i], kbs[i])).all()
