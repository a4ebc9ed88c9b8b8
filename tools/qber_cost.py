#!/usr/bin/env python3
"""What the syndrome-weight QBER estimate (qldpc_qber_estimate_dev) costs and how sharp it is, from one run on an MI355X:

    timeout -k 10 600 python tools/qber_cost.py --out profiles/qber_cost.json

The headline shape -- rate 0.8, N = 65 536 (IRA, K = 52 429, M = 13 107), 4 096 frames, q = 0.02; frames as bench.py forms them: the key VNs through the
BSC, the parity VNs disclosed (class map: pinned); the all-zero codeword -- in one process, hipEvent ms, median of 7 after a warm-up call:

  estimator   `headline`: bits + class map.  `bits_only`: no class map, flips on every VN (every VN noisy).  `punctured`: the headline with n_channel and an
              erase row that punctures a quarter of the parity (what a session frame brings).  For each: the whole call (clears, class rows, counting kernel,
              argmax kernel, pool) and the counting kernel without argmax and pool; for the headline also the counting kernel on its memory-gather path
              (QLDPC_QBER_STAGE=0)
  syndrome    qldpc_syndrome_dev on the headline's bits: the existing kernel that makes the same gathers without counting (one thread per 32 checks)
  decode      one early-exit decode of the headline batch (flooding NMS 0.75, <= 50 iterations): load_bits + run, with the true |LLR| and with the estimator's
  spread      per-frame estimate minus the frame's empirical flip rate over its noisy VNs: mean and standard deviation, grids of 256 and 1 024 points, and
              the pooled estimate

With --merge the tool measures the merged form instead (qldpc_qber_set_merge: runs of checks across erased parity VNs are one observation each) and
writes profiles/qber_merge_cost.json:

    timeout -k 10 600 python tools/qber_cost.py --merge

The same shape and frames, one process, hipEvent ms, median of 7: (1) the unmerged call, (2) the merged call with nothing erased, (3) / (4) the merged call
with 25 % / 49 % of the parity erased, evenly spaced; for (3) and (4) also the unmerged call on the same inputs.  Every leg: the whole call, the counting kernel
alone, the observations per frame and the spread of the per-frame estimate against the frame's empirical flip rate.  Expected: at most 2 x leg 1 at 49 %.

No threshold: the file is the measurement.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, K, FRAMES, N_ITE, QBER = 65536, 52429, 4096, 50, 0.02


def timed(torch, fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(reps):
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return dict(ms=float(np.median(ms)), ms_all=[float(x) for x in ms])


def spaced(M, p):
    """the sessions' evenly spaced puncture pattern: position j of M is erased iff floor((j + 1) p / M) > floor(j p / M)"""
    j = np.arange(M, dtype=np.int64)
    return ((j + 1) * p // M > j * p // M).astype(np.uint8)


def merge_legs(q, torch, args, code, bits, d_cls, d_nch, emp_key, dev):
    F, M = args.frames, N - K
    plain, merged = q.QberEstimator(code, F), q.QberEstimator(code, F, merge=True)
    plain.set_stream(); merged.set_stream()
    k0 = int(np.searchsorted(plain.q, QBER))
    out = dict(workload="N %d K %d IRA (M %d, check degrees <= %d), %d frames, q = %g, all-zero codeword; key VNs through the BSC, parity pinned, erased parity by "
                        "an erase row per frame" % (N, K, M, code.max_cn_degree, F, QBER), grid_step_at_q=float(plain.q[k0] - plain.q[k0 - 1]),
               device_bytes=dict(unmerged=plain.device_bytes(), merged=merged.device_bytes()))

    def leg(est, a):
        res = est.estimate(*a)
        t = dict(call=timed(torch, lambda: est.estimate(*a, out=res), args.reps),
                 counting=timed(torch, lambda: est.estimate(*a, out=res, index=False, pool=False), args.reps))
        est.estimate(*a, out=res)
        torch.cuda.synchronize()
        k = res["index"].cpu().numpy()
        err = res["qber"].cpu().numpy().astype(np.float64)[k >= 0] - emp_key[k >= 0]
        t.update(observations_per_frame=float(res["counts"][:, 1:, 0].sum().item() / F), frames_without_estimate=int((k < 0).sum()),
                 mean_error=float(err.mean()) if err.size else None, sigma=float(err.std()) if err.size else None,
                 pooled=float(est.q[int(res["pool_index"].cpu()[0])]), empirical=float(emp_key.mean()))
        return t
    out["1_unmerged"] = leg(plain, (bits, d_cls))
    out["2_merged_nothing_erased"] = leg(merged, (bits, d_cls))
    for n, pct in ((3, 25), (4, 49)):
        row = np.zeros(N, np.uint8)
        row[K:] = spaced(M, M * pct // 100)
        d_erase = dev(row)[None, :].repeat(F, 1).contiguous()
        a = (bits, d_cls, d_nch, None, d_erase)
        out["%d_merged_%d_percent_erased" % (n, pct)] = leg(merged, a)
        out["%d_unmerged_%d_percent_erased" % (n, pct)] = leg(plain, a)
    base = out["1_unmerged"]
    out["ratio_to_leg_1"] = {k: dict(call=v["call"]["ms"] / base["call"]["ms"], counting=v["counting"]["ms"] / base["counting"]["ms"])
                             for k, v in out.items() if isinstance(v, dict) and "call" in v}
    print(json.dumps({k: (v["call"]["ms"], v["counting"]["ms"], v["observations_per_frame"], v["sigma"]) for k, v in out.items() if isinstance(v, dict) and "call" in v}), flush=True)
    json.dump(out, open(args.out, "w"), indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge", action="store_true", help="measure the merged form instead: profiles/qber_merge_cost.json")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frames", type=int, default=FRAMES)
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "qber_merge_cost.json" if args.merge else "qber_cost.json")
    import torch

    import _qldpc_loader
    q = _qldpc_loader.load()
    F, M = args.frames, N - K
    code = q.Code.ira(N, K)
    rng = np.random.default_rng(1)
    flips = rng.random((F, N)) < QBER
    dev = lambda a: torch.from_numpy(q.pack_bits(a).astype(np.uint32).view(np.int32)).cuda()
    all_bits = dev(flips)
    emp_all, emp_key = flips.mean(axis=1), flips[:, :K].mean(axis=1)
    flips[:, K:] = False
    bits = dev(flips)
    cls = np.zeros(N, np.uint8); cls[K:] = 1
    erase_row = np.zeros(N, np.uint8); erase_row[K::4] = 1
    d_cls = torch.from_numpy(cls).cuda()
    d_nch = torch.full((F,), K, dtype=torch.int32, device="cuda")
    if args.merge:
        return merge_legs(q, torch, args, code, bits, d_cls, d_nch, emp_key, dev)
    d_erase = dev(erase_row)[None, :].repeat(F, 1).contiguous()
    forms = dict(headline=(bits, d_cls), bits_only=(all_bits,), punctured=(bits, d_cls, d_nch, None, d_erase))
    truth = dict(headline=emp_key, bits_only=emp_all, punctured=emp_key)
    out = dict(workload="N %d K %d IRA (M %d, check degrees <= %d), %d frames, q = %g, all-zero codeword; headline: key VNs through the BSC, parity pinned"
                        % (N, K, M, code.max_cn_degree, F, QBER))

    est = q.QberEstimator(code, F)
    est.set_stream()
    res, est_t = {}, {}
    for name, a in forms.items():
        res[name] = est.estimate(*a)
        est_t[name] = dict(call=timed(torch, lambda: est.estimate(*a, out=res[name]), args.reps),
                           counting=timed(torch, lambda: est.estimate(*a, out=res[name], index=False, pool=False), args.reps))
    os.environ["QLDPC_QBER_STAGE"] = "0"
    gat = q.QberEstimator(code, F)
    del os.environ["QLDPC_QBER_STAGE"]
    gat.set_stream()
    res_g = gat.estimate(*forms["headline"])
    est_t["headline"]["counting_memory_gather"] = timed(torch, lambda: gat.estimate(*forms["headline"], out=res_g, index=False, pool=False), args.reps)
    torch.cuda.synchronize()
    assert (res_g["counts"] == res["headline"]["counts"]).all()
    out["estimator_ms"] = est_t
    out["estimator_device_bytes"] = est.device_bytes()
    print("estimator:", {k: {n: t["ms"] for n, t in v.items()} for k, v in est_t.items()}, flush=True)

    spread = {}
    for g in (256, 1024):
        e2 = est if g == 256 else q.QberEstimator(code, F, n_grid=g)
        k0 = int(np.searchsorted(e2.q, QBER))
        spread[str(g)] = dict(grid_step_at_q=float(e2.q[k0] - e2.q[k0 - 1]))
        for name, a in forms.items():
            r2 = e2.estimate(*a)
            torch.cuda.synchronize()
            err = r2["qber"].cpu().numpy().astype(np.float64) - truth[name]
            spread[str(g)][name] = dict(mean_error=float(err.mean()), sigma=float(err.std()), pooled=float(e2.q[int(r2["pool_index"].cpu()[0])]),
                                        empirical=float(truth[name].mean()), informative_checks_per_frame=float(r2["counts"][:, 1:, 0].sum().item() / F))
    out["spread"] = spread
    print("spread:", spread, flush=True)
    json.dump(out, open(args.out, "w"), indent=1)

    dec = q.Decoder(code, K, N_ITE, rule="NMS", rule_param=0.75, n_frames=F, engine="frames")
    dec.set_stream()
    synd = dec.syndrome_of(bits)
    synd_buf = torch.empty_like(synd)
    out["syndrome_dev_ms"] = timed(torch, lambda: q._L.qldpc_syndrome_dev(dec._h, q._vp(bits.data_ptr()), q._vp(synd_buf.data_ptr()), F), args.reps)
    print("syndrome_dev:", out["syndrome_dev_ms"]["ms"], flush=True)
    # the syndrome weight is the estimator's count of unsatisfied checks: the two kernels saw the same checks
    weight = sum(int(torch.bitwise_and(torch.bitwise_right_shift(synd, s), 1).sum().item()) for s in range(32))
    assert weight == int(res["headline"]["counts"][:, :, 1].sum().item())

    decode = {}
    for name, mag in (("true_llr", torch.full((F,), float(q.bsc_llr(QBER)), device="cuda")), ("estimated_llr", res["headline"]["llr_mag"])):
        def run():
            dec.load_bits(bits, mag, d_cls)
            dec.run()
        t = timed(torch, run, args.reps)
        it, ok = (x.cpu().numpy() for x in dec.fetch_status())
        t.update(iteration_sum=int(it.sum()), frames_not_ok=int((ok == 0).sum()))
        decode[name] = t
    out["decode_early_exit_ms"] = decode
    print("decode:", {k: (v["ms"], v["iteration_sum"], v["frames_not_ok"]) for k, v in decode.items()}, flush=True)
    json.dump(out, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
