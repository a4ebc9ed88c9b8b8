#!/usr/bin/env python3
"""What the vertical-layered schedule costs on BASELINE config 2's code (N = 65 536 IRA, NMS 0.75, QBER 2 %), against the horizontal
schedule on the same frames in the same process.  One process per batch size; every run merges its leg into the output file:

    timeout -k 10 600 python tools/vlayered_cost.py --frames 256  --out profiles/vlayered_cost.json && \
    timeout -k 10 900 python tools/vlayered_cost.py --frames 4096 --out profiles/vlayered_cost.json

Per schedule: ms per sweep from the decoder's own profile stats (fixed sweeps, no early exit), the bytes a sweep moves and the rate that
is, the class / layer counts, and with the early exit the mean sweeps per frame and the reconciled Mbit/s (K bits of every frame whose
syndrome closes / wall time of qldpc_run).  The vertical sweep recomputes a check's fold for each of its VNs, so per frame it reads
2 sum dc^2 - E + N rows and writes E + N; the horizontal sweep reads 2 E and writes 2 E (explicit messages), or moves 2 E + 8 M rows on the
compressed check state it uses by default for min-sum.  The vertical decoder is parity-unpinned against AFF3CT (tests/vlayered_ref.py).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vlayered_cost.json"))
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--k", type=int, default=52429)
    ap.add_argument("--qber", type=float, default=0.02)
    ap.add_argument("--alpha", type=float, default=0.75)
    ap.add_argument("--sweeps", type=int, default=10, help="fixed sweeps of the profiled run")
    ap.add_argument("--n-ite", type=int, default=50)
    ap.add_argument("--steps", type=int, default=3)
    args = ap.parse_args()

    import torch

    import _qldpc_loader
    q = _qldpc_loader.load()
    F, N = args.frames, args.n
    code = q.Code.ira(N, args.k, 0.125, 11, 3, 7)
    enc = q.Encoder(code, "IRA")
    K = enc.K
    rng = np.random.default_rng(7)
    info = rng.integers(0, 2, (F, K)).astype(np.uint8)
    cw = enc.encode_packed(torch.from_numpy(q.pack_bits(info).view(np.int32)).cuda())
    noise = np.zeros((F, N), np.uint8)
    noise[:, :K] = rng.random((F, K), dtype=np.float32) < args.qber               # flips on the key VNs; the parity bits are disclosed exactly
    rx = cw ^ torch.from_numpy(q.pack_bits(noise).view(np.int32)).cuda()
    mag = torch.full((F,), float(q.bsc_llr(args.qber)), device="cuda")
    cls = np.zeros(N, np.uint8)
    cls[K:] = q.VN_PINNED
    cls = torch.from_numpy(cls).cuda()

    var, chk = code.edges()
    dc = np.bincount(chk, minlength=code.M).astype(np.int64)
    dc2 = int((dc ** 2).sum())
    vptr = code.vlayer_order()[1]
    lptr = code.layer_order()[1]
    leg = dict(frames=F, sum_dc2=dc2,
               rows_per_sweep=dict(vlayered=2 * dc2 + 2 * N, hlayered_explicit=4 * code.E, hlayered_compressed_state=2 * code.E + 8 * code.M),
               row_ratio_issue_formula=(2 * dc2 + code.E + N) / (4.0 * code.E),
               vlayer_classes=dict(count=int(code.n_vlayers), smallest=int(np.diff(vptr).min()), largest=int(np.diff(vptr).max())),
               hlayer_layers=dict(count=int(code.n_layers), smallest=int(np.diff(lptr).min()), largest=int(np.diff(lptr).max())))

    def run(dec):
        dec.load_bits(rx, mag, cls)
        dec.run()
        dec.sync()

    def one(name, schedule, env=None):
        for k, v in (env or {}).items():
            os.environ[k] = v
        stat = "vn_vlayer" if schedule == "vlayered" else "layer_update"
        res = {}
        d = q.Decoder(code, K, args.sweeps, info_bits_pos=enc.info_bits_pos, rule="NMS", rule_param=args.alpha, enable_syndrome=False, n_frames=F, schedule=schedule)
        run(d)                                                   # warm-up
        d.profile(True)
        d.profile_clear()
        run(d)
        s = {x["name"]: x for x in d.profile_read()}[stat]
        d.profile(False)
        ms = s["total_ms"] / s["launches"]
        res["fixed"] = dict(sweeps=int(s["launches"]), ms_per_sweep=ms, moved_GB_per_sweep=s["moved_bytes"] / s["launches"] / 1e9,
                            moved_TB_s=s["moved_bytes"] / (s["total_ms"] * 1e-3) / 1e12)
        del d
        torch.cuda.empty_cache()
        if env is None:
            d = q.Decoder(code, K, args.n_ite, info_bits_pos=enc.info_bits_pos, rule="NMS", rule_param=args.alpha, enable_syndrome=True, n_frames=F, schedule=schedule)
            run(d)
            t0 = time.perf_counter()
            for _ in range(args.steps):
                run(d)
            dt = (time.perf_counter() - t0) / args.steps
            it, ok = d.fetch_status()
            good = int(ok.sum().item())
            res["early_exit"] = dict(mean_sweeps=float(it.float().mean().item()), sweeps_launched=int(d.last_run_iterations), fer=1.0 - good / F, ms_per_step=dt * 1e3,
                                     reconciled_Mbit_s=good * K / dt / 1e6)
            del d
            torch.cuda.empty_cache()
        for k in (env or {}):
            del os.environ[k]
        leg[name] = res

    one("vlayered", "vlayered")
    one("hlayered", "hlayered")
    one("hlayered_explicit_messages", "hlayered", {"QLDPC_LAYER_CST": "0"})
    v, h, hx = leg["vlayered"], leg["hlayered"], leg["hlayered_explicit_messages"]
    leg["sweep_time_ratio"] = dict(vertical_over_horizontal=v["fixed"]["ms_per_sweep"] / h["fixed"]["ms_per_sweep"],
                                   vertical_over_horizontal_explicit_messages=v["fixed"]["ms_per_sweep"] / hx["fixed"]["ms_per_sweep"])
    leg["early_exit_rate_ratio"] = h["early_exit"]["reconciled_Mbit_s"] / max(v["early_exit"]["reconciled_Mbit_s"], 1e-9)

    out = {}
    if os.path.exists(args.out):
        out = json.load(open(args.out))
    out["workload"] = "BASELINE config 2: N = %d, K = %d IRA (M = %d, E = %d), NMS %.2f, QBER %.1f %%, parity VNs pinned, fp32, 64-frame groups; <= %d sweeps with early exit" % (
        N, K, code.M, code.E, args.alpha, args.qber * 100, args.n_ite)
    out["parity"] = "vertical layered: parity unpinned against AFF3CT; bit-exact against tests/vlayered_ref.py (tests/test_vlayered_gpu.py)"
    out.setdefault("legs", {})[str(F)] = leg
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(leg))


if __name__ == "__main__":
    main()
