#!/usr/bin/env python3
"""What giving up on frames whose syndrome weight has stopped falling (qldpc_decoder_cfg.giveup_patience) costs and buys, from one run on an MI355X:

    timeout -k 10 600 python tools/giveup_cost.py --out profiles/giveup_cost.json [--bench new=FILE parent_a=FILE parent_b=FILE]

grid:  the headline shape -- rate 0.8, N = 65 536, 4 096 frames, flooding NMS 0.75, <= 50 iterations with the early exit, compact auto -- at QBER
       0.029 and 0.0325 with patience 0 (off), 4, 8 and 16, the same frames (all-zero codeword through the BSC) in every cell.  Per cell: hipEvent ms per
       batch (load + run, median of 7), lane-iterations (qldpc_last_run_stats), frame errors, frames given up, false give-ups (frames ok at patience 0
       and not ok here), and the syndrome + status time of one profiled batch (qldpc_profile_read).
blind: one qldpc_mc_blind at 0.0325, 64 bits a request, at most 4 rounds, 4 096 frames, with patience 0 and 8, both decoders with freeze_messages = 1.
bench: --bench name=FILE takes the `early_exit` leg out of the result line of a `bench.py --full` run kept in FILE: this commit with the option off and
       the parent commit twice; the new value has to lie within the spread of the parent's two.
No threshold, no recommended patience: the file is the measurement.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, K, FRAMES, N_ITE = 65536, 52429, 4096, 50
QBERS, PATIENCE = (0.029, 0.0325), (0, 4, 8, 16)


def cell(q, torch, code, bits, mag, patience, reps):
    dec = q.Decoder(code, K, N_ITE, rule="NMS", rule_param=0.75, n_frames=FRAMES, engine="frames", giveup=patience)
    dec.set_stream()

    def decode():
        dec.load_bits(bits, mag)
        dec.run()

    decode()      # warm-up: first launches, the generations of a compacting run
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(reps):
        a.record()
        decode()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    st = dec.last_run_stats()
    it, ok = (t.cpu().numpy() for t in dec.fetch_status())
    words = dec.fetch_packed()
    wrong = (words[:, :K // 32] != 0).any(1) | ((words[:, K // 32] >> (32 - K % 32)) != 0)      # an information bit of the all-zero codeword decoded as 1 (MSB-first)
    gave = dec.fetch_giveup()[0].cpu().numpy() if patience else np.zeros(FRAMES, np.int32)
    dec.profile(True)
    dec.profile_clear()
    decode()
    prof = {p["name"]: dict(launches=p["launches"], ms=p["total_ms"]) for p in dec.profile_read()}
    dec.profile(False)
    out = dict(ms_per_batch=float(np.median(ms)), ms_all=[float(x) for x in ms], lane_iterations=st["lane_iterations"], compactions=st["compactions"],
               iteration_sum=int(it.sum()), frame_errors=int(wrong.sum().item()), frames_not_ok=int((ok == 0).sum()), given_up=int(gave.sum()),
               syndrome_ms=prof.get("syndrome", {}).get("ms", 0.0), status_ms=prof.get("status", {}).get("ms", 0.0), profiled_batch=prof)
    return out, ok


def grid(q, torch, reps):
    code = q.Code.ira(N, K)
    out = {}
    for qber in QBERS:
        rng = np.random.default_rng(1)
        flips = rng.random((FRAMES, N)) < qber
        bits = torch.from_numpy(q.pack_bits(flips).astype(np.uint32).view(np.int32)).cuda()
        mag = torch.full((FRAMES,), float(q.bsc_llr(qber)), device="cuda")
        row, ok0 = {}, None
        for p in PATIENCE:
            row[str(p)], ok = cell(q, torch, code, bits, mag, p, reps)
            ok0 = ok if p == 0 else ok0
            row[str(p)]["false_give_ups"] = int(((ok0 != 0) & (ok == 0)).sum())
            print("qber %.4f patience %2d: %s" % (qber, p, {k: v for k, v in row[str(p)].items() if k not in ("ms_all", "profiled_batch")}), flush=True)
        out["%.4f" % qber] = row
    return out


def blind(q, qber, ask, rounds):
    code = q.Code.ira(N, K)
    enc = q.Encoder(code, "IRA")
    out = {}
    for p in (0, 8):
        dec = q.Decoder(code, enc.K, N_ITE, info_bits_pos=enc.info_bits_pos, rule="NMS", rule_param=0.75, n_frames=FRAMES, engine="frames", giveup=p,
                        freeze_messages=True, compact="off")
        mc = q.MonteCarlo(dec, enc, seed=1, batch=FRAMES)
        mc.blind(qber, ask, rounds, 0, FRAMES)      # warm-up: the pools, first launches
        before = dec.giveup_total()
        res = mc.blind(qber, ask, rounds, 0, FRAMES)
        out[str(p)] = dict(rows=[{k: int(r[k]) for k in ("frames", "frame_errors", "not_converged", "iter_sum", "disclosed")} for r in res["rounds"]],
                           open=int(res["open"]), disclosed=int(res["disclosed"]), decodes=int(res["decodes"]), launches=int(res["launches"]),
                           decode_ms=float(res["decode_ms"]), total_ms=float(res["total_ms"]), given_up=dec.giveup_total() - before)
        print("blind patience %d: %s" % (p, out[str(p)]), flush=True)
    return dict(workload="qldpc_mc_blind, QBER %.4f, %d bits a request, at most %d rounds, %d frames, freeze_messages = 1, compact off" % (qber, ask, rounds, FRAMES), patience=out)


def bench_leg(pairs):
    out = {}
    for pair in pairs:
        name, path = pair.split("=", 1)
        lines = [l for l in open(path) if l.lstrip().startswith("{")]
        out[name] = json.loads(lines[-1])["early_exit"]
    if {"new", "parent_a", "parent_b"} <= set(out):
        lo, hi = sorted((out["parent_a"]["value"], out["parent_b"]["value"]))
        out["new_within_parent_spread"] = bool(lo <= out["new"]["value"] <= hi)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "giveup_cost.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--legs", default="grid,blind")
    ap.add_argument("--bench", nargs="*", default=[], metavar="NAME=FILE")
    ap.add_argument("--merge", action="store_true", help="start from what --out holds already (add a leg to an earlier run's file)")
    args = ap.parse_args()
    import torch

    import _qldpc_loader
    q = _qldpc_loader.load()
    out = dict(workload="N %d K %d IRA, flooding NMS 0.75, <= %d iterations, early exit, compact auto, %d frames (64 groups), all-zero codeword through the BSC"
                        % (N, K, N_ITE, FRAMES))
    if args.merge and os.path.exists(args.out):
        out = json.load(open(args.out))
    if "grid" in args.legs:
        out["grid"] = grid(q, torch, args.reps)
        json.dump(out, open(args.out, "w"), indent=1)
    if "blind" in args.legs:
        out["blind"] = blind(q, 0.0325, 64, 4)
    if args.bench:
        out["bench_early_exit"] = bench_leg(args.bench)
    json.dump(out, open(args.out, "w"), indent=1)


if __name__ == "__main__":
    main()
