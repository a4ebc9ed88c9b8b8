#!/usr/bin/env python3
"""What blind reconciliation rounds inside the Monte-Carlo loop (qldpc_mc_blind) cost beside the plain loop, on the headline code (N = 65 536,
K = 52 429, flooding NMS 0.75, <= 50 iterations with the early exit, a 4 096-frame decoder with compact = 2) at a QBER in the waterfall:

    timeout -k 10 900 python tools/mc_blind_cost.py --out profiles/mc_blind_cost.json

blind:  one qldpc_mc_blind (--ask bits per round, --rounds rounds) over --max-frames frames: wall time, launches, decodes / frames, the rows of
        the rounds, the hipEvent time of every stage in total and per launch, and the efficiency f the disclosed bits add up to.
run:    one qldpc_mc_run over the same frames on the same decoder: the same stages; its FER is what the rounds start from.
ratio:  the blind call's decode_ms and total_ms over the run's.  Decoding the whole batch again in every round would cost rounds + 1 decodes per
        frame; decodes / frames says what the pools make of that.
No threshold and no claim: the file is the measurement.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, K, BATCH, N_ITE = 65536, 52429, 4096, 50
BLIND_STAGES = ("source_ms", "encode_ms", "channel_ms", "load_ms", "decode_ms", "select_ms", "advance_ms")
RUN_STAGES = ("source_ms", "encode_ms", "channel_ms", "load_ms", "decode_ms", "monitor_ms")


def measure(q, qber, ask, rounds, max_frames):
    code = q.Code.ira(N, K)
    enc = q.Encoder(code, "IRA")
    dec = q.Decoder(code, enc.K, N_ITE, info_bits_pos=enc.info_bits_pos, rule="NMS", rule_param=0.75, n_frames=BATCH, compact="off")
    mc = q.MonteCarlo(dec, enc, seed=1, batch=BATCH)
    mc.run(qber, 0, BATCH)                                                                 # warm-up: first launches, allocations
    mc.blind(qber, ask, rounds, 0, BATCH)
    r = mc.run(qber, 0, max_frames)
    b = mc.blind(qber, ask, rounds, 0, max_frames)
    rows = b["rounds"]
    out = dict(workload="N %d K %d flooding NMS 0.75, <= %d iterations, early exit, compact = 2, batch %d, QBER %.4f, ask %d bits x <= %d rounds, %d frames"
                        % (N, enc.K, N_ITE, BATCH, qber, ask, rounds, max_frames),
               run=dict(total_ms=r["total_ms"], batches=r["batches"], frames=r["frames"], frame_errors=r["frame_errors"], not_converged=r["not_converged"],
                        stage_ms={k: r[k] for k in RUN_STAGES}),
               blind=dict(total_ms=b["total_ms"], launches=b["launches"], frames=b["frames"], frame_errors=b["frame_errors"], undetected=b["undetected"], open=b["open"],
                          disclosed=b["disclosed"], decodes=b["decodes"], decodes_per_frame=b["decodes"] / b["frames"], stage_ms={k: b[k] for k in BLIND_STAGES},
                          per_launch_ms={k: b[k] / b["launches"] for k in BLIND_STAGES},
                          rounds=[{k: int(row[k]) for k in rows.dtype.names} for row in rows],
                          efficiency=q.mc_blind_efficiency(enc.K, N - enc.K, b["frames"], b["disclosed"], qber),
                          efficiency_without_rounds=q.mc_blind_efficiency(enc.K, N - enc.K, b["frames"], 0, qber)),
               device_bytes=mc.device_bytes)
    out["blind_decode_over_run_decode"] = b["decode_ms"] / r["decode_ms"]
    out["blind_total_over_run_total"] = b["total_ms"] / r["total_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mc_blind_cost.json"))
    ap.add_argument("--qber", type=float, default=0.029)      # the foot of the waterfall: 124 of 16 384 first decodes fail
    ap.add_argument("--ask", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--max-frames", type=int, default=4 * BATCH)
    args = ap.parse_args()
    import _qldpc_loader
    out = measure(_qldpc_loader.load(), args.qber, args.ask, args.rounds, args.max_frames)
    out["what"] = ("blind reconciliation rounds inside the Monte-Carlo loop on the headline code: one qldpc_mc_blind and one qldpc_mc_run over the same frames, the "
                   "stage times of both by hipEvents, decodes per frame, the rows of the rounds and the efficiency the disclosed bits add up to")
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
