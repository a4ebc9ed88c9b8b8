#!/usr/bin/env python3
"""What guessing rounds inside the Monte-Carlo loop (qldpc_mc_guess) buy and cost beside the plain loop, on the headline code (N = 65 536,
K = 52 429, flooding NMS 0.75, <= 50 iterations with the early exit, a 4 096-frame decoder with compact = 2) at a QBER at the foot of the
waterfall, the shape of tools/mc_blind_cost.py:

    timeout -k 10 900 python tools/mc_guess_cost.py --out profiles/mc_guess_cost.json

run:    one qldpc_mc_run over --max-frames frames: wall time, the stages, its FER: what the guesses start from.
guess:  per g of --bits one qldpc_mc_guess over the same frames on the same decoder in the same process: the FER before (failed first decodes) and
        after (open + closed or rescued wrong), rescued / open / ambiguous, the trials, how many ended with a zero syndrome, their mean iteration
        count, launches, wall time and decode time over the run's, and the hipEvent time of every stage.
No threshold and no claim: the file is the measurement.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, K, BATCH, N_ITE = 65536, 52429, 4096, 50
GUESS_STAGES = ("source_ms", "encode_ms", "channel_ms", "load_ms", "decode_ms", "select_ms", "expand_ms", "pick_ms", "advance_ms")
RUN_STAGES = ("source_ms", "encode_ms", "channel_ms", "load_ms", "decode_ms", "monitor_ms")


def measure(q, qber, bits, max_frames):
    code = q.Code.ira(N, K)
    enc = q.Encoder(code, "IRA")
    dec = q.Decoder(code, enc.K, N_ITE, info_bits_pos=enc.info_bits_pos, rule="NMS", rule_param=0.75, n_frames=BATCH, compact="off")
    mc = q.MonteCarlo(dec, enc, seed=1, batch=BATCH)
    mc.run(qber, 0, BATCH)                                                                 # warm-up: first launches, allocations
    mc.guess(qber, min(bits), 0, BATCH)
    r = mc.run(qber, 0, max_frames)
    out = dict(workload="N %d K %d flooding NMS 0.75, <= %d iterations, early exit, compact = 2, batch %d, QBER %.4f, %d frames"
                        % (N, enc.K, N_ITE, BATCH, qber, max_frames),
               run=dict(total_ms=r["total_ms"], batches=r["batches"], frames=r["frames"], frame_errors=r["frame_errors"], not_converged=r["not_converged"],
                        fer=r["frame_errors"] / r["frames"], stage_ms={k: r[k] for k in RUN_STAGES}),
               guess={})
    for g in bits:
        b = mc.guess(qber, g, 0, max_frames)
        rows = [{k: int(row[k]) for k in b["rows"].dtype.names} for row in b["rows"]]
        failed = rows[1]["frames"] + rows[2]["frames"]
        after = rows[0]["frame_errors"] + rows[1]["frame_errors"] + rows[2]["frames"]
        out["guess"]["g%d" % g] = dict(
            guess_bits=g, trials_per_failed_frame=1 << g, total_ms=b["total_ms"], launches=b["launches"], frames=b["frames"], failed_first_decodes=failed,
            fer_before=(rows[0]["frame_errors"] + failed) / b["frames"], fer_after=after / b["frames"], rescued=b["rescued"], rescued_wrong=rows[1]["frame_errors"],
            open=b["open"], ambiguous=b["ambiguous"], undetected=b["undetected"], trials=b["trials"], n_ok_sum=b["n_ok_sum"],
            trial_iterations_mean=(b["trial_iter_sum"] / b["trials"]) if b["trials"] else None, decodes=b["decodes"], decodes_per_frame=b["decodes"] / b["frames"],
            stage_ms={k: b[k] for k in GUESS_STAGES}, rows=dict(zip(q.MC_GUESS_ROWS, rows)),
            total_over_run_total=b["total_ms"] / r["total_ms"], decode_over_run_decode=b["decode_ms"] / r["decode_ms"])
    out["device_bytes"] = mc.device_bytes
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mc_guess_cost.json"))
    ap.add_argument("--qber", type=float, default=0.029)      # the foot of the waterfall, the point of tools/mc_blind_cost.py
    ap.add_argument("--bits", type=int, nargs="+", default=[0, 4, 8])
    ap.add_argument("--max-frames", type=int, default=4 * BATCH)
    args = ap.parse_args()
    import _qldpc_loader
    out = measure(_qldpc_loader.load(), args.qber, args.bits, args.max_frames)
    out["what"] = ("guessing rounds inside the Monte-Carlo loop on the headline code: one qldpc_mc_run and one qldpc_mc_guess per g over the same frames in one process, "
                   "FER before and after, rescued / open / ambiguous, trials, wall and decode time over the run's, the stage times of all by hipEvents")
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
