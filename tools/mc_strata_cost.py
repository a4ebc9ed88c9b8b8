#!/usr/bin/env python3
"""What the fixed-weight channel of the error strata (qldpc_mc_strata, kernel mc_channel_weight) costs beside the decode, on the headline code
(N = 65 536, K = 52 429, flooding NMS 0.75, <= 50 iterations with the early exit, batches of 4 096 frames, chunks of 64 frames):

    timeout -k 10 900 python tools/mc_strata_cost.py --out profiles/mc_strata_cost.json

strata: one strata call over --points weights (evenly spaced over --weights lo:hi) with --max-frames per weight and no stop rule, |LLR| of
        --design-qber: wall time, rounds, frames and the hipEvent time of every stage per round.
sweep:  one qldpc_mc_sweep over as many QBER points (weight / K each) on the same frames: the same stages; its channel stage is the BSC kernel
        mc_channel over the slot tables of the round, the baseline.
ratio:  channel_ms / decode_ms of both, and the strata's channel_ms over the sweep's (about 5 x the generator work is expected).
No threshold and no claim: the file is the measurement.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, K, BATCH, N_ITE, CHUNK = 65536, 52429, 4096, 50, 64
STAGES = ("source_ms", "encode_ms", "channel_ms", "load_ms", "erase_ms", "decode_ms", "monitor_ms")


def leg(res, rows):
    return dict(total_ms=res["total_ms"], rounds=res["rounds"], frames=res["frames"], per_round_ms={k: res[k] / res["rounds"] for k in STAGES},
                channel_over_decode=res["channel_ms"] / res["decode_ms"], frame_errors=[int(x) for x in rows["frame_errors"]])


def measure(q, weights, design_qber, max_frames):
    code = q.Code.ira(N, K)
    enc = q.Encoder(code, "IRA")
    dec = q.Decoder(code, enc.K, N_ITE, info_bits_pos=enc.info_bits_pos, rule="NMS", rule_param=0.75, n_frames=BATCH)
    mc = q.MonteCarlo(dec, enc, seed=1, batch=BATCH)
    qbers = [w / enc.K for w in weights]
    mc.strata(weights[:1], design_qber, max_frames=BATCH, chunk=CHUNK)                     # warm-up: first launches, allocations
    mc.sweep(qbers[:1], max_frames=BATCH, chunk=CHUNK)
    t = mc.strata(weights, design_qber, max_frames=max_frames, chunk=CHUNK)
    st = t["strata"]
    assert (st["channel_flips"] == st["frames"] * st["weight"].astype(np.uint64)).all()
    w = mc.sweep(qbers, max_frames=max_frames, chunk=CHUNK)
    out = dict(workload="N %d K %d flooding NMS 0.75, <= %d iterations, early exit, batch %d, chunk %d, %d weights %d .. %d at the |LLR| of QBER %.4f, "
                        "%d frames per weight" % (N, enc.K, N_ITE, BATCH, CHUNK, len(weights), weights[0], weights[-1], design_qber, max_frames),
               strata=leg(t, st), sweep=leg(w, w["points"]), device_bytes=mc.device_bytes)
    out["strata_channel_over_sweep_channel"] = t["channel_ms"] / w["channel_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mc_strata_cost.json"))
    ap.add_argument("--points", type=int, default=8)
    ap.add_argument("--weights", default="1050:1780")
    ap.add_argument("--design-qber", type=float, default=0.027)
    ap.add_argument("--max-frames", type=int, default=BATCH)
    args = ap.parse_args()
    lo, hi = (int(x) for x in args.weights.split(":"))
    import _qldpc_loader
    out = measure(_qldpc_loader.load(), [int(x) for x in np.linspace(lo, hi, args.points)], args.design_qber, args.max_frames)
    out["what"] = ("the fixed-weight channel of the error strata on the headline code: one qldpc_mc_strata over P weights and one qldpc_mc_sweep over P QBER points "
                   "on the same frames, the per-round stage times of both by hipEvents, channel_ms / decode_ms of both and the ratio of the two channel stages")
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
