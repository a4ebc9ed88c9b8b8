#!/usr/bin/env python3
"""What the device-resident puncture-pattern search (qldpc_mc_search) costs around the decoder, on the headline code (N = 65 536, K = 52 429,
flooding NMS 0.75, <= 50 iterations with the early exit, QBER 2 %, batches of 4 096 frames, F = 64 frames per pattern = 64 patterns per round):

    timeout -k 10 600 python tools/mc_search_cost.py --out profiles/mc_search_cost.json

search: the per-round hipEvent time of every stage of qldpc_mc_search (pattern kernel, expansion, generate, load, erase load, decode, fetch +
        monitor), averaged over --steps rounds after one warm-up round, and the share (pattern + expansion + erase load + monitor) / decode.
run:    qldpc_mc_run without a puncture set over the same frames (the loop as it was before the search existed), for comparison.
No threshold: the only claim to check is that the search's non-decode stages stay small beside decode_ms of the same run.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, K, QBER, BATCH, N_ITE, F, EFF = 65536, 52429, 0.02, 4096, 50, 64, 1.6
SEARCH_STAGES = ("pattern_ms", "expand_ms", "generate_ms", "load_ms", "erase_ms", "decode_ms", "monitor_ms")
RUN_STAGES = ("source_ms", "encode_ms", "channel_ms", "load_ms", "decode_ms", "monitor_ms")


def measure(q, steps):
    code = q.Code.ira(N, K)
    enc = q.Encoder(code, "IRA")
    dec = q.Decoder(code, enc.K, N_ITE, info_bits_pos=enc.info_bits_pos, rule="NMS", rule_param=0.75, n_frames=BATCH)
    mc = q.MonteCarlo(dec, enc, seed=1, batch=BATCH)
    per_round = BATCH // F
    n_punct = min(max(q.parity_bits_to_punct(N, enc.K, q.min_code_rate(QBER, EFF)), 0), N - enc.K)
    mc.search(QBER, n_punct, F, first_pattern=0, max_patterns=per_round, stop_at_goal=False)          # warm-up: first launches, allocations
    r = mc.search(QBER, n_punct, F, first_pattern=per_round, max_patterns=steps * per_round, stop_at_goal=False)
    assert r["patterns"] == steps * per_round and r["batches"] == steps
    search = {k: r[k] / steps for k in SEARCH_STAGES}
    around = search["pattern_ms"] + search["expand_ms"] + search["erase_ms"] + search["monitor_ms"]
    fe = r["stats"]["frame_errors"]
    mc.run(QBER, 0, BATCH)
    p = mc.run(QBER, per_round * F, steps * BATCH)                                                     # the same frames, nothing punctured
    assert p["frames"] == steps * BATCH and p["batches"] == steps
    return dict(workload="N %d K %d flooding NMS 0.75, <= %d iterations, early exit, QBER %.3f, %d rounds of %d patterns x %d frames, %d of %d parity VNs "
                         "punctured (efficiency %.2f)" % (N, enc.K, N_ITE, QBER, steps, per_round, F, n_punct, N - enc.K, EFF),
                search=dict(per_round_ms=search, pattern_expand_erase_monitor_over_decode=around / search["decode_ms"],
                            patterns_per_s=r["patterns"] / (r["total_ms"] * 1e-3), frames_per_s=r["frames"] / (r["total_ms"] * 1e-3),
                            patterns_without_frame_errors=int((fe == 0).sum()), frame_errors=int(fe.sum()), avg_iterations=float(r["stats"]["iter_sum"].sum()) / r["frames"]),
                run=dict(per_batch_ms={k: p[k] / steps for k in RUN_STAGES}, frames_per_s=p["frames"] / (p["total_ms"] * 1e-3), frame_errors=p["frame_errors"],
                         avg_iterations=p["iter_sum"] / p["frames"]),
                device_bytes=mc.device_bytes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mc_search_cost.json"))
    ap.add_argument("--steps", type=int, default=4)
    args = ap.parse_args()
    import _qldpc_loader
    out = measure(_qldpc_loader.load(), args.steps)
    out["what"] = ("the device-resident puncture-pattern search on the headline code: per-round stage times by hipEvents, beside qldpc_mc_run without a "
                   "puncture set on the same frames")
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
