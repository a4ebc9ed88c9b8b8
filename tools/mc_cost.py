#!/usr/bin/env python3
"""What the device-resident Monte-Carlo loop (qldpc_mc_run) costs around the decoder, on the headline code (N = 65 536, K = 52 429, flooding
NMS 0.75, <= 50 iterations with the early exit, QBER 2 %, batches of 4 096 frames).  One process per leg; every run merges its leg into the
output file:

    timeout -k 10 600 python tools/mc_cost.py --leg split --out profiles/mc_cost.json && \
    timeout -k 10 900 python tools/mc_cost.py --leg sim   --out profiles/mc_cost.json

split:  the per-batch hipEvent time of every stage of qldpc_mc_run (source, encode, channel, load, decode, fetch + monitor), averaged over
        --steps batches after one warm-up batch, the share (source + channel + monitor) / decode, and frames per second of the whole call.
        With --awgn the same batches are run again through the 6-bit AWGN table (qldpc_mc_set_channel; sigma 0.4869, whose hard-decision
        error rate is the BSC's 2 %) and `channel_ms` and `load_ms` of the soft path (mc_soft_channel, qldpc_load_llr_dev) are printed beside
        the BSC's (mc_channel, qldpc_load_bits_dev).  The levels are not scaled to LLRs, so the soft leg's decode counters mean nothing.
sim:    frames per second of `qldpc_sim` with and without -D at the same point.  A process is timed as a whole at two frame counts and the
        difference taken, so that building the code and the decoder does not count.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, K, QBER, BATCH, N_ITE = 65536, 52429, 0.02, 4096, 50
AWGN_SIGMA = 0.4869                                                    # Phi(-1 / sigma) = 0.02
STAGES = ("source_ms", "encode_ms", "channel_ms", "load_ms", "decode_ms", "monitor_ms")


def leg_split(q, steps, awgn=False):
    code = q.Code.ira(N, K)
    enc = q.Encoder(code, "IRA")
    dec = q.Decoder(code, enc.K, N_ITE, info_bits_pos=enc.info_bits_pos, rule="NMS", rule_param=0.75, n_frames=BATCH)
    mc = q.MonteCarlo(dec, enc, seed=1, batch=BATCH)
    mc.run(QBER, 0, BATCH)                                             # warm-up: first launches, the encoder's workspace
    r = mc.run(QBER, BATCH, steps * BATCH)
    assert r["frames"] == steps * BATCH and r["batches"] == steps
    per_batch = {k: r[k] / steps for k in STAGES}
    around = per_batch["source_ms"] + per_batch["channel_ms"] + per_batch["monitor_ms"]
    soft = {}
    if awgn:
        mc.set_awgn(sigma=AWGN_SIGMA)
        mc.run(QBER, 0, BATCH)                                         # warm-up of the soft path: its first launches
        s = mc.run(QBER, BATCH, steps * BATCH)
        assert s["frames"] == steps * BATCH and s["batches"] == steps
        soft = dict(awgn=dict(sigma=AWGN_SIGMA, levels=64, per_batch_ms={k: s[k] / steps for k in STAGES},
                              channel_ms_soft_vs_bsc=(s["channel_ms"] / steps, per_batch["channel_ms"]),
                              load_ms_soft_vs_bsc=(s["load_ms"] / steps, per_batch["load_ms"]),
                              hard_error_rate=s["channel_flips"] / s["channel_bits"], device_bytes=mc.device_bytes))
        print("per batch of %d frames: channel_ms soft %.4f / BSC %.4f, load_ms soft %.4f / BSC %.4f" % (
            BATCH, s["channel_ms"] / steps, per_batch["channel_ms"], s["load_ms"] / steps, per_batch["load_ms"]))
    return dict(soft, workload="N %d K %d flooding NMS 0.75, <= %d iterations, early exit, QBER %.3f, %d batches of %d frames" % (N, K, N_ITE, QBER, steps, BATCH),
                per_batch_ms=per_batch, source_channel_monitor_over_decode=around / per_batch["decode_ms"],
                frames_per_s=r["frames"] / (r["total_ms"] * 1e-3), decode_only_frames_per_s=r["frames"] / (r["decode_ms"] * 1e-3),
                frame_errors=r["frame_errors"], avg_iterations=r["iter_sum"] / r["frames"], empirical_qber=r["channel_flips"] / r["channel_bits"],
                device_bytes=mc.device_bytes)


def leg_sim():
    exe = os.path.join(ROOT, "qcrypto-ldpc_amd", "host", "qldpc_sim")
    base = [exe, "-N", str(N), "-K", str(K), "-r", "NMS", "-p", "0.75", "-i", str(N_ITE), "-s", "%g:%g:0.01" % (QBER, QBER), "-S", "1"]

    def wall(extra):
        t0 = time.perf_counter()
        p = subprocess.run(base + extra, capture_output=True, text=True, timeout=800)
        if p.returncode != 0:
            raise RuntimeError("qldpc_sim: %d %s" % (p.returncode, p.stderr[-1000:]))
        return time.perf_counter() - t0, [l for l in p.stdout.splitlines() if not l.startswith("#") and "|" in l][-1].strip()

    out = {}
    for name, flag, batch, lo, hi in (("host", [], 1024, 1024, 3072), ("device", ["-D"], BATCH, BATCH, 9 * BATCH)):
        t_lo, _ = wall(flag + ["-b", str(batch), "-f", str(lo)])
        t_hi, row = wall(flag + ["-b", str(batch), "-f", str(hi)])
        out[name] = dict(batch=batch, frames=(lo, hi), wall_s=(t_lo, t_hi), frames_per_s=(hi - lo) / (t_hi - t_lo), row=row)
    out["device_over_host"] = out["device"]["frames_per_s"] / out["host"]["frames_per_s"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("split", "sim"), required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mc_cost.json"))
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--awgn", action="store_true", help="leg split: also time the soft path (6-bit AWGN table) beside the BSC's")
    args = ap.parse_args()
    if args.leg == "sim":
        leg = leg_sim()
    else:
        import _qldpc_loader
        leg = leg_split(_qldpc_loader.load(), args.steps, args.awgn)
    out = {}
    if os.path.exists(args.out):
        out = json.load(open(args.out))
    out["what"] = ("the device-resident Monte-Carlo loop on the headline code: per-batch stage times by hipEvents, and frames per second of "
                   "qldpc_sim with and without -D (whole processes at two frame counts, the difference)")
    out[args.leg] = leg
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(leg))


if __name__ == "__main__":
    main()
