#!/usr/bin/env python3
"""What active-frame compaction gives (or costs) on the horizontal-layered schedule with the per-sweep syndrome exit: compact "off" and "on" on the
same frames in the same process, medians of the timed steps after a warm-up.  One process per case; every run merges its case into the output file:

    timeout -k 10 600 python tools/layered_compact_cost.py --case flat  --frames 4096 --out profiles/layered_compact.json && \
    timeout -k 10 600 python tools/layered_compact_cost.py --case mixed --frames 512  --out profiles/layered_compact.json && \
    timeout -k 10 600 python tools/layered_compact_cost.py --case mixed --frames 4096 --out profiles/layered_compact.json && \
    timeout -k 10 600 python tools/layered_compact_cost.py --case stream --out profiles/layered_compact.json

  flat    the layered_schedule early-exit shape of bench.py: the headline code (N = 65 536 IRA, K = 52 429), NMS 0.75, QBER 2 % on every frame
  mixed   the same code with a QBER per frame ~ U[2 %, 3 %] (what a session's batch looks like), <= 50 sweeps
  stream  BASELINE config 3 through host/qldpc_stream (512 epochs, sessions sized for 512 blocks) with QLDPC_COMPACT unset / 1

Per decoder case and mode: ms per step and reconciled Gbit/s (K bits of every frame whose syndrome closes / wall time of load + run), sweeps launched,
lane-iterations, compactions, the useful fraction (sum of the frames' sweep counts / lane-iterations), the decoder's device bytes (the difference between
the modes is the side buffers and the generations' per-frame state), and from the decoder's own profile stats the mean time of an ordinary sweep, of the
first sweep after a compaction (it reads the old generation's check state through the slot map) and of the posterior gather in front of it.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PARENT_LAYERED_EARLY_EXIT = dict(source="profiles/bench_r03_g.json, layered_schedule.early_exit (the parent commit's recorded run of the same shape)",
                                 ms_per_step=15.172468998935074, Mbit_s=14153.871991109214, avg_sweeps=5.24853515625, sweeps_launched=8)
PARENT_CONFIG3_STREAM = dict(source="profiles/r03_config3_stream_layered.json / tools/README.md (qldpc_stream -b 512 -r 5 from C at the parent commit)", ms=13.2)


def decoder_case(args):
    import torch

    import _qldpc_loader
    q = _qldpc_loader.load()
    F, N = args.frames, 65536
    code = q.Code.ira(N, 52429, 0.125, 11, 3, 7)
    enc = q.Encoder(code, "IRA")
    K = enc.K
    rng = np.random.default_rng(7 if args.case == "flat" else 2)
    qber = np.full(F, 0.02) if args.case == "flat" else rng.uniform(0.02, 0.03, F)
    info = rng.integers(0, 2, (F, K)).astype(np.uint8)
    cw = enc.encode_packed(torch.from_numpy(q.pack_bits(info).view(np.int32)).cuda())
    noise = np.zeros((F, N), np.uint8)
    noise[:, :K] = rng.random((F, K), dtype=np.float32) < qber[:, None].astype(np.float32)      # flips on the key VNs; the parity bits are disclosed exactly
    rx = cw ^ torch.from_numpy(q.pack_bits(noise).view(np.int32)).cuda()
    mag = torch.from_numpy(np.array([q.bsc_llr(float(p)) for p in qber], np.float32)).cuda()
    cls = np.zeros(N, np.uint8)
    cls[K:] = q.VN_PINNED
    cls = torch.from_numpy(cls).cuda()

    def step(dec):
        dec.load_bits(rx, mag, cls)
        dec.run()
        dec.sync()

    res, hard = {}, {}
    for mode in ("off", "on"):
        dec = q.Decoder(code, K, args.n_ite, info_bits_pos=enc.info_bits_pos, rule="NMS", rule_param=0.75, enable_syndrome=True, n_frames=F, schedule="hlayered", compact=mode)
        for _ in range(args.warmup):
            step(dec)
        dts = []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            step(dec)
            dts.append(time.perf_counter() - t0)
        dt = statistics.median(dts)
        it, ok = dec.fetch_status()
        st = dec.last_run_stats()
        good = int(ok.sum().item())
        r = dict(ms_per_step=dt * 1e3, ms_min=min(dts) * 1e3, ms_max=max(dts) * 1e3, reconciled_Gbit_s=good * K / dt / 1e9, fer=1.0 - good / F,
                 mean_sweeps=float(it.float().mean().item()), min_sweeps=int(it.min().item()), max_sweeps=int(it.max().item()), sweeps_launched=int(dec.last_run_iterations),
                 lane_iterations=st["lane_iterations"], compactions=st["compactions"], final_groups=st["final_groups"],
                 useful_fraction=float(it.sum().item()) / max(1, st["lane_iterations"]), device_bytes=int(dec.device_bytes))
        dec.profile(True)
        dec.profile_clear()
        step(dec)
        ks = {s["name"]: s for s in dec.profile_read()}
        dec.profile(False)
        for name, key in (("layer_update", "ordinary_sweep"), ("layer_update_remap", "first_sweep_after_compaction"), ("compact_rows", "posterior_gather")):
            if name in ks:
                r[key] = dict(launches=ks[name]["launches"], mean_ms=ks[name]["total_ms"] / ks[name]["launches"])
        hard[mode] = (dec.fetch_packed().cpu().numpy(), it.cpu().numpy(), ok.cpu().numpy())
        res[mode] = r
        del dec
        torch.cuda.empty_cache()
    same = all((a == b).all() for a, b in zip(hard["off"], hard["on"]))
    res["identical_results"] = bool(same)
    res["side_buffer_and_generation_bytes"] = res["on"]["device_bytes"] - res["off"]["device_bytes"]
    res["speedup_on_over_off"] = res["off"]["ms_per_step"] / res["on"]["ms_per_step"]
    res["workload"] = "N = %d, K = %d IRA (M = %d, E = %d), NMS 0.75, %s, parity VNs pinned, fp32, compressed check state, %d frames, <= %d sweeps; %d timed steps after %d warm-up" % (
        N, K, code.M, code.E, "QBER 2 % on every frame" if args.case == "flat" else "QBER per frame ~ U[2 %, 3 %] (rng seed 2)", F, args.n_ite, args.steps, args.warmup)
    if args.case == "flat" and F == 4096:
        p = PARENT_LAYERED_EARLY_EXIT
        res["parent_cross_check"] = dict(p, off_ms_per_step=res["off"]["ms_per_step"], off_over_parent=res["off"]["ms_per_step"] / p["ms_per_step"],
                                         note="compared with the recorded leg, not with a rebuilt parent: that figure is the mean of 5 steps of bench.py on another day and box, "
                                              "this one the median of %d; the non-compacting instances of the layer kernels are unchanged in VGPR / SGPR / scratch" % args.steps)
    return "%s_%d" % (args.case, F), res


def stream_case(args):
    exe = os.path.join(ROOT, "qcrypto-ldpc_amd", "host", "qldpc_stream")
    res = {}
    for mode in ("unset", "1"):
        env = dict(os.environ)
        env.pop("QLDPC_COMPACT", None)
        if mode == "1":
            env["QLDPC_COMPACT"] = "1"
        runs = []
        for flags in (["-b", "512", "-r", str(args.steps)], ["-b", "512", "-r", "1", "-p"]):      # timed; once more under the decoders' profile for the kernel split
            out = subprocess.run([exe] + flags, env=env, check=True, capture_output=True, text=True, timeout=500).stdout
            runs.append(json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1]))
        t, prof = runs
        res["QLDPC_COMPACT_" + mode] = dict(ms_mean=t["ms_mean"], ms_best=t["ms_best"], Mbit_s_mean=t["Mbit_s_mean"], reconciled=t["reconciled"], epochs=t["epochs"],
                                            avg_iterations=t["avg_iterations"], mean_iterations_per_rate=t["mean_iterations_per_rate"], max_iterations_per_rate=t["max_iterations_per_rate"],
                                            epochs_per_rate=t["epochs_per_rate"], kernels_profiled_run=prof.get("kernels"))
    a, b = res["QLDPC_COMPACT_unset"], res["QLDPC_COMPACT_1"]
    res["speedup_on_over_off"] = a["ms_mean"] / b["ms_mean"]
    res["workload"] = t["workload"] + "; mean of %d calls (the tool's own ms_mean), no median available from it" % args.steps
    res["parent_cross_check"] = dict(PARENT_CONFIG3_STREAM, unset_ms_mean=a["ms_mean"], unset_over_parent=a["ms_mean"] / PARENT_CONFIG3_STREAM["ms"])
    return "config3_stream", res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["flat", "mixed", "stream"], required=True)
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "layered_compact.json"))
    ap.add_argument("--n-ite", type=int, default=50)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    name, res = stream_case(args) if args.case == "stream" else decoder_case(args)
    out = {}
    if os.path.exists(args.out):
        out = json.load(open(args.out))
    out.setdefault("cases", {})[name] = res
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({name: res}))


if __name__ == "__main__":
    main()
