#!/usr/bin/env python3
"""What a decoder gang (qldpc.h "decoder gangs") gives or costs against decoders side by side on their own streams.  One process per case; every
run merges its case into the output file:

    timeout -k 10 900 python tools/gang_cost.py --case decoders --out profiles/gang_cost.json && \
    timeout -k 10 900 python tools/gang_cost.py --case stream   --out profiles/gang_cost.json

  decoders  the four mother codes of BASELINE config 3 (rates 0.5 / 0.7 / 0.8 / 0.9, PEG depth 2, K = 57 344), 128 frames each at a QBER inside the
            rate's range, NMS 0.75 with the per-sweep early exit, run three ways on the same frames in the same process: one after another; side by
            side on four streams from four host threads (the sessions' shape today); as one gang.  Per way: ms per step (median), layer launches
            and sweeps, and that the three give the same decisions.
  stream    BASELINE config 3 through host/qldpc_stream (512 epochs, sessions sized for 512 blocks) with QLDPC_RECON_GANG unset / 1, and one
            rocprofv3 --kernel-trace --stats run of each: count and mean duration of the layer kernels (every GPU step under its own time limit).

No threshold is set here: the gang stays opt-in whatever comes out.  The stream is compared with the unset run of the same binary and with the
parent's recorded 13.2 ms (profiles/r03_config3_stream_layered.json, tools/README.md).
"""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PARENT_CONFIG3_STREAM = dict(source="profiles/r03_config3_stream_layered.json / tools/README.md (qldpc_stream -b 512 -r 5 from C at the parent commit)", ms=13.2)
RATES = ((0.5, 0.08), (0.7, 0.04), (0.8, 0.018), (0.9, 0.006))      # mother rate, QBER of its frames (inside the rate's range at efficiency 1.4)


def decoders_case(args):
    import torch

    import _qldpc_loader
    q = _qldpc_loader.load()
    K, F = 57344, args.frames
    rng = np.random.default_rng(3)
    members = []
    for R, p in RATES:
        M = int(round(K * (1.0 - R) / R))
        N = K + M
        code = q.Code.ira_peg(N, K, 0.125, 11, 3, 2, 7)
        enc = q.Encoder(code, "IRA")
        info = rng.integers(0, 2, (F, K)).astype(np.uint8)
        cw = enc.encode_packed(torch.from_numpy(q.pack_bits(info).view(np.int32)).cuda())
        noise = np.zeros((F, N), np.uint8)
        noise[:, :K] = rng.random((F, K), dtype=np.float32) < np.float32(p)      # flips on the key VNs; the parity bits are disclosed exactly
        rx = cw ^ torch.from_numpy(q.pack_bits(noise).view(np.int32)).cuda()
        mag = torch.full((F,), float(q.bsc_llr(p)), dtype=torch.float32, device="cuda")
        cls = np.zeros(N, np.uint8)
        cls[K:] = q.VN_PINNED
        members.append(dict(R=R, p=p, code=code, K=K, N=N, rx=rx, mag=mag, cls=torch.from_numpy(cls).cuda()))

    def decoders():
        return [q.Decoder(m["code"], m["K"], args.n_ite, rule="NMS", rule_param=0.75, enable_syndrome=True, n_frames=F, schedule="hlayered") for m in members]

    def load(d, m):
        d.load_bits(m["rx"], m["mag"], m["cls"])

    def timed(step):
        for _ in range(args.warmup):
            step()
        dts = []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            step()
            dts.append(time.perf_counter() - t0)
        return dict(ms_per_step=statistics.median(dts) * 1e3, ms_min=min(dts) * 1e3, ms_max=max(dts) * 1e3)

    def layer_stats(decs, step):
        for d in decs:
            d.profile(True)
            d.profile_clear()
        step()
        out = {}
        for d in decs:
            for s in d.profile_read():
                if s["name"].startswith("layer_update"):
                    o = out.setdefault(s["name"], dict(sweeps=0, total_ms=0.0))
                    o["sweeps"] += s["launches"]
                    o["total_ms"] += s["total_ms"]
            d.profile(False)
        return out

    def results(decs):
        out = []
        for d in decs:
            it, ok = d.fetch_status()
            out.append((d.fetch_packed().cpu().numpy(), it.cpu().numpy(), ok.cpu().numpy()))
        return out

    res, hard = {}, {}
    plan = q.gang_plan([m["code"] for m in members], ["NMS"] * 4, [1] * 4)

    # one after another, on one stream
    decs = decoders()

    def sequential():
        for d, m in zip(decs, members):
            load(d, m)
            d.run()
        for d in decs:
            d.sync()
    res["sequential"] = timed(sequential)
    res["sequential"]["layer"] = layer_stats(decs, sequential)
    hard["sequential"] = results(decs)
    sweeps = [int(d.last_run_iterations) for d in decs]
    res["sequential"]["sweeps_per_member"] = sweeps
    res["sequential"]["layer_launches"] = sum(s * q.gang_plan([m["code"]], ["NMS"], [1])["launches_per_sweep"] for s, m in zip(sweeps, members))

    # side by side: four streams, four host threads (what a session does today)
    streams = [torch.cuda.Stream() for _ in members]
    for d, s in zip(decs, streams):
        d.set_stream(s)

    def one(d, m):
        load(d, m)
        d.run()
        d.sync()

    def side_by_side():
        th = [threading.Thread(target=one, args=(d, m)) for d, m in zip(decs, members)]
        for t in th:
            t.start()
        for t in th:
            t.join()
    torch.cuda.synchronize()
    res["four_streams"] = timed(side_by_side)
    res["four_streams"]["layer"] = layer_stats(decs, side_by_side)
    res["four_streams"]["layer_launches"] = res["sequential"]["layer_launches"]
    hard["four_streams"] = results(decs)
    del decs

    # one gang
    decs = decoders()
    gang = q.DecoderGang(decs)

    def ganged():
        for d, m in zip(decs, members):
            load(d, m)
        gang.run()
        decs[0].sync()
    res["gang"] = timed(ganged)
    st = gang.last_run_stats()
    res["gang"].update(sweeps=st["sweeps"], layer_launches=st["launches"], solo_layer_launches=st["solo_launches"], members_dropped=st["dropped"])
    res["gang"]["layer"] = layer_stats(decs, ganged)
    hard["gang"] = results(decs)

    res["identical_results"] = bool(all(all((a == b).all() for a, b in zip(x, y)) for w in ("four_streams", "gang") for x, y in zip(hard["sequential"], hard[w])))
    res["plan"] = plan
    res["gang_over_four_streams"] = res["four_streams"]["ms_per_step"] / res["gang"]["ms_per_step"]
    res["gang_over_sequential"] = res["sequential"]["ms_per_step"] / res["gang"]["ms_per_step"]
    res["workload"] = "config-3 mother codes (K = %d, rates %s, PEG depth 2), QBER %s, %d frames each, NMS 0.75, <= %d sweeps, early exit; median of %d steps after %d warm-up (load + run + sync)" % (
        K, [r for r, _ in RATES], [p for _, p in RATES], F, args.n_ite, args.steps, args.warmup)
    return "decoders", res


def layer_kernels(stats_csv):
    """count and mean duration of the layer kernels of a rocprofv3 --stats run"""
    out = {}
    with open(stats_csv) as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            if "qk_cn_layer" not in name:
                continue
            kind = "gang" if "_gang" in name else "solo"
            o = out.setdefault(kind, dict(calls=0, total_ns=0.0))
            o["calls"] += int(row["Calls"])
            o["total_ns"] += float(row["TotalDurationNs"])
    for o in out.values():
        o["mean_us"] = o["total_ns"] / max(1, o["calls"]) / 1e3
    return out


def stream_case(args):
    exe = os.path.join(ROOT, "qcrypto-ldpc_amd", "host", "qldpc_stream")
    res = {}
    for mode in ("unset", "1"):
        env = dict(os.environ)
        env.pop("QLDPC_RECON_GANG", None)
        if mode == "1":
            env["QLDPC_RECON_GANG"] = "1"
        out = subprocess.run(["timeout", "-k", "10", "300", exe, "-b", "512", "-r", str(args.steps)], env=env, check=True, capture_output=True, text=True).stdout
        t = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])
        r = dict(ms_mean=t["ms_mean"], ms_best=t["ms_best"], Mbit_s_mean=t["Mbit_s_mean"], reconciled=t["reconciled"], epochs=t["epochs"], avg_iterations=t["avg_iterations"],
                 epochs_per_rate=t.get("epochs_per_rate"))
        out = subprocess.run(["timeout", "-k", "10", "300", exe, "-b", "512", "-r", "1", "-p"], env=env, check=True, capture_output=True, text=True).stdout
        r["kernels_profiled_run"] = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1]).get("kernels")
        if shutil.which("rocprofv3"):
            tmp = tempfile.mkdtemp(prefix="gang_cost_")
            try:
                subprocess.run(["timeout", "-k", "10", "300", "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", exe, "-b", "512", "-r", "1"],
                               env=env, check=True, capture_output=True, text=True)
                found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
                r["layer_kernels_one_call_and_warmup"] = layer_kernels(found[0]) if found else None
            finally:
                shutil.rmtree(tmp, ignore_errors=True)
        res["QLDPC_RECON_GANG_" + mode] = r
    a, b = res["QLDPC_RECON_GANG_unset"], res["QLDPC_RECON_GANG_1"]
    res["gang_over_unset"] = a["ms_mean"] / b["ms_mean"]
    res["workload"] = t["workload"] + "; mean of %d calls (the tool's own ms_mean)" % args.steps
    res["parent_cross_check"] = dict(PARENT_CONFIG3_STREAM, unset_ms_mean=a["ms_mean"], unset_over_parent=a["ms_mean"] / PARENT_CONFIG3_STREAM["ms"])
    return "config3_stream", res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=["decoders", "stream"], required=True)
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gang_cost.json"))
    ap.add_argument("--n-ite", type=int, default=50)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    name, res = stream_case(args) if args.case == "stream" else decoders_case(args)
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
