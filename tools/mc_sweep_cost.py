#!/usr/bin/env python3
"""What the device-resident QBER sweep (qldpc_mc_sweep) costs and gives against one qldpc_mc_run per point, on the headline code (N = 65 536,
K = 52 429, flooding NMS 0.75, <= 50 iterations with the early exit, batches of 4 096 frames, chunks of 64 frames = 64 slots per round):

    timeout -k 10 900 python tools/mc_sweep_cost.py --out profiles/mc_sweep_cost.json

sweep:  one sweep of --points QBER points (evenly spaced over --qber lo:hi) with --max-frames and --max-fe per point: wall time, rounds, frames, the
        hipEvent time of every stage per round, and the lane occupancy of every round (frame slots dealt / batch), replayed on the host with
        mc_sweep_deal from the failed frames of the runs below.
runs:   the host loop the sweep replaces, one qldpc_mc_run per point with the same max_frames and max_fe (batch-granular stop): wall time,
        batches and frames.
same:   one qldpc_mc_run per point over exactly the frames_q frames the sweep gave the point (the same frames, no stop rule): wall time and
        batches; its counters must equal the sweep's rows, which the tool asserts.
No threshold and no claim: the file is the measurement.

--tables: the sweep over points of a table channel (qldpc_mc_sweep_tables) instead, on the reference's fixed-point AWGN experiment (NR_2_6_52, first
2 z VNs punctured, all-zero codeword, layered 8-bit OMS offset 2, 20 iterations): ONE MonteCarlo.sweep_awgn over the four published Eb/N0 points
against four set_awgn + run calls over the same --max-frames frames in the same process, both on the host's clock (the four calls include their
table uploads and stream syncs, which is what a caller pays), with the sweep's per-round stage times; the rows must be equal, which the tool
asserts.  Writes profiles/mc_sweep_tables_cost.json.

    timeout -k 10 600 python tools/mc_sweep_cost.py --tables
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, K, BATCH, N_ITE, CHUNK = 65536, 52429, 4096, 50, 64
SWEEP_STAGES = ("source_ms", "encode_ms", "channel_ms", "load_ms", "erase_ms", "decode_ms", "monitor_ms")
ROW = ("frames", "frame_errors", "bit_errors", "undetected", "not_converged", "iter_sum", "iter_max", "channel_flips", "channel_bits")


def occupancy(q, fails, frames, max_frames, max_fe):
    """frame slots dealt per round / batch: the sweep's schedule replayed with the host mirror of its deal over the failed frames of each point"""
    P, S = len(fails), BATCH // CHUNK
    done, fe, out = np.zeros(P, np.uint64), np.zeros(P, np.uint64), []
    while True:
        give = q.mc_sweep_deal(done, fe, CHUNK, S, max_frames, max_fe)
        if give.sum() == 0:
            break
        n = np.minimum(give.astype(np.int64) * CHUNK, max_frames - done.astype(np.int64))
        out.append(float(n.sum()) / BATCH)
        for p in np.nonzero(give)[0]:
            fe[p] += np.uint64(((fails[p] >= done[p]) & (fails[p] < done[p] + np.uint64(n[p]))).sum())
            done[p] += np.uint64(n[p])
    assert (done == frames).all(), (done, frames)
    return out


def measure(q, qbers, max_frames, max_fe):
    code = q.Code.ira(N, K)
    enc = q.Encoder(code, "IRA")
    dec = q.Decoder(code, enc.K, N_ITE, info_bits_pos=enc.info_bits_pos, rule="NMS", rule_param=0.75, n_frames=BATCH)
    mc = q.MonteCarlo(dec, enc, seed=1, batch=BATCH, fail_cap=max_frames)
    mc.sweep(qbers[:1], max_frames=BATCH, chunk=CHUNK)                                      # warm-up: first launches, allocations
    mc.run(qbers[0], 0, BATCH)
    w = mc.sweep(qbers, max_frames=max_frames, max_frame_errors=max_fe, chunk=CHUNK)
    pts = w["points"]
    runs = [mc.run(qb, 0, max_frames, max_fe) for qb in qbers]
    same, fails = [], []
    for i, qb in enumerate(qbers):
        r = mc.run(qb, 0, int(pts["frames"][i]))
        assert all(int(r[k]) == int(pts[k][i]) for k in ROW), (i, r, pts[i])
        same.append(r)
        fails.append(mc.failed_frames())
    occ = occupancy(q, fails, pts["frames"], max_frames, max_fe)
    assert len(occ) == w["rounds"]
    return dict(workload="N %d K %d flooding NMS 0.75, <= %d iterations, early exit, batch %d, chunk %d, %d points QBER %.4f .. %.4f, max_frames %d, max_fe %d"
                         % (N, enc.K, N_ITE, BATCH, CHUNK, len(qbers), qbers[0], qbers[-1], max_frames, max_fe),
                sweep=dict(total_ms=w["total_ms"], rounds=w["rounds"], frames=w["frames"], per_round_ms={k: w[k] / w["rounds"] for k in SWEEP_STAGES},
                           occupancy_per_round=occ, mean_occupancy=float(np.mean(occ)), frames_per_point=[int(x) for x in pts["frames"]],
                           frame_errors_per_point=[int(x) for x in pts["frame_errors"]], closed_by=[int(x) for x in pts["closed_by"]]),
                runs=dict(total_ms=sum(r["total_ms"] for r in runs), batches=sum(r["batches"] for r in runs), frames=sum(r["frames"] for r in runs),
                          decode_ms=sum(r["decode_ms"] for r in runs), frames_per_point=[int(r["frames"]) for r in runs]),
                same=dict(total_ms=sum(r["total_ms"] for r in same), batches=sum(r["batches"] for r in same), frames=sum(r["frames"] for r in same),
                          decode_ms=sum(r["decode_ms"] for r in same)),
                device_bytes=mc.device_bytes)


def measure_tables(q, frames, reps):
    pins = json.load(open(os.path.join(ROOT, "tests", "golden", "matlab_fp_fer.json")))["NR_2_6_52"]
    code = q.Code.from_qc(os.path.join(ROOT, "tests", "golden", pins["qc"]))
    enc = q.Encoder(code, "QC")
    cls = np.zeros(code.N, np.uint8)
    cls[:2 * pins["z"]] = q.VN_PUNCTURED
    rate, ebno = enc.K / (code.N - 2 * pins["z"]), [row[0] for row in pins["rows"]]
    dec = q.Decoder(code, enc.K, 20, info_bits_pos=enc.info_bits_pos, rule="OMS", rule_param=2.0, n_frames=frames, schedule="hlayered", enable_syndrome=False,
                    msg_dtype="i8", quant_scale=1.0)
    mc = q.MonteCarlo(dec, enc, vn_class=cls, seed=1)
    mc.set_source("zero")
    mc.sweep_awgn(ebno[:1], rate, max_frames=frames)                                       # warm-up: first launches, allocations
    mc.set_awgn(ebno_db=ebno[0], rate=rate)
    mc.run(0.1, 0, frames)
    sweeps, calls = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        w = mc.sweep_awgn(ebno, rate, max_frames=frames)
        sweeps.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        runs = []
        for e in ebno:
            mc.set_awgn(ebno_db=e, rate=rate)
            runs.append(mc.run(0.1, 0, frames))
        calls.append((time.perf_counter() - t0) * 1e3)
        for i, r in enumerate(runs):
            assert all(int(r[k]) == int(w["points"][k][i]) for k in ROW), (i, r, w["points"][i])
    return dict(workload="NR_2_6_52 N %d K %d, first %d VNs punctured, all-zero codeword, layered 8-bit OMS offset 2, 20 iterations, batch %d, Eb/N0 %s dB, "
                         "%d frames per point, %d repetitions" % (code.N, enc.K, 2 * pins["z"], frames, ebno, frames, reps),
                sweep=dict(wall_ms=sweeps, median_wall_ms=float(np.median(sweeps)), rounds=w["rounds"], frames=w["frames"],
                           per_round_ms={k: w[k] / w["rounds"] for k in SWEEP_STAGES}, frame_errors_per_point=[int(x) for x in w["points"]["frame_errors"]]),
                calls=dict(wall_ms=calls, median_wall_ms=float(np.median(calls)), batches=sum(r["batches"] for r in runs), frames=sum(r["frames"] for r in runs),
                           decode_ms=sum(r["decode_ms"] for r in runs), channel_ms=sum(r["channel_ms"] for r in runs)),
                calls_over_sweep=float(np.median(calls) / np.median(sweeps)), device_bytes=mc.device_bytes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mc_sweep_cost.json"))
    ap.add_argument("--points", type=int, default=8)
    ap.add_argument("--qber", default="0.02:0.034")
    ap.add_argument("--max-frames", type=int, default=4 * BATCH)
    ap.add_argument("--max-fe", type=int, default=100)
    ap.add_argument("--tables", action="store_true", help="the table-channel leg: sweep_awgn over the published points against set_awgn + run per point")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    lo, hi = (float(x) for x in args.qber.split(":"))
    import _qldpc_loader
    if args.tables:
        out = measure_tables(_qldpc_loader.load(), 20000 if args.max_frames == 4 * BATCH else args.max_frames, args.reps)
        out["what"] = ("the sweep over points of a table channel on the reference's fixed-point AWGN experiment: one sweep_awgn over the four published Eb/N0 "
                       "points against four set_awgn + run calls over the same frames, wall times on the host's clock, and the sweep's per-round stage times")
        path = args.out if args.out != ap.get_default("out") else os.path.join(ROOT, "profiles", "mc_sweep_tables_cost.json")
        with open(path, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")
        print(json.dumps(out))
        return
    out = measure(_qldpc_loader.load(), [float(x) for x in np.linspace(lo, hi, args.points)], args.max_frames, args.max_fe)
    out["what"] = ("the device-resident QBER sweep on the headline code: one sweep of P points against P calls of qldpc_mc_run (with the same stop rule, and over "
                   "exactly the sweep's frames), the sweep's per-round stage times by hipEvents and its lane occupancy per round")
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
