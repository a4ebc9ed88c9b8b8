#!/usr/bin/env python3
"""What a Monte-Carlo point of the polar decoders costs on the device, beside the host-fed route it replaces, at the published shapes: N = 2^10 x
20 000 frames, SC with int8 messages (3 dB, K = 512) and list 4 with CRC 11 (2.25 dB, A = 500).

    loop      one PolarMonteCarlo.run of the 20 000 frames as one batch: the hipEvent times of its stages and the wall time of the call, median of
              --runs after a warm-up run
    host-fed  in the same process, what tests/polar_ref.py::fer_point and tests/polar_list_ref.py::list_point do per point, each step timed by the
              wall clock around a synchronize: numpy generation (messages, CRC, encode, normals, quantisation), upload, decode, download, compare

Writes profiles/polar_mc_cost.json.  No threshold is set on the ratio: it is reported.

    python tools/polar_mc_cost.py [--out profiles/polar_mc_cost.json] [--runs 7]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _qldpc_loader  # noqa: E402
import polar_list_ref as LR  # noqa: E402
import polar_mc_ref as M  # noqa: E402
import polar_ref as R  # noqa: E402

FRAMES = 20000
STAGES = ("source_ms", "encode_ms", "channel_ms", "decode_ms", "monitor_ms", "total_ms")


def median_of(rows):
    return {k: float(np.median([r[k] for r in rows])) for k in rows[0]}


def host_fed(torch, q, dec, pos, A, crc, sigma, rmax, maxqr, rounding, rng):
    """one point the host-fed way -> the wall ms of every step, and the block errors"""
    N, t = dec.N, {}
    clock = time.perf_counter
    t0 = clock()
    msg = rng.integers(0, 2, (FRAMES, A), dtype=np.uint8)
    word = np.concatenate([msg, LR.crc_word(LR.crc_bits(msg, *crc), crc[0])], axis=1) if crc[0] else msg
    u = np.zeros((FRAMES, N), np.uint8)
    u[:, pos] = word
    r = (1.0 - 2.0 * R.encode(u)) + sigma * rng.standard_normal((FRAMES, N))
    if rounding == "floor":
        rq = np.clip(np.floor(r / rmax * maxqr), -(maxqr + 1), maxqr).astype(np.int8)
    else:
        rq = np.round(np.clip(r, -rmax, rmax) / rmax * maxqr).astype(np.int8)
    t["generate_ms"] = (clock() - t0) * 1e3
    t0 = clock()
    d_rq = torch.from_numpy(rq).cuda()
    torch.cuda.synchronize()
    t["upload_ms"] = (clock() - t0) * 1e3
    t0 = clock()
    out = dec.decode(d_rq, want=("info",))["info"]
    torch.cuda.synchronize()
    t["decode_ms"] = (clock() - t0) * 1e3
    t0 = clock()
    info = out.cpu().numpy().view(np.uint32)
    t["download_ms"] = (clock() - t0) * 1e3
    t0 = clock()
    errors = int((R.unpack(info, len(pos))[:, :A] != msg).any(axis=1).sum())
    t["compare_ms"] = (clock() - t0) * 1e3
    t["total_ms"] = sum(t.values())
    return t, errors


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "polar_mc_cost.json"))
    ap.add_argument("--runs", type=int, default=7)
    args = ap.parse_args()
    import torch
    q = _qldpc_loader.load()
    pub = R.published()
    res = {"what": "N = 1024 x %d frames.  loop: hipEvent ms of the stages of one PolarMonteCarlo.run (one batch) and the wall ms of the call; host_fed: wall ms of "
                   "numpy generation, upload, decode, download and compare in the same process; medians of %d after a warm-up" % (FRAMES, args.runs), "points": {}}
    points = [("sc_i8_3dB", None, M.sc_point(q, 4), "floor", pub["rmax"]), ("list4_crc11_2.25dB", 4, M.list_point(q, 3), "round", pub["res3"]["rmax"])]
    for name, L, (row, pos, tab, _), rounding, rmax in points:
        crc = LR.CRC11 if L else (0, 0)
        A = len(pos) - crc[0]
        sigma = float(np.sqrt(1.0 / (2.0 * (A / 1024) * 10.0 ** (row[0] / 10.0))))
        dec = q.PolarList(10, pos, "i8", 31, L, *crc, max_frames=FRAMES) if L else q.Polar(10, pos, "i8", 31, max_frames=FRAMES)
        mc = q.PolarMonteCarlo(dec, M.MC_SEED)
        mc.set_channel(*tab)
        first = mc.run(0, FRAMES)
        loop = [mc.run(0, FRAMES) for _ in range(args.runs)]
        rng = np.random.default_rng(1)
        host_fed(torch, q, dec, pos, A, crc, sigma, rmax, pub["maxqr"], rounding, rng)
        fed = [host_fed(torch, q, dec, pos, A, crc, sigma, rmax, pub["maxqr"], rounding, rng) for _ in range(args.runs)]
        out = {"ebno_db": row[0], "published_fer": row[1], "frames": FRAMES, "list_size": L or 0, "crc_len": crc[0], "device_bytes_decoder": dec.device_bytes(),
               "device_bytes_loop": mc.device_bytes(), "loop": median_of([{k: r[k] for k in STAGES} for r in loop]),
               "loop_frame_errors": first["frame_errors"], "loop_same_every_run": bool(all(r["frame_errors"] == first["frame_errors"] for r in loop)),
               "host_fed": median_of([t for t, _ in fed]), "host_fed_frame_errors": [e for _, e in fed]}
        out["host_fed_over_loop"] = out["host_fed"]["total_ms"] / out["loop"]["total_ms"]
        out["decode_share_of_loop"] = out["loop"]["decode_ms"] / out["loop"]["total_ms"]
        res["points"][name] = out
        print(name, json.dumps(out["loop"]), json.dumps(out["host_fed"]), "ratio %.1f" % out["host_fed_over_loop"], flush=True)
        del mc, dec
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
