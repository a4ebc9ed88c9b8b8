#!/usr/bin/env python3
"""What the genie-aided polar code construction costs on the device, all legs in one process: hipEvent ms (median of 7 after a warm-up call) at
N = 2^10 x 20 000 frames and N = 2^16 x 4 096 frames in both message types of
  (a) decode   Polar.decode with every position frozen to the truth and no output asked for,
  (b) tally    Polar.tally into a row that exists,
  (c) leaf     the route without the tally kernel: Polar.decode with the leaf output, then the rule in torch on the device (the truth's bits
               are unpacked before the clock starts),
and (d) the wall clock of PolarMonteCarlo.construct beside PolarMonteCarlo.run over 10^6 frames of N = 2^10 on a BSC of QBER 0.05.  Then the
construction itself: the set of K = 512 from those 10^6 frames, and its FER beside the 5G set's over 10^5 held-out frames through run().
--polar-cost NAME=FILE (any number) copies the decode medians of tools/polar_cost.py outputs in, for builds to be put side by side.
Writes profiles/polar_construct_cost.json.

    python tools/polar_construct_cost.py [--out profiles/polar_construct_cost.json] [--runs 7] [--polar-cost parent=a.json --polar-cost head=b.json]
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
from polar_common import awgn_frames, event_ms  # noqa: E402

SHAPES = [(10, 20000, "i8"), (10, 20000, "f32"), (16, 4096, "i8"), (16, 4096, "f32")]
QBER, MC_FRAMES, HELD_OUT, MC_BATCH = 0.05, 1000000, 100000, 20000


def unpack_dev(torch, words, N):
    """int32 [F, W] packed MSB-first on the device -> bool [F, N]"""
    shifts = torch.arange(31, -1, -1, device=words.device, dtype=torch.int32)
    return (((words.unsqueeze(2) >> shifts) & 1) != 0).reshape(words.shape[0], -1)[:, :N]


def legs(q, torch, rng, n, F, messages, runs):
    N, W = 1 << n, (1 << n) // 32
    llr = awgn_frames(rng, n, F, messages)
    d_llr = torch.from_numpy(llr).cuda()
    d_u = torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31, (F, W)).astype(np.int32)).cuda()
    dec = q.Polar(n, [], messages, 31, max_frames=F)
    acc = torch.zeros((2, N), dtype=torch.int64, device="cuda")
    bits = unpack_dev(torch, d_u, N)

    def leaf_route():
        leaf = dec.decode(d_llr, d_u, leaf=True, want=())["leaf"]
        tie = leaf == 0
        acc[1] += tie.sum(dim=0)
        acc[0] += (~tie & ((leaf < 0) != bits)).sum(dim=0)

    row = {"log2_n": n, "frames": F, "messages": messages,
           "decode_ms": event_ms(torch, lambda: dec.decode(d_llr, d_u, want=()), runs),
           "tally_ms": event_ms(torch, lambda: dec.tally(d_llr, d_u, out=acc), runs)}
    acc.zero_()
    dec.tally(d_llr, d_u, out=acc)
    by_kernel = acc.clone()
    row["leaf_route_ms"] = event_ms(torch, leaf_route, runs)
    acc.zero_()
    leaf_route()
    row["routes_agree"] = bool(torch.equal(acc, by_kernel))
    Fh = min(F, 64)
    row["device_equals_mirror"] = bool(np.array_equal(dec.tally(d_llr[:Fh], d_u[:Fh]).cpu().numpy().view(np.uint64),
                                                      q.polar_tally_host(n, llr[:Fh], d_u[:Fh].cpu().numpy().view(np.uint32), messages, 31)))
    return row


def loop(q, torch):
    """construct beside run over MC_FRAMES frames, then the constructed set of K = 512 beside the 5G set on HELD_OUT frames of another seed"""
    import polar_ref as R
    n, N, K = 10, 1024, 512
    t = int(np.floor(QBER * 4294967296.0))
    mag = np.float32(np.log((1.0 - QBER) / QBER))
    table = ([(1 << 32) - t], [t], [mag, -mag])
    nr = np.sort(R.nr_order(N)[N - K:]).astype(np.int32)

    def mc_of(pos, seed):
        dec = q.Polar(n, pos, "f32", 31, max_frames=MC_BATCH)
        mc = q.PolarMonteCarlo(dec, seed, 0, 16, "random")
        mc.set_channel(*table)
        return mc

    mc = mc_of(nr, 1)
    mc.construct(0, MC_BATCH)
    mc.run(0, MC_BATCH)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = mc.construct(0, MC_FRAMES)
    t1 = time.perf_counter()
    run = mc.run(0, MC_FRAMES)
    t2 = time.perf_counter()
    out = {"log2_n": n, "frames": MC_FRAMES, "batch": MC_BATCH, "qber": QBER, "messages": "f32",
           "construct_wall_ms": (t1 - t0) * 1e3, "run_wall_ms": (t2 - t1) * 1e3,
           "construct_stage_ms": {k: got[k] for k in q.POLAR_MC_MS}, "run_stage_ms": {k: run[k] for k in q.POLAR_MC_MS}}
    order = q.polar_construct_order(got["wrong"], got["ties"], q.polar_pw_order(n))
    built = np.sort(order[N - K:]).astype(np.int32)
    out["construction"] = {"train_seed": 1, "train_frames": MC_FRAMES, "K": K, "positions_not_in_the_5g_set": int(len(set(built.tolist()) - set(nr.tolist()))),
                           "score_sum_of_the_set": int((2 * got["wrong"] + got["ties"])[built].sum()),
                           "union_bound_on_fer": float((2 * got["wrong"] + got["ties"])[built].sum() / (2.0 * MC_FRAMES)),
                           "k_at_union_bound_1e-2": q.polar_construct_k(got["wrong"], got["ties"], order, MC_FRAMES, 1e-2)}
    for name, pos in (("constructed", built), ("5g", nr)):
        res = mc_of(pos, 3).run(0, HELD_OUT)
        out["construction"]["held_out_%s" % name] = {"seed": 3, "frames": res["frames"], "frame_errors": res["frame_errors"]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "polar_construct_cost.json"))
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--polar-cost", action="append", default=[], metavar="NAME=FILE")
    args = ap.parse_args()
    import torch
    q = _qldpc_loader.load()
    rng = np.random.default_rng(1)
    res = {"what": "hipEvent ms, median of %d after a warm-up call, one process: decode (all frozen, no outputs), tally, and decode with leaf + the "
                   "rule in torch; wall ms of construct and run over 10^6 frames; the constructed K = 512 set beside the 5G set" % args.runs,
           "shapes": {}}
    for n, F, messages in SHAPES:
        row = legs(q, torch, rng, n, F, messages, args.runs)
        res["shapes"]["n=%d x %d %s" % (n, F, messages)] = row
        print(n, F, messages, row["decode_ms"]["median"], row["tally_ms"]["median"], row["leaf_route_ms"]["median"], row["routes_agree"],
              row["device_equals_mirror"], flush=True)
        torch.cuda.empty_cache()
    res["loop"] = loop(q, torch)
    print(json.dumps(res["loop"]), flush=True)
    if args.polar_cost:
        side = res["existing_decoder_polar_cost_decode_dev_ms"] = {}
        for item in args.polar_cost:
            name, path = item.split("=", 1)
            for shape, row in json.load(open(path))["shapes"].items():
                side.setdefault(shape, {})[name] = row["decode_dev_ms"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
