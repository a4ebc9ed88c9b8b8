#!/usr/bin/env python3
"""What a call of the polar subsystem costs on the device: hipEvent time of one qldpc_polar_decode_dev and one qldpc_polar_encode_dev call (median of
7 after a warm-up call) at N = 2^10 x 20 000 frames in both message types and at N = 2^16 x 4 096 frames, beside the host mirror on the same frames
(one thread, a subset of the frames scaled up where the whole batch would take minutes).  Writes profiles/polar_cost.json.

    python tools/polar_cost.py [--out profiles/polar_cost.json] [--runs 7]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _qldpc_loader  # noqa: E402
from polar_common import awgn_frames, event_ms  # noqa: E402

SHAPES = [(10, 20000, "i8"), (10, 20000, "f32"), (16, 4096, "i8")]
HOST_FRAMES = {10: 2000, 16: 32}      # frames the host mirror is timed on


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "polar_cost.json"))
    ap.add_argument("--runs", type=int, default=7)
    args = ap.parse_args()
    import torch
    q = _qldpc_loader.load()
    rng = np.random.default_rng(1)
    res = {"what": "hipEvent ms of one decode_dev (u, info and x asked for) and one encode_dev call, median of %d; host mirror: one thread, "
                   "timed on host_frames frames and scaled to the batch" % args.runs, "shapes": {}}
    for n, F, messages in SHAPES:
        N, W = 1 << n, (1 << n) // 32
        pos = np.sort(q.polar_pw_order(n)[N // 2:]).astype(np.int32)
        llr = awgn_frames(rng, n, F, messages)
        dec = q.Polar(n, pos, messages, 31, max_frames=F)
        d_llr = torch.from_numpy(llr).cuda()
        d_u = torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31, (F, W)).astype(np.int32)).cuda()
        d_x = torch.empty_like(d_u)
        row = {"log2_n": n, "frames": F, "messages": messages, "n_info": int(pos.size), "device_bytes": dec.device_bytes(),
               "decode_dev_ms": event_ms(torch, lambda: dec.decode(d_llr), args.runs),
               "encode_dev_ms": event_ms(torch, lambda: dec.encode(d_u, out=d_x), args.runs)}
        row["decode_frames_per_s"] = F / (row["decode_dev_ms"]["median"] * 1e-3)
        row["f_g_steps_per_s"] = row["decode_frames_per_s"] * N * n
        Fh = min(F, HOST_FRAMES[n])
        t = time.perf_counter()
        host = q.polar_decode_host(n, pos, llr[:Fh], None, messages, 31)
        t_dec = time.perf_counter() - t
        u_host = d_u[:Fh].cpu().numpy().view(np.uint32)
        t = time.perf_counter()
        q.polar_encode_host(n, u_host)
        t_enc = time.perf_counter() - t
        row["host_frames"] = Fh
        row["decode_host_ms"] = t_dec * 1e3 * F / Fh
        row["encode_host_ms"] = t_enc * 1e3 * F / Fh
        got = dec.decode(d_llr[:Fh])
        row["device_equals_mirror"] = bool(all(np.array_equal(got[k].cpu().numpy().view(np.uint32), host[k]) for k in ("u", "info", "x")))
        res["shapes"]["n=%d x %d %s" % (n, F, messages)] = row
        print(json.dumps({k: row[k] for k in ("log2_n", "frames", "messages", "decode_host_ms", "encode_host_ms", "device_equals_mirror")}),
              row["decode_dev_ms"]["median"], row["encode_dev_ms"]["median"], flush=True)
        del dec, d_llr, d_u, d_x
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
