#!/usr/bin/env python3
"""What a call of the polar list decoder costs on the device: hipEvent time of one qldpc_polar_list_decode_dev call (median of 7 after a warm-up call,
every output asked for) at N = 2^10 x 20 000 frames with list sizes 1, 2, 4 and 8 in both message types, beside one qldpc_polar_decode_dev call on
the same frames in the same process, and at N = 2^14 x 4 096 frames with list size 4.  Writes profiles/polar_list_cost.json.

    python tools/polar_list_cost.py [--out profiles/polar_list_cost.json] [--runs 7]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _qldpc_loader  # noqa: E402
from polar_common import awgn_frames, event_ms  # noqa: E402

SHAPES = [(10, 20000, "i8", (1, 2, 4, 8)), (10, 20000, "f32", (1, 2, 4, 8)), (14, 4096, "i8", (4,))]
CRC11 = (11, 0x621)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "polar_list_cost.json"))
    ap.add_argument("--runs", type=int, default=7)
    args = ap.parse_args()
    import torch
    q = _qldpc_loader.load()
    rng = np.random.default_rng(1)
    res = {"what": "hipEvent ms of one PolarList.decode call (all outputs, CRC 11) and of one Polar.decode call (u, info, x) on the same frames, "
                   "median of %d; ratio = list / SC" % args.runs, "shapes": {}}
    for n, F, messages, lists in SHAPES:
        N = 1 << n
        pos = np.sort(q.polar_pw_order(n)[N // 2:]).astype(np.int32)
        llr = awgn_frames(rng, n, F, messages)
        d_llr = torch.from_numpy(llr).cuda()
        sc = q.Polar(n, pos, messages, 31, max_frames=F)
        sc_ms = event_ms(torch, lambda: sc.decode(d_llr), args.runs)
        sc_x = sc.decode(d_llr, want=("x",))["x"].cpu().numpy()
        del sc
        for L in lists:
            dec = q.PolarList(n, pos, messages, 31, L, *CRC11, max_frames=F)
            row = {"log2_n": n, "frames": F, "messages": messages, "n_info": int(pos.size), "list_size": L, "device_bytes": dec.device_bytes(),
                   "sc_decode_dev_ms": sc_ms, "list_decode_dev_ms": event_ms(torch, lambda: dec.decode(d_llr), args.runs)}
            row["ratio_to_sc"] = row["list_decode_dev_ms"]["median"] / sc_ms["median"]
            row["frames_per_s"] = F / (row["list_decode_dev_ms"]["median"] * 1e-3)
            if L == 1:                                             # a list of one without a CRC is the SC decoder
                one = q.PolarList(n, pos, messages, 31, 1, max_frames=F)
                row["list_of_one_equals_sc"] = bool(np.array_equal(one.decode(d_llr, want=("x",))["x"].cpu().numpy(), sc_x))
                del one
            Fh = min(F, 256)
            host = q.polar_list_decode_host(n, pos, llr[:Fh], None, None, messages, 31, L, *CRC11)
            got = dec.decode(d_llr[:Fh])
            row["device_equals_mirror"] = bool(all(np.array_equal(got[k].cpu().numpy().view(np.uint32), host[k].view(np.uint32)) for k in host))
            res["shapes"]["n=%d x %d %s L=%d" % (n, F, messages, L)] = row
            print(json.dumps({k: row[k] for k in ("log2_n", "frames", "messages", "list_size", "ratio_to_sc", "device_equals_mirror")}),
                  row["list_decode_dev_ms"]["median"], sc_ms["median"], flush=True)
            del dec
        del d_llr
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
