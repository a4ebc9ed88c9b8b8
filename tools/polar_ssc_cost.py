#!/usr/bin/env python3
"""What the SSC rule saves on the device: hipEvent time of one qldpc_polar_decode_dev call (median of 7 after a warm-up call) on an SC and on an
SSC context of the same code in one process, alternating, at the shapes of tools/polar_cost.py (N = 2^10 x 20 000 frames in both message types,
N = 2^16 x 4 096 frames int8) on the polarization-weight half-rate code and, at 2^10, on the 5G set.  Each shape also in the reconciliation
call's form: x alone asked for, with a frozen row.  Beside each time, the plan of the code: its steps by kind and the share of the f/g element
steps and of the leaf blocks it keeps (counted from the plan; a mixed block's five inner levels counted in full), and whether device and mirror
agree on the timed frames.  Writes profiles/polar_ssc_cost.json (the committed file also holds, under polar_cost_parent_head, the runs of
tools/polar_cost.py on the parent commit's build and on this one in the same session).

    python tools/polar_ssc_cost.py [--out profiles/polar_ssc_cost.json] [--runs 7]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _qldpc_loader  # noqa: E402
from polar_common import awgn_frames, event_ms  # noqa: E402

SHAPES = [(10, 20000, "i8", "pw"), (10, 20000, "f32", "pw"), (10, 20000, "i8", "5g"), (10, 20000, "f32", "5g"), (16, 4096, "i8", "pw")]
HOST_FRAMES = {10: 2000, 16: 32}      # frames the mirrors are compared on


def plan_stats(n, steps):
    """the steps by kind, and the f/g element steps and leaf blocks the plan keeps of SC's N log2 N and N / 32"""
    N, kinds, fg = 1 << n, [0, 0, 0], 0
    for j, lam, kind in np.asarray(steps).tolist():
        kinds[kind] += 1
        top = n - 1 if j == 0 else ((j & -j).bit_length() - 1) + 5
        fg += sum(1 << l for l in range(top, (lam + 1 if kind == 0 else lam) - 1, -1)) + (5 * 32 if kind == 2 else 0)
    return {"steps": len(steps), "rate0": kinds[0], "rate1": kinds[1], "mixed": kinds[2], "fg_steps_kept": fg / (N * n), "leaf_blocks_kept": kinds[2] / (N // 32)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "polar_ssc_cost.json"))
    ap.add_argument("--runs", type=int, default=7)
    args = ap.parse_args()
    import torch
    q = _qldpc_loader.load()
    import polar_ref as R
    rng = np.random.default_rng(1)
    res = {"what": "hipEvent ms of one decode_dev call on an SC and an SSC context of the same code, alternating in one process, median of %d; "
                   "'all': u, info and x asked for, no frozen row; 'recon': x alone, with a frozen row" % args.runs, "shapes": {}}
    for n, F, messages, code in SHAPES:
        N, W = 1 << n, (1 << n) // 32
        pos = np.sort(q.polar_pw_order(n)[N // 2:] if code == "pw" else R.nr_order(N)[N // 2:]).astype(np.int32)
        llr = awgn_frames(rng, n, F, messages)
        fz = rng.integers(0, 1 << 32, (F, W), dtype=np.uint64).astype(np.uint32)
        dec = {rule: q.Polar(n, pos, messages, 31, max_frames=F, rule=rule) for rule in ("sc", "ssc")}
        d_llr, d_fz = torch.from_numpy(llr).cuda(), torch.from_numpy(fz.view(np.int32)).cuda()
        row = {"log2_n": n, "frames": F, "messages": messages, "code": code, "n_info": int(pos.size), "plan": plan_stats(n, q.polar_ssc_plan(n, pos)),
               "device_bytes": {rule: d.device_bytes() for rule, d in dec.items()}}
        calls = {"all": lambda d: d.decode(d_llr), "recon": lambda d: d.decode(d_llr, d_fz, want=("x",))}
        for form, call in calls.items():
            for rule in ("sc", "ssc", "sc", "ssc"):          # alternating; the second pass is the one kept, the first is beside it
                t = event_ms(torch, lambda: call(dec[rule]), args.runs)
                key = "%s_%s_ms" % (form, rule)
                if key in row:
                    row[key + "_first_pass"] = row[key]
                row[key] = t
            row["%s_ssc_over_sc" % form] = row["%s_ssc_ms" % form]["median"] / row["%s_sc_ms" % form]["median"]
        Fh = min(F, HOST_FRAMES[n])
        host = q.polar_decode_ssc_host(n, pos, llr[:Fh], fz[:Fh], messages, 31)
        got = dec["ssc"].decode(d_llr[:Fh], d_fz[:Fh])
        row["host_frames"] = Fh
        row["device_equals_mirror"] = bool(all(np.array_equal(got[k].cpu().numpy().view(np.uint32), host[k]) for k in ("u", "info", "x")))
        res["shapes"]["n=%d x %d %s %s" % (n, F, messages, code)] = row
        print(n, F, messages, code, json.dumps(row["plan"]), {k: round(row[k]["median"], 4) for k in row if k.endswith("_ms")}, row["device_equals_mirror"], flush=True)
        del dec, d_llr, d_fz
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
