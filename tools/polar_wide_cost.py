#!/usr/bin/env python3
"""What the two forms of the polar SC decoder cost on the device, in one process: hipEvent time of one decode call (u, info and x asked for; median
of 7 after a warm-up call) of Polar(form="lanes") and Polar(form="wide") on the same frames, at n in {10, 14, 16, 18, 20} x {1, 8, 64, 4 096}
frames with int8 messages, and with float messages at n = 16 and 20.  Per shape: both contexts' device_bytes, the ratio lanes / wide, whether the
wide result is the host mirror's.  A shape whose lanes context would not fit in device memory is skipped and listed.  Then the alternatives of
the wide form at the one-frame shapes: chip levels, workgroup sizes and the leaf block on one lane or on 32, through QLDPC_POLAR_WIDE_CHIP,
QLDPC_POLAR_WIDE_LANES and QLDPC_POLAR_WIDE_LEAF, which a context reads when it is created.  Then where a frame's time goes.  Writes profiles/polar_wide_cost.json.

    python tools/polar_wide_cost.py [--out profiles/polar_wide_cost.json] [--runs 7] [--quick] [--max-log2-beliefs 32]
"""
import argparse
import json
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _qldpc_loader  # noqa: E402
from polar_common import awgn_frames, event_ms  # noqa: E402

SIZES = (10, 14, 16, 18, 20)
FRAMES = (1, 8, 64, 4096)
F32_SIZES = (16, 20)
GATED = ((16, "i8"), (16, "f32"), (20, "i8"), (20, "f32"))      # one frame of these: the wide form has to win
CHIPS = (8, 10, 12, 13)
LANES = (64, 256, 512, 1024)
MIRROR_MAX = 1 << 24      # the mirror is run on as many frames as keep frames x N at or below this


def core_define(name):
    text = open(os.path.join(ROOT, "qcrypto-ldpc_amd", "csrc", "qldpc_polar_wide_core.h")).read()
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))


def frames_of(torch, rng, n, F, messages):
    """F frames of a half-rate code on AWGN: at most 64 distinct ones on the host, repeated on the device (a decode's time does not depend on the
    values) -> (the distinct frames, the device tensor [F, N])"""
    Fd = min(F, 64)
    llr = awgn_frames(rng, n, Fd, messages)
    return llr, torch.from_numpy(llr).cuda().repeat((F + Fd - 1) // Fd, 1)[:F].contiguous()


def lanes_bytes(n, F, messages):
    """what a lanes context of F frames allocates (qldpc_kernels_polar.h): beliefs and two rows for each group of 64 frames"""
    groups, N = (F + 63) // 64, 1 << n
    return groups * ((2 * N - 64) * 64 * (1 if messages == "i8" else 4) + 2 * (N // 32) * 64 * 4)


def with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def where_the_time_goes(res):
    """from the one-frame int8 shapes: a frame of 2^n has 2^(n - 5) leaf blocks, and before a leaf block the levels above it are renewed, half a
    belief per leaf and level, on all lanes.  A straight line ms = fixed + blocks x per_block through the shapes, and what each shape leaves of it:
    were the levels above the chip level (scratch) or below it (LDS) a visible share, the time per leaf block would grow with n, by the n - 6
    levels a longer frame has.  The alternatives say the same from the other side: the chip level and the workgroup size do not move the time,
    the lanes of a leaf block do"""
    one = {n: res["shapes"]["n=%d x 1 i8" % n]["wide_ms"]["median"] for n in SIZES if "n=%d x 1 i8" % n in res["shapes"]}
    if len(one) < 3:
        return {}
    ns = sorted(one)
    blocks, ms = np.array([float(1 << (n - 5)) for n in ns]), np.array([one[n] for n in ns])
    per_block, fixed = np.polyfit(blocks, ms, 1, w=1.0 / ms)      # relative errors: the largest shape does not decide alone
    out = {"fixed_ms": float(fixed), "us_per_leaf_block": float(per_block * 1e3),
           "us_per_leaf_block_by_log2_n": {str(n): float((one[n] - fixed) * 1e3 / (1 << (n - 5))) for n in ns},
           "ms_left_by_the_line_by_log2_n": {str(n): float(one[n] - fixed - per_block * (1 << (n - 5))) for n in ns}}
    alt = res["alternatives"].get("n=16 x 1 i8")
    if alt:
        name = "chip=%d lanes=%d leaf_lanes=" % (res["chip_level"], res["workgroup"])
        if name + "1" in alt and name + "32" in alt:
            out["us_per_leaf_block_at_n16_leaf_on_one_lane"] = alt[name + "1"]["ms"] * 1e3 / 2048
            out["us_per_leaf_block_at_n16_leaf_on_32_lanes"] = alt[name + "32"]["ms"] * 1e3 / 2048
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "polar_wide_cost.json"))
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="the one-frame shapes only, no alternatives")
    ap.add_argument("--max-log2-beliefs", type=int, default=32, help="skip (and list) shapes of more than 2^this frames x N, to bound the run's time")
    args = ap.parse_args()
    import torch
    q = _qldpc_loader.load()
    rng = np.random.default_rng(1)
    free_bytes = torch.cuda.mem_get_info()[0]
    chip, lanes, leaf_lanes = core_define("PLW_CHIP_LOG"), core_define("PLW_LANES"), core_define("PLW_LEAF_LANES") or 1
    res = {"what": "hipEvent ms of one decode call (u, info and x asked for), median of %d after a warm-up call, both forms in one process on the same "
                   "frames; ratio = lanes median / wide median (above 1: the wide form is faster)" % args.runs,
           "chip_level": chip, "workgroup": lanes, "leaf_block_lanes": leaf_lanes, "shapes": {}, "skipped": [], "alternatives": {}, "gate": {}}
    shapes = [(n, F, "i8") for n in SIZES for F in FRAMES] + [(n, F, "f32") for n in F32_SIZES for F in FRAMES]
    if args.quick:
        shapes = [s for s in shapes if s[1] == 1]
    for n, F, messages in shapes:
        N, key = 1 << n, "n=%d x %d %s" % (n, F, messages)
        need = lanes_bytes(n, F, messages) + F * N * (5 if messages == "i8" else 8) + 3 * F * (N // 8)
        if need > 0.8 * free_bytes or F * N > 1 << args.max_log2_beliefs:
            res["skipped"].append({"shape": key, "lanes_context_and_frames_bytes": int(need), "free_bytes": int(free_bytes),
                                   "why": "device memory" if need > 0.8 * free_bytes else "more than 2^%d beliefs: the run's time" % args.max_log2_beliefs})
            print("skip", key, need >> 20, "MiB", flush=True)
            continue
        pos = np.sort(q.polar_pw_order(n)[N // 2:]).astype(np.int32)
        llr, d_llr = frames_of(torch, rng, n, F, messages)
        row = {"log2_n": n, "frames": F, "messages": messages, "chip_level": min(chip, n - 1), "workgroup": lanes}
        got = {}
        for form in ("lanes", "wide"):
            dec = q.Polar(n, pos, messages, 31, max_frames=F, form=form)
            row[form + "_device_bytes"] = dec.device_bytes()
            row[form + "_ms"] = event_ms(torch, lambda: dec.decode(d_llr), args.runs)
            got[form] = {k: v.cpu().numpy().view(np.uint32) for k, v in dec.decode(d_llr).items()}
            del dec
        row["ratio_lanes_over_wide"] = row["lanes_ms"]["median"] / row["wide_ms"]["median"]
        row["device_bytes_ratio"] = row["lanes_device_bytes"] / row["wide_device_bytes"]
        Fh = max(1, min(len(llr), MIRROR_MAX >> n))
        host = q.polar_decode_host(n, pos, llr[:Fh], None, messages, 31)
        row["mirror_frames"] = Fh
        row["wide_equals_mirror"] = bool(all(np.array_equal(got["wide"][k][:Fh], host[k]) for k in host))
        row["wide_equals_lanes"] = bool(all(np.array_equal(got["wide"][k], got["lanes"][k]) for k in got["wide"]))
        res["shapes"][key] = row
        print(key, "lanes %.3f ms, wide %.3f ms, ratio %.2f, bytes %d / %d, mirror %s, lanes %s" % (
            row["lanes_ms"]["median"], row["wide_ms"]["median"], row["ratio_lanes_over_wide"], row["lanes_device_bytes"], row["wide_device_bytes"],
            row["wide_equals_mirror"], row["wide_equals_lanes"]), flush=True)
        if F == 1 and (n, messages) in GATED:
            lo, hi = row["wide_ms"], row["lanes_ms"]
            spread = max(lo["worst"] - lo["best"], hi["worst"] - hi["best"])
            res["gate"][key] = {"lanes_median_ms": hi["median"], "wide_median_ms": lo["median"], "larger_spread_of_7_ms": spread,
                                "wide_wins_by_more_than_the_spread": bool(hi["median"] - lo["median"] > spread)}
        if F == 1 and (n, messages) in GATED and not args.quick:
            alt = {}
            for c, l, leaf in [(c, lanes, leaf_lanes) for c in CHIPS] + [(chip, l, leaf_lanes) for l in LANES if l != lanes] + [(chip, lanes, 1), (chip, lanes, 32)]:
                env = {"QLDPC_POLAR_WIDE_CHIP": c, "QLDPC_POLAR_WIDE_LANES": l, "QLDPC_POLAR_WIDE_LEAF": leaf}
                dec = with_env(env, lambda: q.Polar(n, pos, messages, 31, max_frames=1, form="wide"))
                t = event_ms(torch, lambda: dec.decode(d_llr), args.runs)
                same = all(np.array_equal(v.cpu().numpy().view(np.uint32), got["wide"][k]) for k, v in dec.decode(d_llr).items())
                name = "chip=%d lanes=%d leaf_lanes=%d" % (c, l, leaf)
                alt[name] = {"ms": t["median"], "best": t["best"], "device_bytes": dec.device_bytes(), "equals_default": bool(same)}
                print("   %s: %.3f ms %s" % (name, t["median"], same), flush=True)
                del dec
            res["alternatives"][key] = alt
        del d_llr
    res["where_the_time_goes"] = where_the_time_goes(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
