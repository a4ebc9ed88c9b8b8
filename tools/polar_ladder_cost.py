#!/usr/bin/env python3
"""What a frozen set per frame and incremental freezing rounds cost on the device: hipEvent ms, medians of 7 after a warm-up call, one process.

  rows      Polar.decode_rows with all-zero rows against Polar.decode on the same context and frames (u, info and x asked for), at N = 2^10 x 20 000
            and N = 2^16 x 4 096, both message types at 2^10 and int8 at 2^16: the price of the extra word.
  rounds    PolarRecon.decode_rounds at QBER 6 %, N = 2^10 x 20 000, K = 512 in polarization-weight order, CRC 32, the ladder the 128 least reliable
            information positions, step 16, 5 rounds from zero, against five whole-batch PolarRecon.decode calls on the same session: what compaction
            buys.  open_per_round is recorded.  The call rewrites keys and counts, so every timed call starts from fresh copies, made outside the
            events.

Writes profiles/polar_ladder_cost.json; --polar-cost NAME=FILE adds the output of a tools/polar_cost.py run under polar_cost_parent_head.

    python tools/polar_ladder_cost.py [--out profiles/polar_ladder_cost.json] [--runs 7] [--polar-cost parent=a.json --polar-cost head=b.json]
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

ROWS_SHAPES = [(10, 20000, "i8"), (10, 20000, "f32"), (16, 4096, "i8")]
QBER, STEP, ROUNDS, LADDER = 0.06, 16, 5, 128
CRC32 = (32, 0x04C11DB7)


def timed_with_setup(torch, setup, fn, runs):
    """event_ms of fn(state) where state = setup() is made afresh, outside the events, before every call"""
    out = []
    for k in range(runs + 1):
        state = setup()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(state)
        b.record()
        b.synchronize()
        if k:
            out.append(a.elapsed_time(b))
    return {"median": float(np.median(out)), "best": float(min(out)), "worst": float(max(out)), "runs": [round(v, 4) for v in out]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "polar_ladder_cost.json"))
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--polar-cost", action="append", default=[], metavar="NAME=FILE")
    args = ap.parse_args()
    import torch
    q = _qldpc_loader.load()
    rng = np.random.default_rng(1)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32) if a.dtype == np.uint32 else np.ascontiguousarray(a)).cuda()
    res = {"what": "hipEvent ms, median of %d after a warm-up call, one process; rows: decode_rows with all-zero rows over decode on the same context and frames; "
                   "rounds: decode_rounds (step %d, %d rounds, QBER %g) against %d whole-batch session decodes" % (args.runs, STEP, ROUNDS, QBER, ROUNDS),
           "rows": {}, "rounds": {}}
    for n, F, messages in ROWS_SHAPES:
        N, W = 1 << n, (1 << n) // 32
        pos = np.sort(q.polar_pw_order(n)[N // 2:]).astype(np.int32)
        dec = q.Polar(n, pos, messages, 31, max_frames=F)
        d_llr = dev(awgn_frames(rng, n, F, messages))
        d_rows = torch.zeros((F, W), dtype=torch.int32, device="cuda")
        row = {"log2_n": n, "frames": F, "messages": messages, "n_info": int(pos.size),
               "decode_ms": event_ms(torch, lambda: dec.decode(d_llr), args.runs),
               "decode_rows_ms": event_ms(torch, lambda: dec.decode_rows(d_llr, d_rows), args.runs),
               "decode_again_ms": event_ms(torch, lambda: dec.decode(d_llr), args.runs)}
        row["rows_over_decode"] = row["decode_rows_ms"]["median"] / row["decode_ms"]["median"]
        a, b = dec.decode(d_llr), dec.decode_rows(d_llr, d_rows)
        row["equal_outputs"] = bool(all(torch.equal(a[k], b[k]) for k in a))
        res["rows"]["n=%d x %d %s" % (n, F, messages)] = row
        print(json.dumps({k: (round(v["median"], 4) if isinstance(v, dict) else v) for k, v in row.items()}), flush=True)
        del dec, d_llr, d_rows
    for messages in ("i8", "f32"):
        n, B = 10, 20000
        N, W = 1 << n, (1 << n) // 32
        order = q.polar_pw_order(n)
        pos = order[N // 2:].astype(np.int32)                     # ascending reliability: the ladder is its head
        xp = pos[:LADDER].copy()
        dec = q.Polar(n, pos, messages, 31, max_frames=B)
        sess = q.PolarRecon(dec, *CRC32, max_blocks=B, extra_pos=xp)
        alice = rng.integers(0, 1 << 32, (B, W), dtype=np.uint64).astype(np.uint32)
        flips = np.packbits(rng.random((B, N), dtype=np.float32) < QBER, axis=1, bitorder="big").view(">u4").astype(np.uint32)
        d_alice, d_bob = dev(alice), dev(alice ^ flips)
        syn, crc, xb = sess.encode(d_alice, want_extra=True)
        fresh = lambda: (d_bob.clone(), torch.zeros(B, dtype=torch.int32, device="cuda"))
        last = {}

        def rounds(state):
            last.update(sess.decode_rounds(state[0], syn, crc, xb, state[1], step=STEP, max_rounds=ROUNDS))

        def whole(state):
            for _ in range(ROUNDS):
                sess.decode(state[0], syn, crc)

        row = {"log2_n": n, "blocks": B, "messages": messages, "n_info": int(pos.size), "n_extra": LADDER, "step": STEP, "max_rounds": ROUNDS, "qber": QBER,
               "session_device_bytes": sess.device_bytes(), "context_device_bytes": dec.device_bytes(),
               "alice_call_ms": event_ms(torch, lambda: sess.encode(d_alice), args.runs),
               "alice_ladder_call_ms": event_ms(torch, lambda: sess.encode(d_alice, want_extra=True), args.runs),
               "one_decode_call_ms": timed_with_setup(torch, fresh, lambda s: sess.decode(s[0], syn, crc), args.runs),
               "decode_rounds_ms": timed_with_setup(torch, fresh, rounds, args.runs),
               "whole_batch_decodes_ms": timed_with_setup(torch, fresh, whole, args.runs)}
        row["open_per_round"] = last["open_per_round"]
        row["failed_blocks"] = int((last["status"] != 0).sum().item())
        row["rounds_over_whole"] = row["decode_rounds_ms"]["median"] / row["whole_batch_decodes_ms"]["median"]
        row["rounds_over_one_decode"] = row["decode_rounds_ms"]["median"] / row["one_decode_call_ms"]["median"]
        res["rounds"]["n=%d x %d %s" % (n, B, messages)] = row
        print(json.dumps({k: (round(v["median"], 4) if isinstance(v, dict) else v) for k, v in row.items()}), flush=True)
        del sess, dec
    for item in args.polar_cost:
        name, path = item.split("=", 1)
        res.setdefault("polar_cost_parent_head", {}).setdefault(name, []).append(json.load(open(path)))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
