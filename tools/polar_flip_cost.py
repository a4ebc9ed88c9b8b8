#!/usr/bin/env python3
"""What SC-Flip trials cost on the device: hipEvent ms, medians of 7 after a warm-up call, one process.

PolarRecon.decode_flip at QBER 6 %, K = N / 2 in polarization-weight order, CRC 32, no ladder, at N = 2^10 x 20 000 blocks (both message types) and
N = 2^16 x 4 096 blocks (int8), T in {1, 8, 32}, against PolarRecon.decode on the same context and session.  Recorded per shape and T:

  whole call        decode_flip from fresh copies of Bob's keys (made outside the events), with n_tried and the blocks rescued
  plain call        PolarRecon.decode on the same session: what a caller paid before
  first pass        decode_rounds with one round on the same session: the kernels of the call's first pass
  probe             Polar.decode_rows with the leaf output on n_tried frames
  select            qldpc_polar_flip_select_dev on n_tried leaf rows (at 2^16 this is the T N / 64 loads a lane of the successive minima)
  trial decode      Polar.decode_rows (info and x) on the chunks of max_blocks / T blocks x T frames that the call runs
  rest              the whole call minus the four above: trial prior, settle, the memsets and the read-back, which have no entry of their own

No threshold is set.  Writes profiles/polar_flip_cost.json.

    python tools/polar_flip_cost.py [--out profiles/polar_flip_cost.json] [--runs 7] [--shapes 10:20000:i8,10:20000:f32,16:4096:i8]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _qldpc_loader  # noqa: E402
from polar_common import event_ms  # noqa: E402
from polar_ladder_cost import timed_with_setup  # noqa: E402

QBER, FLIPS = 0.06, (1, 8, 32)
CRC32 = (32, 0x04C11DB7)


def bsc_words(torch, B, N, qber, gen, rows=256):
    """packed rows [B, N / 32] of a BSC's flips, made on the device a slab of rows at a time"""
    weights = (1 << torch.arange(31, -1, -1, device="cuda", dtype=torch.int64))
    out = torch.empty((B, N // 32), dtype=torch.int32, device="cuda")
    for b0 in range(0, B, rows):
        b1 = min(B, b0 + rows)
        bits = (torch.rand((b1 - b0, N // 32, 32), device="cuda", generator=gen) < qber).to(torch.int64)
        words = (bits * weights).sum(dim=2)
        out[b0:b1] = torch.where(words >= 1 << 31, words - (1 << 32), words).to(torch.int32)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "polar_flip_cost.json"))
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--shapes", default="10:20000:i8,10:20000:f32,16:4096:i8")
    args = ap.parse_args()
    import torch
    q = _qldpc_loader.load()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(20263)
    med = lambda v: v["median"]
    res = {"what": "hipEvent ms, median of %d after a warm-up call, one process; decode_flip at QBER %g, K = N / 2, CRC-32, no ladder, against the plain session "
                   "decode on the same context; rest = whole call - first pass - probe - select - trial decode" % (args.runs, QBER), "shapes": {}}
    for shape in args.shapes.split(","):
        n, B, messages = shape.split(":")
        n, B = int(n), int(B)
        N, W = 1 << n, (1 << n) // 32
        pos = q.polar_pw_order(n)[N // 2:].astype(np.int32)
        dec = q.Polar(n, pos, messages, 31, max_frames=B)
        sess = q.PolarRecon(dec, *CRC32, max_blocks=B, max_flips=max(FLIPS))
        d_alice = torch.randint(-(1 << 31), 1 << 31, (B, W), device="cuda", generator=gen, dtype=torch.int64).to(torch.int32)
        d_bob = d_alice ^ bsc_words(torch, B, N, QBER, gen)
        syn, crc = sess.encode(d_alice)
        fresh = lambda: d_bob.clone()
        zeros = torch.zeros(B, dtype=torch.int32, device="cuda")
        row = {"log2_n": n, "blocks": B, "messages": messages, "n_info": int(pos.size), "qber": QBER, "session_device_bytes": sess.device_bytes(),
               "context_device_bytes": dec.device_bytes(),
               "plain_call_ms": timed_with_setup(torch, fresh, lambda k: sess.decode(k, syn, crc), args.runs),
               "first_pass_ms": timed_with_setup(torch, lambda: (d_bob.clone(), zeros.clone()), lambda s: sess.decode_rounds(s[0], syn, crc, None, s[1], max_rounds=1), args.runs),
               "flips": {}}
        for T in FLIPS:
            last = {}
            whole = timed_with_setup(torch, fresh, lambda k: last.update(sess.decode_flip(k, syn, crc, n_flips=T)), args.runs)
            tried = int(last["n_tried"])
            at = {"n_flips": T, "n_tried": tried, "rescued": int((last["flip_pos"] >= 0).sum().item()), "still_failed": int((last["status"] != 0).sum().item()),
                  "whole_call_ms": whole, "whole_over_plain": med(whole) / med(row["plain_call_ms"])}
            if tried:
                # stand-ins of the stages on frames of the call's shapes: the decoder's time does not depend on what the rows hold
                chunk = B // T
                llr = torch.ones((B, N), dtype=torch.int8 if messages == "i8" else torch.float32, device="cuda")
                rows = torch.zeros((B, W), dtype=torch.int32, device="cuda")
                probe = 0.0
                for o0 in range(0, tried, chunk):
                    nc = min(chunk, tried - o0)
                    probe += med(event_ms(torch, lambda: dec.decode_rows(llr[:nc], rows[:nc], leaf=True, want=()), args.runs))
                leaf = dec.decode_rows(llr[:min(tried, B)], rows[:min(tried, B)], leaf=True, want=())["leaf"]
                mask = torch.from_numpy(q.polar_recon_tables(n, pos)[0].view(np.int32)).cuda()
                sel = torch.empty((tried, T), dtype=torch.int32, device="cuda")
                stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
                kind = 0 if messages == "i8" else 1
                select = event_ms(torch, lambda: q._L.qldpc_polar_flip_select_dev(stream, n, kind, tried, C.c_void_p(leaf.data_ptr()), C.c_void_p(mask.data_ptr()), None, None, T,
                                                                                 C.c_void_p(sel.data_ptr())), args.runs)
                trial = 0.0
                for o0 in range(0, tried, chunk):
                    nc = min(chunk, tried - o0) * T
                    trial += med(event_ms(torch, lambda: dec.decode_rows(llr[:nc], rows[:nc], want=("info", "x")), args.runs))
                at.update(probe_ms=probe, select_ms=med(select), trial_decode_ms=trial, chunks=(tried + chunk - 1) // chunk)
                at["rest_ms"] = med(whole) - med(row["first_pass_ms"]) - probe - med(select) - trial
                del llr, rows, leaf, sel
            row["flips"]["T=%d" % T] = at
            print(json.dumps({k: (round(v["median"], 4) if isinstance(v, dict) else (round(v, 4) if isinstance(v, float) else v)) for k, v in at.items()}), flush=True)
        res["shapes"]["n=%d x %d %s" % (n, B, messages)] = row
        print(json.dumps({k: (round(v["median"], 4) if isinstance(v, dict) and "median" in v else v) for k, v in row.items() if k != "flips"}), flush=True)
        del sess, dec, d_alice, d_bob
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
