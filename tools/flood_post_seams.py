#!/usr/bin/env python3
"""The headline step of bench.py (load_bits / run / fetch_packed on the rate-0.8 N = 65 536 code, flooding NMS 0.75, 50 iterations fixed,
4 096 frames) timed with the decoder's profiling on, as bench.py times it, and off: the difference is what the two event records of every
prof_scope cost, i.e. their share of the ~10 us between two passes of the kernel trace.  Prints one JSON line.

  python tools/flood_post_seams.py [--steps 20] [--warmup 5] [--rounds 3]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--frames", type=int, default=4096)
    args = ap.parse_args()

    import torch

    import _qldpc_loader
    import bench
    q = _qldpc_loader.load()
    device = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    F, qber, n_ite = args.frames, 0.02, 50
    code = q.Code.ira(65536, 52429, 0.125, 11, 3, 7)
    enc = q.Encoder(code, "IRA", device=0)
    K, N = enc.K, code.N
    _, rx = bench.make_frames(q, torch, code, enc, F, qber, 1000, device)
    mag = torch.full((F,), q.bsc_llr(qber), dtype=torch.float32, device=device)
    cls = torch.zeros(N, dtype=torch.uint8, device=device)
    cls[K:] = q.VN_PINNED
    out = torch.empty((F, (N + 31) // 32), dtype=torch.int32, device=device)
    dec = q.Decoder(code, K, n_ite, rule="NMS", rule_param=0.75, enable_syndrome=False, n_frames=F, device=0)
    dec.set_stream(torch.cuda.current_stream(device))

    def step():
        dec.load_bits(rx, mag, cls)
        dec.run()
        dec.fetch_packed(out)

    def timed():
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / args.steps * 1e3

    for _ in range(args.warmup):
        step()
    res = {"profiling_on_ms": [], "profiling_off_ms": []}
    for _ in range(args.rounds):      # alternating, so that a drift of the clocks falls on both alike
        dec.profile(True)
        dec.profile_clear()
        res["profiling_on_ms"].append(timed())
        dec.profile_read()
        dec.profile(False)
        res["profiling_off_ms"].append(timed())
    on, off = min(res["profiling_on_ms"]), min(res["profiling_off_ms"])
    scopes = 2 * n_ite + 2 + 2      # check and variable passes, the closing pair, load and fetch
    res.update(steps=args.steps, flood_post=bool(dec.flood_post), scopes_per_step=scopes, best_on_ms=on, best_off_ms=off,
               us_per_scope=(on - off) * 1e3 / scopes)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
