#!/usr/bin/env python3
"""What error verification by the universal hash costs (PolyHash.blocks_dev), all calls in one process:

    timeout -k 10 600 python tools/polyhash_cost.py --out profiles/polyhash_cost.json && \
    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d PROF -o calls -- python tools/polyhash_cost.py --calls 20

(the second command, a run of its own: the time of the kernel alone, read from the trace's per-kernel statistics)

Shapes: 4 096 blocks of 52 429 bits (the headline's keys), 512 blocks of mixed lengths (20 000 .. 65 536 bits, the config-3 stream) and one
block of 2^24 bits, each with n_keys 1 and 2 and one key row shared by the call.  Per shape, after two warm-up calls, the hipEvent time of
what one blocks_dev call queued, median and best of --steps (7), the call queued behind device fills so that the host's preparation of
the call is not in the interval (host_call_ms: how long the host took to queue it); the tags of block 0 are compared with the host mirror first.  Beside it:
copy_probe over the same number of bytes (GB/s read + written, both access widths), and one PrivAmp.blocks_dev and one direct
Toeplitz.blocks_dev call on the same blocks with 64 output bits (the smallest job either hash can be given on these keys).

No threshold is fixed: the figure to read is key_GB_per_s (the bytes of the keys, which is all the call has to read: 4 bytes per word) against
the copy rate of the same run, and against the multiply bound DESIGN 3.3 derives from the instruction count.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARM = 2


def event_ms(torch, call, steps, busy):
    """hipEvent ms of what one call queued.  The call is queued while the device is still busy with fills of `busy` (the first event lies
    behind them), so the time the host takes to prepare the call is not part of the interval; the fills also leave the caches cold"""
    for _ in range(WARM):
        call()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    call()
    host_ms = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    fills = 8 + int(host_ms / 0.03)                              # a fill of 256 MiB takes about 0.1 ms: three times the host's time, and 0.8 ms
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(fills):
            busy.zero_()
        a.record()
        call()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return dict(median=float(np.median(ms)), best=float(min(ms)), runs=[round(x, 4) for x in ms], host_call_ms=round(host_ms, 4))


def shape(q, torch, rng, name, bits, steps, busy):
    n, stride = len(bits), (max(bits) + 31) // 32
    keys = rng.integers(0, 1 << 32, (n, stride), dtype=np.uint32)
    keys_t = torch.from_numpy(keys.view(np.int32)).cuda()
    key_bytes = 4 * sum((b + 31) // 32 for b in bits)
    res = dict(blocks=n, key_bits=("%d" % bits[0]) if len(set(bits)) == 1 else "%d .. %d, mean %.0f" % (min(bits), max(bits), float(np.mean(bits))), key_bytes=key_bytes)
    for r in (1, 2):
        hk = rng.integers(0, 1 << 32, 2 * r, dtype=np.uint32)
        hk_t = torch.from_numpy(hk.view(np.int32)).cuda()
        ph = q.PolyHash(max_blocks=n, max_key_bits=max(bits), n_keys=r)
        out_t = torch.zeros((n, 2 * r), dtype=torch.int32, device="cuda")
        ph.blocks_dev(keys_t, bits, hk_t, key_shared=True, out_t=out_t)
        torch.cuda.synchronize()
        want = np.concatenate([q.polyhash_host(keys[0], bits[0], hk[2 * i:2 * i + 2]) for i in range(r)])
        assert (out_t[0].cpu().numpy().view(np.uint32) == want).all(), "blocks_dev differs from the host mirror at %s" % name
        ms = event_ms(torch, lambda: ph.blocks_dev(keys_t, bits, hk_t, key_shared=True, out_t=out_t), steps, busy)
        res["polyhash_n_keys_%d" % r] = dict(event_ms=ms, key_GB_per_s=key_bytes / (ms["median"] * 1e-3) / 1e9, device_bytes=ph.device_bytes)
        del ph
    res["copy_probe_GB_per_s"] = dict(narrow=q.copy_probe(nbytes=max(key_bytes, 1 << 20), reps=10, wide=False), wide=q.copy_probe(nbytes=max(key_bytes, 1 << 20), reps=10, wide=True),
                                      what="bytes read + bytes written per second over a buffer of key_bytes")
    ob = [64] * n
    pa = q.PrivAmp(max_blocks=n, max_key_bits=max(bits), max_final_bits=64)
    out_t = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
    seeds = [int(x) for x in rng.integers(1, 1 << 32, n)]
    res["privamp_64_bits"] = dict(event_ms=event_ms(torch, lambda: pa.blocks_dev(keys_t, bits, seeds, ob, out_t=out_t), steps, busy))
    del pa
    tz = q.Toeplitz(max_blocks=n, max_key_bits=max(bits), max_out_bits=64)
    seed_t = torch.from_numpy(rng.integers(0, 1 << 32, q.toeplitz_seed_words(max(bits), 64), dtype=np.uint32).view(np.int32)).cuda()
    res["toeplitz_direct_64_bits"] = dict(event_ms=event_ms(torch, lambda: tz.blocks_dev(keys_t, bits, seed_t, ob, seed_shared=True, out_t=out_t), steps, busy))
    del tz
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "polyhash_cost.json"))
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--headline-blocks", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=0, help="nothing but this many headline calls with one key, to be run under the kernel trace of a profiler (a run of its own)")
    args = ap.parse_args()
    import torch

    import _qldpc_loader
    q = _qldpc_loader.load()
    if q.device_count() < 1:
        raise RuntimeError("polyhash_cost: no HIP device visible; nothing is measured without one")
    rng = np.random.default_rng(61)
    if args.calls:
        bits = [52429] * args.headline_blocks
        keys_t = torch.from_numpy(rng.integers(0, 1 << 32, (len(bits), 1639), dtype=np.uint32).view(np.int32)).cuda()
        hk_t = torch.from_numpy(rng.integers(0, 1 << 32, 2, dtype=np.uint32).view(np.int32)).cuda()
        ph = q.PolyHash(max_blocks=len(bits), max_key_bits=52429)
        out_t = torch.zeros((len(bits), 2), dtype=torch.int32, device="cuda")
        for _ in range(args.calls):
            ph.blocks_dev(keys_t, bits, hk_t, key_shared=True, out_t=out_t)
        torch.cuda.synchronize()
        print(json.dumps(dict(calls=args.calls, blocks=len(bits), key_bits=52429)))
        return
    busy = torch.empty(1 << 26, dtype=torch.int32, device="cuda")
    shapes = {"headline": [52429] * args.headline_blocks, "config 3": [int(b) for b in rng.integers(20000, 65537, 512)], "one long block": [1 << 24]}
    out = dict(what="hipEvent ms of what one PolyHash.blocks_dev call queued (one shared key row), median of `steps` after %d warm-up calls, all in one process; "
                    "key_GB_per_s = key_bytes over the median" % WARM, steps=args.steps, tile_words=q.POLYHASH_TILE_WORDS,
               shapes={k: shape(q, torch, rng, k, v, args.steps, busy) for k, v in shapes.items()})
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
