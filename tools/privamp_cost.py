#!/usr/bin/env python3
"""What privacy amplification costs per block, one block per call (qldpc_privamp / qldpc_privamp_dev) against the batched calls
(qldpc_privamp_blocks / _blocks_dev), on blocks of 56 880 -> 41 935 bits.  One process per leg; every run merges
its leg into the output file:

    timeout -k 10 300 python tools/privamp_cost.py --leg sizes  --out profiles/privamp_batch_cost.json && \
    timeout -k 10 300 python tools/privamp_cost.py --leg mixed  --out profiles/privamp_batch_cost.json && \
    timeout -k 10 900 python tools/privamp_cost.py --leg stream --out profiles/privamp_batch_cost.json

sizes:  n in {1, 8, 64, 512}: wall ms (best of --steps) and blocks/s of n qldpc_privamp calls, n qldpc_privamp_dev calls on resident keys,
        one qldpc_privamp_blocks call, one qldpc_privamp_blocks_dev call (wall, and the hipEvent time of what it queued).
mixed:  one batch of 512 blocks of lengths drawn from 20 000 .. 65 536 bits (a jump table per distinct length, built on the device), and the
        same number of blocks at their mean length (one table) for what the tables cost.
stream: the JSON line of `qldpc_stream -b 512 -r 5 -H` (reconciliation, then the hash of the reconciled blocks in one call).
Every batched result is compared with the one-block call's before it is timed.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WB, FB = 56880, 41935


def best(fn, steps):
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return min(ts) * 1e3


def dev_call(q, torch, pa, keys_t, wbs, seeds, fbs, steps):
    """(wall ms, event ms) of one blocks_dev call, best of `steps`"""
    n = keys_t.shape[0]
    out_t = torch.zeros((n, (max(fbs) + 31) // 32), dtype=torch.int32, device="cuda")
    wall, evt = [], []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        pa.blocks_dev(keys_t, wbs, seeds, fbs, out_t=out_t)
        b.record()
        torch.cuda.synchronize()
        wall.append(time.perf_counter() - t0)
        evt.append(a.elapsed_time(b))
    return min(wall) * 1e3, min(evt), out_t


def leg_sizes(q, torch, steps):
    import ctypes as C
    rng = np.random.default_rng(1)
    nmax = 512
    keys = [q.pack_bits(rng.integers(0, 2, WB)) for _ in range(nmax)]
    seeds = [int(x) for x in rng.integers(1, 1 << 32, nmax)]
    OW = (FB + 31) // 32
    keys_t = torch.from_numpy(np.stack(keys).view(np.int32)).cuda()
    old_out = torch.zeros((nmax, OW), dtype=torch.int32, device="cuda")
    pa = q.PrivAmp(max_blocks=nmax, max_key_bits=WB, max_final_bits=FB)
    res = {}
    for n in (1, 8, 64, 512):
        wbs, fbs = [WB] * n, [FB] * n

        def old_host():
            return [q.privamp(keys[i], WB, seeds[i], FB) for i in range(n)]

        def old_dev():
            for i in range(n):
                q._chk(q._L.qldpc_privamp_dev(keys_t[i].data_ptr(), WB, C.c_uint32(seeds[i]), FB, old_out[i].data_ptr(), torch.cuda.current_stream().cuda_stream), "privamp_dev")
            torch.cuda.synchronize()

        def new_host():
            return pa.blocks(keys[:n], wbs, seeds[:n], fbs)

        ref, got = old_host(), new_host()
        assert all((a == b).all() for a, b in zip(ref, got)), "batched hash differs from qldpc_privamp"
        old_dev()
        w, e, out_t = dev_call(q, torch, pa, keys_t[:n], wbs, seeds[:n], fbs, steps + 1)
        assert (out_t.cpu().numpy().view(np.uint32) == np.stack(ref)).all() and (old_out[:n].cpu().numpy().view(np.uint32) == np.stack(ref)).all()
        ms = dict(privamp_n_calls=best(old_host, steps), privamp_dev_n_calls=best(old_dev, steps), privamp_blocks=best(new_host, steps),
                  privamp_blocks_dev=w, privamp_blocks_dev_event=e)
        res[str(n)] = dict(wall_ms=ms, blocks_per_s={k: n / (v * 1e-3) for k, v in ms.items()})
    return dict(block="%d -> %d bits" % (WB, FB), steps=steps, device_bytes=pa.device_bytes, n=res)


def leg_mixed(q, torch, steps):
    rng = np.random.default_rng(2)
    n = 512
    wbs = [int(x) for x in rng.integers(20000, 65537, n)]
    fbs = [int(w * FB / WB) for w in wbs]
    seeds = [int(x) for x in rng.integers(1, 1 << 32, n)]
    keys = [q.pack_bits(rng.integers(0, 2, w)) for w in wbs]
    pa = q.PrivAmp(max_blocks=n, max_key_bits=65536, max_final_bits=65536)
    got = pa.blocks(keys, wbs, seeds, fbs)
    for i in range(0, n, 37):
        assert (got[i] == q.privamp(keys[i], wbs[i], seeds[i], fbs[i])).all(), "batched hash differs from qldpc_privamp"
    keys_np = np.zeros((n, 2048), np.uint32)
    for i, k in enumerate(keys):
        keys_np[i, :k.size] = k
    keys_t = torch.from_numpy(keys_np.view(np.int32)).cuda()
    w, e, _ = dev_call(q, torch, pa, keys_t, wbs, seeds, fbs, steps + 1)
    # the same number of blocks at the mean length: one table instead of one per distinct length
    mw = int(round(sum(wbs) / n))
    mf = int(mw * FB / WB)
    w1, e1, _ = dev_call(q, torch, pa, keys_t, [mw] * n, seeds, [mf] * n, steps + 1)
    return dict(blocks=n, workbits="U[20000, 65536]", final_bits="workbits x %d / %d" % (FB, WB), distinct_lengths_in_words=len({(x + 31) // 32 for x in wbs}),
                key_Mbit=sum(wbs) / 1e6, final_Mbit=sum(fbs) / 1e6, steps=steps,
                wall_ms=dict(privamp_blocks=best(lambda: pa.blocks(keys, wbs, seeds, fbs), steps), privamp_blocks_dev=w, privamp_blocks_dev_event=e),
                one_length=dict(workbits=mw, final_bits=mf, wall_ms=dict(privamp_blocks_dev=w1, privamp_blocks_dev_event=e1)))


def leg_stream():
    exe = os.path.join(ROOT, "qcrypto-ldpc_amd", "host", "qldpc_stream")
    p = subprocess.run([exe, "-b", "512", "-r", "5", "-H"], capture_output=True, text=True, timeout=800)
    if p.returncode not in (0, 3):
        raise RuntimeError("qldpc_stream: %d %s" % (p.returncode, p.stderr[-1000:]))
    return dict(command="qldpc_stream -b 512 -r 5 -H", result=json.loads(p.stdout.strip().splitlines()[-1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("sizes", "mixed", "stream"), required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "privamp_batch_cost.json"))
    ap.add_argument("--steps", type=int, default=5)
    args = ap.parse_args()
    if args.leg == "stream":
        leg = leg_stream()
    else:
        import torch

        import _qldpc_loader
        q = _qldpc_loader.load()
        leg = (leg_sizes if args.leg == "sizes" else leg_mixed)(q, torch, args.steps)
    out = {}
    if os.path.exists(args.out):
        out = json.load(open(args.out))
    out["what"] = "privacy amplification per block: one block per call against one batched call; wall ms are the best of `steps` runs, host calls include their copies"
    out[args.leg] = leg
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(leg))


if __name__ == "__main__":
    main()
