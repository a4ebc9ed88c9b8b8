#!/usr/bin/env python3
"""What Toeplitz hashing costs (qldpc_toeplitz_blocks / _blocks_dev) on blocks of 56 880 -> 41 935 bits with one shared seed, beside the
LFSR hash of the same shapes (PrivAmp.blocks): the difference is what soundness costs.  One process per leg; every run merges its leg into
the output file:

    timeout -k 10 600 python tools/toeplitz_cost.py --leg sizes  --out profiles/toeplitz_cost.json && \
    timeout -k 10 900 python tools/toeplitz_cost.py --leg stream --out profiles/toeplitz_cost.json

sizes:  n in {1, 8, 64, 512} blocks: wall ms (best of --steps) of one Toeplitz.blocks call and of one Toeplitz.blocks_dev call (wall, and the
        hipEvent time of what it queued), bit-products per second (n x key_bits x out_bits over the event time), and the wall ms of one
        PrivAmp.blocks call on the same keys.  Block 0 of every n is compared with the host mirror before anything is timed.
stream: the JSON line of `qldpc_stream -b 512 -r 5 -U` (reconciliation, then the Toeplitz hash of the reconciled blocks in one call).
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
KB, OB = 56880, 41935


def best(fn, steps):
    ts = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return min(ts) * 1e3


def dev_call(torch, tz, keys_t, seed_t, kbs, obs, steps):
    """(wall ms, event ms) of one blocks_dev call, best of `steps`"""
    n = keys_t.shape[0]
    out_t = torch.zeros((n, (max(obs) + 31) // 32), dtype=torch.int32, device="cuda")
    wall, evt = [], []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        tz.blocks_dev(keys_t, kbs, seed_t, obs, seed_shared=True, out_t=out_t)
        b.record()
        torch.cuda.synchronize()
        wall.append(time.perf_counter() - t0)
        evt.append(a.elapsed_time(b))
    return min(wall) * 1e3, min(evt), out_t


def leg_sizes(q, torch, steps):
    rng = np.random.default_rng(1)
    nmax = 512
    keys = [q.pack_bits(rng.integers(0, 2, KB)) for _ in range(nmax)]
    seed = q.pack_bits(rng.integers(0, 2, KB + OB - 1))
    lfsr_seeds = [int(x) for x in rng.integers(1, 1 << 32, nmax)]
    keys_t = torch.from_numpy(np.stack(keys).view(np.int32)).cuda()
    seed_t = torch.from_numpy(seed.view(np.int32)).cuda()
    tz = q.Toeplitz(max_blocks=nmax, max_key_bits=KB, max_out_bits=OB)
    pa = q.PrivAmp(max_blocks=nmax, max_key_bits=KB, max_final_bits=OB)
    ref0 = q.toeplitz_host(keys[0], KB, seed, OB)
    res = {}
    for n in (1, 8, 64, 512):
        kbs, obs = [KB] * n, [OB] * n
        got = tz.blocks(keys[:n], kbs, seed, obs)
        assert (got[0] == ref0).all(), "Toeplitz.blocks differs from the host mirror"
        w, e, out_t = dev_call(torch, tz, keys_t[:n], seed_t, kbs, obs, steps + 1)
        assert (out_t.cpu().numpy().view(np.uint32) == np.stack(got)).all(), "blocks_dev differs from blocks"
        ms = dict(toeplitz_blocks=best(lambda: tz.blocks(keys[:n], kbs, seed, obs), steps), toeplitz_blocks_dev=w, toeplitz_blocks_dev_event=e,
                  privamp_blocks=best(lambda: pa.blocks(keys[:n], kbs, lfsr_seeds[:n], obs), steps))
        products = float(n) * KB * OB
        res[str(n)] = dict(wall_ms=ms, bit_products=products,
                           bit_products_per_s=dict(toeplitz_blocks=products / (ms["toeplitz_blocks"] * 1e-3), toeplitz_blocks_dev_event=products / (e * 1e-3)),
                           toeplitz_over_privamp_wall=ms["toeplitz_blocks"] / ms["privamp_blocks"])
    return dict(block="%d -> %d bits, one shared seed of %d bits" % (KB, OB, KB + OB - 1), steps=steps, device_bytes=tz.device_bytes, n=res)


def leg_stream():
    exe = os.path.join(ROOT, "qcrypto-ldpc_amd", "host", "qldpc_stream")
    p = subprocess.run([exe, "-b", "512", "-r", "5", "-U"], capture_output=True, text=True, timeout=800)
    if p.returncode not in (0, 3):
        raise RuntimeError("qldpc_stream: %d %s" % (p.returncode, p.stderr[-1000:]))
    return dict(command="qldpc_stream -b 512 -r 5 -U", result=json.loads(p.stdout.strip().splitlines()[-1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("sizes", "stream"), required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "toeplitz_cost.json"))
    ap.add_argument("--steps", type=int, default=5)
    args = ap.parse_args()
    if args.leg == "stream":
        leg = leg_stream()
    else:
        import torch

        import _qldpc_loader
        q = _qldpc_loader.load()
        leg = leg_sizes(q, torch, args.steps)
    out = {}
    if os.path.exists(args.out):
        out = json.load(open(args.out))
    out["what"] = ("Toeplitz hashing per call against the LFSR hash of the same shapes; wall ms are the best of `steps` runs, host calls include "
                   "their copies; bit-products = blocks x key_bits x out_bits")
    out[args.leg] = leg
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(leg))


if __name__ == "__main__":
    main()
