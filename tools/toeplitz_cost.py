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

The NTT method against the direct one (`--method direct | ntt | both`, default both), into profiles/toeplitz_ntt_cost.json:

    timeout -k 10 900 python tools/toeplitz_cost.py --leg sweep --out profiles/toeplitz_ntt_cost.json && \
    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d PROF -o passes -- python tools/toeplitz_cost.py --leg passes && \
    python tools/toeplitz_cost.py --leg kernels --kernel-stats PROF/.../passes_kernel_stats.csv --out profiles/toeplitz_ntt_cost.json

sweep:  one blocks_dev call (device rows, hipEvent time of what it queued) per method, the methods alternating in ONE process after two warm-up
        calls each, median and best of --steps: single blocks of n = m = 2^16, 2^18, 2^20, 2^22, 2^24 bits (--max-log2 stops earlier), and the
        daemon's 56 880 -> 41 935 bits as 1 and 256 blocks with a seed per block and with one shared seed.  The two methods' words are compared
        at every shape before anything is timed; the ratio is direct over NTT, and `crossover` names the first n = m at which NTT is faster.
passes: nothing but --steps NTT calls at n = m = 2^--max-log2, to be run under the kernel trace of a profiler (a run of its own).
kernels: reads that trace's per-kernel statistics (--kernel-stats, a CSV with Name / Calls / AverageNs columns) and files the tzn_* rows.
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


def _rows(torch, q, rng, blocks, n, m, shared):
    keys = np.stack([q.pack_bits(rng.integers(0, 2, n)) for _ in range(blocks)])
    sw = q.toeplitz_seed_words(n, m)
    seeds = rng.integers(0, 1 << 32, (1 if shared else blocks, sw), dtype=np.uint32)
    dev = lambda a: torch.from_numpy(a.view(np.int32)).cuda()
    return dev(keys), dev(seeds)


def _time_shape(torch, ctxs, keys_t, seeds_t, n, m, shared, steps):
    """{method: [event ms]} of one blocks_dev call each, the methods alternating; their words compared first"""
    blocks = keys_t.shape[0]
    kbs, obs = [n] * blocks, [m] * blocks
    outs = {k: torch.zeros((blocks, (m + 31) // 32), dtype=torch.int32, device="cuda") for k in ctxs}
    for k, c in ctxs.items():
        for _ in range(2):
            c.blocks_dev(keys_t, kbs, seeds_t, obs, seed_shared=shared, out_t=outs[k])
    torch.cuda.synchronize()
    if len(ctxs) == 2:
        assert torch.equal(outs["direct"], outs["ntt"]), "the two methods differ at %d blocks of %d -> %d" % (blocks, n, m)
    ms = {k: [] for k in ctxs}
    for _ in range(steps):
        for k, c in ctxs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            c.blocks_dev(keys_t, kbs, seeds_t, obs, seed_shared=shared, out_t=outs[k])
            b.record()
            torch.cuda.synchronize()
            ms[k].append(a.elapsed_time(b))
    return ms


def _entry(ms, blocks, n, m, stats):
    e = dict(blocks=blocks, key_bits=n, out_bits=m, bit_products=float(blocks) * n * m)
    for k, v in ms.items():
        e[k + "_event_ms"] = dict(median=float(np.median(v)), best=float(min(v)), runs=[round(x, 4) for x in v])
    if len(ms) == 2:
        e["direct_over_ntt"] = float(np.median(ms["direct"]) / np.median(ms["ntt"]))
    if stats:
        e["ntt_stats"] = stats
    return e


def leg_sweep(q, torch, steps, methods, max_log2):
    rng = np.random.default_rng(2)

    def ctxs(blocks, n, m):
        return {k: q.Toeplitz(max_blocks=blocks, max_key_bits=n, max_out_bits=m, method=k) for k in methods}

    single, crossover = {}, None
    for lg in (16, 18, 20, 22, 24):
        if lg > max_log2:
            break
        n = m = 1 << lg
        c = ctxs(1, n, m)
        keys_t, seeds_t = _rows(torch, q, rng, 1, n, m, False)
        ms = _time_shape(torch, c, keys_t, seeds_t, n, m, False, steps)
        single["2^%d" % lg] = e = _entry(ms, 1, n, m, c["ntt"].stats() if "ntt" in c else None)
        if crossover is None and e.get("direct_over_ntt", 0) > 1:
            crossover = "2^%d" % lg
        del c, keys_t, seeds_t
    daemon = {}
    for blocks in (1, 256):
        c = ctxs(blocks, KB, OB)
        for shared in (False, True):
            keys_t, seeds_t = _rows(torch, q, rng, blocks, KB, OB, shared)
            ms = _time_shape(torch, c, keys_t, seeds_t, KB, OB, shared, steps)
            daemon["%d blocks, %s" % (blocks, "one shared seed" if shared else "a seed per block")] = _entry(ms, blocks, KB, OB, c["ntt"].stats() if "ntt" in c else None)
    return dict(steps=steps, methods=list(methods), single_blocks=single, daemon_blocks=daemon,
                crossover=crossover if len(methods) == 2 else "not measured: one method only",
                what="hipEvent ms around one blocks_dev call; direct_over_ntt is the ratio of the medians; crossover: the first n = m of the sweep at which NTT is faster")


def leg_passes(q, torch, steps, max_log2):
    n = m = 1 << max_log2
    rng = np.random.default_rng(3)
    c = q.Toeplitz(max_blocks=1, max_key_bits=n, max_out_bits=m, method="ntt")
    keys_t, seeds_t = _rows(torch, q, rng, 1, n, m, False)
    out_t = torch.zeros((1, m // 32), dtype=torch.int32, device="cuda")
    for _ in range(steps):
        c.blocks_dev(keys_t, [n], seeds_t, [m], out_t=out_t)
    torch.cuda.synchronize()
    return dict(calls=steps, key_bits=n, out_bits=m, stats=c.stats())


def leg_kernels(path):
    import csv
    rows = {}
    for r in csv.DictReader(open(path)):
        name = r.get("Name", "")
        if "tzn_" in name:
            rows[name.split("(")[0].replace("void ", "")] = dict(calls=int(r["Calls"]), average_us=float(r["AverageNs"]) / 1e3, total_ms=float(r["TotalDurationNs"]) / 1e6)
    if not rows:
        raise RuntimeError("no tzn_* kernel in %s" % path)
    return dict(source="per-kernel statistics of a kernel trace of `--leg passes`", kernels=rows,
                what="tzn_fwd<B, 1 | 2>: pass 0 from key / seed bits; tzn_fwd<B, 0>: the later forward passes; tzn_inv<B, product, output>: the first "
                     "inverse pass takes the product, the last one writes the words")


def leg_stream():
    exe = os.path.join(ROOT, "qcrypto-ldpc_amd", "host", "qldpc_stream")
    p = subprocess.run([exe, "-b", "512", "-r", "5", "-U"], capture_output=True, text=True, timeout=800)
    if p.returncode not in (0, 3):
        raise RuntimeError("qldpc_stream: %d %s" % (p.returncode, p.stderr[-1000:]))
    return dict(command="qldpc_stream -b 512 -r 5 -U", result=json.loads(p.stdout.strip().splitlines()[-1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("sizes", "stream", "sweep", "passes", "kernels"), required=True)
    ap.add_argument("--method", choices=("direct", "ntt", "both"), default="both")
    ap.add_argument("--max-log2", type=int, default=24)
    ap.add_argument("--kernel-stats")
    ap.add_argument("--out", help="default: profiles/toeplitz_cost.json; profiles/toeplitz_ntt_cost.json for the sweep and kernels legs")
    ap.add_argument("--steps", type=int, default=5)
    args = ap.parse_args()
    if not args.out:
        args.out = os.path.join(ROOT, "profiles", "toeplitz_ntt_cost.json" if args.leg in ("sweep", "kernels") else "toeplitz_cost.json")
    if args.leg == "stream":
        leg = leg_stream()
    elif args.leg == "kernels":
        leg = leg_kernels(args.kernel_stats)
    elif args.leg in ("sweep", "passes"):
        import torch

        import _qldpc_loader
        q = _qldpc_loader.load()
        if args.leg == "passes":
            print(json.dumps(leg_passes(q, torch, args.steps, args.max_log2)))
            return
        leg = leg_sweep(q, torch, args.steps, ("direct", "ntt") if args.method == "both" else (args.method,), args.max_log2)
    else:
        import torch

        import _qldpc_loader
        q = _qldpc_loader.load()
        leg = leg_sizes(q, torch, args.steps)
    out = {}
    if os.path.exists(args.out):
        out = json.load(open(args.out))
    if args.leg in ("sweep", "kernels"):
        out[args.leg] = leg
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")
        print(json.dumps(leg))
        return
    out["what"] = ("Toeplitz hashing per call against the LFSR hash of the same shapes; wall ms are the best of `steps` runs, host calls include "
                   "their copies; bit-products = blocks x key_bits x out_bits")
    out[args.leg] = leg
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(leg))


if __name__ == "__main__":
    main()
