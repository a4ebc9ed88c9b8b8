#!/usr/bin/env python3
"""What blind reconciliation costs and gives, from one run on an MI355X:

    timeout -k 10 900 python tools/blind_cost.py --out profiles/blind_cost.json

kernel: the time of qldpc_fetch_weakest_dev (16 positions per frame, candidates = the information VNs) on the headline shape -- N = 65 536,
        K = 52 429, flooding NMS 0.75, <= 50 iterations with the early exit, 4 096 frames in 64 groups -- with 1, 8 and 64 groups holding a taken
        frame, beside the decode time of the same batch in the same run (hipEvents; flooding: the time includes the posterior pass
        qldpc_fetch_post_dev would run too), and their ratio.
stream: a config-3-style stream of mixed-rate epochs (--epochs blocks of 28 000 .. 32 000 or 52 000 .. 57 000 bits, QBER 1 .. 5 % per block, estimated exactly)
        through a session with rate_gap scaled by 1.0 / 0.75 / 0.5, two ways on the same blocks: the existing path (first decode, then the
        withheld parity bits for the blocks that failed) and blind rounds of --ask bits.  Per setting: leak per key bit, wall time, the histogram
        of rounds, bits asked, blocks left unreconciled.
No threshold and no claim: the file is the measurement.
"""
import argparse
import json
import os
import sys
import time

import tempfile

import numpy as np

# the sessions' mother codes are grown once and kept on disk between the three settings (and between runs)
os.environ.setdefault("QLDPC_CODE_CACHE", os.path.join(tempfile.gettempdir(), "qldpc_code_cache_%d" % os.getuid()))
os.makedirs(os.environ["QLDPC_CODE_CACHE"], exist_ok=True)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, K, FRAMES, N_ITE = 65536, 52429, 4096, 50


def kernel_leg(q, torch, qber, reps):
    code = q.Code.ira(N, K)
    dec = q.Decoder(code, K, N_ITE, rule="NMS", rule_param=0.75, n_frames=FRAMES, engine="frames", compact="off")
    rng = np.random.default_rng(1)
    flips = rng.random((FRAMES, N)) < qber                             # the all-zero codeword through the BSC
    bits = torch.from_numpy(q.pack_bits(flips).astype(np.uint32).view(np.int32)).cuda()
    mag = torch.full((FRAMES,), float(q.bsc_llr(qber)), device="cuda")
    cand = np.zeros(N, np.uint8)
    cand[:K] = 1
    cand_t = torch.from_numpy(np.tile(q.pack_bits(cand).astype(np.uint32).view(np.int32), (FRAMES, 1))).cuda()

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms = []
        for _ in range(reps):
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return float(np.median(ms)), [float(x) for x in ms]

    dec.set_stream()

    def decode():
        dec.load_bits(bits, mag)
        dec.run()

    decode()
    dec.fetch_weakest(16, cand_t)                                    # warm-up: first launches, the posterior buffer
    decode_ms, decode_all = timed(decode)
    ok = dec.fetch_status()[1].cpu().numpy()
    out = dict(workload="N %d K %d flooding NMS 0.75, <= %d iterations, early exit, compaction off, %d frames (64 groups), QBER %.3f, 16 of the %d information VNs per frame"
                        % (N, K, N_ITE, FRAMES, qber, K), frames_failed=int((ok == 0).sum()), decode_ms=decode_ms, decode_ms_all=decode_all, weakest={})
    for groups in (1, 8, 64):
        take = np.zeros(FRAMES, np.int32)
        take[np.arange(groups) * 64] = 1                            # one taken frame in each of `groups` groups
        take_t = torch.from_numpy(take).cuda()
        ms, all_ms = timed(lambda: dec.fetch_weakest(16, cand_t, take_t))
        out["weakest"][str(groups)] = dict(ms=ms, ms_all=all_ms, over_decode=ms / decode_ms)
    return out


def stream_leg(q, epochs, ask, scales, max_rounds):
    rng = np.random.default_rng(3)
    kb = [int(rng.integers(28000, 32001)) if rng.random() < 0.5 else int(rng.integers(52000, 57001)) for _ in range(epochs)]      # two mother sizes
    qb = [float(x) for x in rng.uniform(0.01, 0.05, epochs)]
    keys, bobs = [], []
    for n, p in zip(kb, qb):
        a = rng.integers(0, 2, n).astype(np.uint8)
        keys.append(q.pack_bits(a))
        bobs.append(q.pack_bits(a ^ (rng.random(n) < p)))
    total = float(sum(kb))
    base_gap = 0.05                                                  # the min-sum family's default (qldpc.h: rate_gap)
    out = {}
    for sc in scales:
        r = q.Recon(max_blocks=64, rate_gap=base_gap * sc)
        msgs, pars = r.encode_blocks(keys, kb, qb)
        r.decode_blocks(bobs, kb, qb, msgs, pars)                    # warm-up: codes, decoders, first launches
        # the existing path: first decode, then the withheld parity bits
        t0 = time.perf_counter()
        st, fixed, co, it = r.decode_blocks(bobs, kb, qb, msgs, pars)
        leak = [r.leaked_bits(m) for m in msgs]
        failed = [i for i in range(epochs) if st[i] != 0]
        left = list(failed)
        if failed:
            second = [r.encode_planned(keys[i], kb[i], msgs[i], 0) for i in failed if msgs[i].n_punct > 0]
            idx = [i for i in failed if msgs[i].n_punct > 0]
            if idx:
                st2, _, _, _ = r.decode_blocks([bobs[i] for i in idx], [kb[i] for i in idx], [qb[i] for i in idx], [m for m, _ in second], [p for _, p in second])
                for t, i in enumerate(idx):
                    leak[i] = r.leaked_bits(second[t][0])
                    if st2[t] == 0:
                        left.remove(i)
        parent = dict(wall_ms=(time.perf_counter() - t0) * 1e3, first_round_failures=len(failed), unreconciled=len(left), leak_per_key_bit=sum(leak) / total)
        # blind rounds
        t0 = time.perf_counter()
        known = [(np.zeros(0, np.int32), np.zeros(0, np.uint8)) for _ in range(epochs)]
        open_, rounds, asked = list(range(epochs)), np.zeros(epochs, np.int32), 0
        leak = [0] * epochs
        for _ in range(max_rounds + 1):
            st, fixed, co, it, lk, asks = r.decode_blind([bobs[i] for i in open_], [kb[i] for i in open_], [qb[i] for i in open_], [msgs[i] for i in open_],
                                                         [pars[i] for i in open_], [known[i] for i in open_], ask)
            nxt = []
            for t, i in enumerate(open_):
                leak[i] = int(lk[t])
                if st[t] == 0:
                    continue
                known[i] = (np.concatenate([known[i][0], asks[t]]).astype(np.int32), np.concatenate([known[i][1], q.recon_disclose(keys[i], kb[i], asks[t])]))
                asked += int(asks[t].size)
                rounds[i] += 1
                nxt.append(i)
            open_ = nxt
            if not open_:
                break
        blind = dict(wall_ms=(time.perf_counter() - t0) * 1e3, rounds_histogram=np.bincount(rounds).tolist(), bits_asked=asked, unreconciled=len(open_),
                     leak_per_key_bit=sum(leak) / total)
        out["%.2f" % sc] = dict(rate_gap=base_gap * sc, parent_path=parent, blind=blind)
    return dict(workload="%d blocks of 28 000 .. 32 000 or 52 000 .. 57 000 bits, QBER 1 .. 5 %% per block (known exactly), sessions with max_blocks 64, %d bits a request, "
                         "at most %d requests" % (epochs, ask, max_rounds), settings=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "blind_cost.json"))
    ap.add_argument("--qber", type=float, default=0.03)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=96)
    ap.add_argument("--ask", type=int, default=64)
    ap.add_argument("--max-rounds", type=int, default=12)
    ap.add_argument("--legs", default="kernel,stream")
    args = ap.parse_args()
    import torch

    import _qldpc_loader
    q = _qldpc_loader.load()
    out = {}
    if "kernel" in args.legs:
        out["kernel"] = kernel_leg(q, torch, args.qber, args.reps)
        json.dump(out, open(args.out, "w"), indent=1)
    if "stream" in args.legs:
        out["stream"] = stream_leg(q, args.epochs, args.ask, (1.0, 0.75, 0.5), args.max_rounds)
    json.dump(out, open(args.out, "w"), indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
