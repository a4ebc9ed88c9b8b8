#!/usr/bin/env python3
"""What the keyed tag inside Bob's verify step (qldpc_recon_decode_blocks_tagged) costs beside the two-step way -- qldpc_recon_decode_blocks, then
qldpc_polyhash_blocks on the keys it returned, which uploads them a second time -- on a call shaped like the config-3 stream of bench.py: 512 blocks of
52 429 bits, QBER ~ U[0.5 %, 6 %], the four table rates, one session with max_blocks = 512:

    timeout -k 10 600 python tools/recon_tag_cost.py --out profiles/recon_tag_cost.json

Per r of --keys the wall time of the C calls (arguments marshalled outside, each call returns when its results are in place) for the tagged call, for the
plain decode and for the plain decode followed by the polyhash call, on the same blocks in the same process, alternating, --reps times each: medians, the
spread of each, and their ratios; and whether the tags of the two ways are equal.
No threshold and no claim: the file is the measurement.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BLOCKS, KEY_BITS = 512, 52429


def measure(q, keys, reps):
    rng = np.random.default_rng(42)
    true_q = rng.uniform(0.005, 0.06, BLOCKS).astype(np.float32)
    alice = rng.integers(0, 2, (BLOCKS, KEY_BITS)).astype(np.uint8)
    bob = alice ^ (rng.random((BLOCKS, KEY_BITS)) < true_q[:, None])
    aw, bw = q.pack_bits(alice), q.pack_bits(bob)
    r = q.Recon(max_blocks=BLOCKS)
    kb = [KEY_BITS] * BLOCKS
    msgs, pars = r.encode_blocks([aw[i] for i in range(BLOCKS)], kb, true_q)
    plain = r.prepare_decode([bw[i] for i in range(BLOCKS)], kb, true_q, msgs, pars)
    plain.run()                                                                            # warm-up: Bob's decoders
    L, ip, fp, up = q._L, C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    out = dict(workload="%d blocks of %d bits, QBER ~ U[0.005, 0.06], one session, max_blocks %d, defaults otherwise; one hash-key row shared by the blocks"
                        % (BLOCKS, KEY_BITS, BLOCKS), keys={})
    for n_keys in keys:
        hk = rng.integers(0, 1 << 32, 2 * n_keys, dtype=np.uint64).astype(np.uint32)
        tags, tags2 = np.zeros((BLOCKS, 2 * n_keys), np.uint32), np.zeros((BLOCKS, 2 * n_keys), np.uint32)
        hp = (up * BLOCKS)(*[hk.ctypes.data_as(up)] * BLOCKS)
        tp = (up * BLOCKS)(*[tags[i].ctypes.data_as(up) for i in range(BLOCKS)])
        tp2 = (up * BLOCKS)(*[tags2[i].ctypes.data_as(up) for i in range(BLOCKS)])
        ph = q.PolyHash(max_blocks=BLOCKS, max_key_bits=KEY_BITS, n_keys=n_keys)

        def tagged_call():
            """the one C call on the buffers of `plain`, nothing else in the timed region"""
            plain.reset()
            t = time.perf_counter()
            rc = L.qldpc_recon_decode_blocks_tagged(r._h, BLOCKS, plain._kp, plain._kb.ctypes.data_as(ip), plain._qb.ctypes.data_as(fp), plain._msgs, plain._pp, n_keys, hp, tp,
                                                    plain.status.ctypes.data_as(ip), plain.corrected.ctypes.data_as(ip), plain.iterations.ctypes.data_as(ip))
            dt = time.perf_counter() - t
            if rc:
                raise RuntimeError("qldpc_recon_decode_blocks_tagged: %d %s" % (rc, L.qldpc_last_error().decode()))
            return dt

        def two_step_call():
            """decode_blocks, then the polyhash context on the keys it returned: -> (both calls, the decode alone)"""
            plain.reset()
            t = time.perf_counter()
            plain.run()
            t1 = time.perf_counter()
            rc = L.qldpc_polyhash_blocks(ph._h, BLOCKS, plain._kp, plain._kb.ctypes.data_as(ip), hp, tp2)
            t2 = time.perf_counter()
            if rc:
                raise RuntimeError("qldpc_polyhash_blocks: %d %s" % (rc, L.qldpc_last_error().decode()))
            return t2 - t, t1 - t

        tagged_call(); two_step_call()                                                     # warm-up
        t_tag, t_two, t_dec = [], [], []
        for _ in range(reps):                                                              # alternating: other work shares the machine
            t_tag.append(tagged_call())
            st_tag, tg = plain.status.copy(), tags.copy()
            both, dec = two_step_call()
            t_two.append(both); t_dec.append(dec)
        ok = plain.status == 0
        out["keys"]["r%d" % n_keys] = dict(
            n_keys=n_keys, tagged_ms=sorted(1e3 * x for x in t_tag), two_step_ms=sorted(1e3 * x for x in t_two), decode_blocks_ms=sorted(1e3 * x for x in t_dec),
            tagged_median_ms=1e3 * float(np.median(t_tag)), two_step_median_ms=1e3 * float(np.median(t_two)), decode_blocks_median_ms=1e3 * float(np.median(t_dec)),
            tagged_over_decode_blocks=float(np.median(t_tag) / np.median(t_dec)), tagged_over_two_step=float(np.median(t_tag) / np.median(t_two)),
            blocks_ok=int(ok.sum()), same_status=bool((st_tag == plain.status).all()), tags_equal_on_ok_blocks=bool((tg[ok] == tags2[ok]).all()),
            tags_zero_on_failed_blocks=bool(not tg[~ok].any()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recon_tag_cost.json"))
    ap.add_argument("--keys", type=int, nargs="+", default=[1, 2])
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import _qldpc_loader
    q = _qldpc_loader.load()
    out = measure(q, args.keys, args.reps)
    out["what"] = ("the keyed tag inside the verify step of a reconciliation session on a config-3-like call: qldpc_recon_decode_blocks_tagged beside qldpc_recon_decode_blocks "
                   "followed by qldpc_polyhash_blocks on the returned keys, the same blocks in one process, alternating, wall time of the C calls")
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
