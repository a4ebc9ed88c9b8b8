#!/usr/bin/env python3
"""What guessing rounds inside a reconciliation session (qldpc_recon_decode_guess) buy and cost beside qldpc_recon_decode_blocks, on a call shaped like the
config-3 stream of bench.py: 512 blocks of 52 429 bits, QBER ~ U[0.5 %, 6 %], the four table rates, one session with max_blocks = 512 -- and --low of the
blocks (about 2 %) planned for a QBER --under times their true one, so that their first decode is likely to fail (one measurement per value of --under:
far under its QBER a block is beyond any guess, close to it a few guessed bits can tip the decode):

    timeout -k 10 900 python tools/recon_guess_cost.py --out profiles/recon_guess_cost.json

blocks: per g of --bits the wall time of the one C call (arguments marshalled outside, the call returns when the results are in place) for decode_blocks and
        for decode_guess on the same blocks in the same process, alternating, --reps times each: medians, the spread of each, and their ratio;
        blocks failed at once, rescued, still failed, wrong or ambiguous rescues, trials run and their mean iteration count.
second: what a second round with the withheld parity (encode_planned with n_punct = 0 + decode) would have leaked on top for the same failed blocks, and
        how many of them it recovers.  Guessing leaks nothing.
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


def measure(q, bits, reps, low, under):
    rng = np.random.default_rng(42)
    true_q = rng.uniform(0.005, 0.06, BLOCKS).astype(np.float32)
    plan_q = true_q.copy()
    too_low = rng.choice(BLOCKS, low, replace=False)
    plan_q[too_low] *= under
    alice = rng.integers(0, 2, (BLOCKS, KEY_BITS)).astype(np.uint8)
    bob = alice ^ (rng.random((BLOCKS, KEY_BITS)) < true_q[:, None])
    aw, bw = q.pack_bits(alice), q.pack_bits(bob)
    r = q.Recon(max_blocks=BLOCKS)
    kb = [KEY_BITS] * BLOCKS
    msgs, pars = r.encode_blocks([aw[i] for i in range(BLOCKS)], kb, plan_q)
    plain = r.prepare_decode([bw[i] for i in range(BLOCKS)], kb, plan_q, msgs, pars)
    plain.run()                                                                            # warm-up: Bob's decoders
    guess = np.zeros(BLOCKS, q.RECON_GUESS_DTYPE)
    L, ip, fp = q._L, C.POINTER(C.c_int), C.POINTER(C.c_float)

    def guess_call(g):
        """the one C call on the buffers of `plain`, nothing else in the timed region"""
        plain.reset()
        t = time.perf_counter()
        rc = L.qldpc_recon_decode_guess(r._h, BLOCKS, plain._kp, plain._kb.ctypes.data_as(ip), plain._qb.ctypes.data_as(fp), plain._msgs, plain._pp, g,
                                        C.c_void_p(guess.ctypes.data), plain.status.ctypes.data_as(ip), plain.corrected.ctypes.data_as(ip),
                                        plain.iterations.ctypes.data_as(ip))
        dt = time.perf_counter() - t
        if rc:
            raise RuntimeError("qldpc_recon_decode_guess: %d %s" % (rc, L.qldpc_last_error().decode()))
        return dt

    def plain_call():
        plain.reset()
        t = time.perf_counter()
        plain.run()
        return time.perf_counter() - t

    plain_call()
    st0 = plain.status.copy()
    failed0 = np.flatnonzero(st0 != 0)
    groups = {}
    for m in msgs:
        groups[(int(m.rate_index), int(m.code_k), int(m.code_m))] = groups.get((int(m.rate_index), int(m.code_k), int(m.code_m)), 0) + 1
    out = dict(workload="%d blocks of %d bits, QBER ~ U[0.005, 0.06], %d of them planned for %.2f x their QBER, one session, max_blocks %d, defaults otherwise"
                        % (BLOCKS, KEY_BITS, low, under, BLOCKS),
               rate_groups={"rate %d K %d M %d" % k: v for k, v in sorted(groups.items())}, failed_first_decodes=int(failed0.size),
               failed_of_the_blocks_planned_too_low=int(np.isin(failed0, too_low).sum()), guess={})
    for g in bits:
        guess_call(g)                                                                      # warm-up: the pools of the entries
        t_plain, t_guess = [], []
        for _ in range(reps):                                                              # alternating: other work shares the machine
            t_plain.append(plain_call())
            t_guess.append(guess_call(g))
        st = plain.status.copy()
        tried = guess["tried"] == 1
        rescued = tried & (st == 0)
        wrong = int(sum(not (plain.keys[i] == aw[i]).all() for i in np.flatnonzero(st == 0)))
        trials = int(tried.sum()) << g
        out["guess"]["g%d" % g] = dict(
            guess_bits=g, trials_per_failed_block=1 << g, decode_blocks_ms=sorted(1e3 * x for x in t_plain), decode_guess_ms=sorted(1e3 * x for x in t_guess),
            decode_blocks_median_ms=1e3 * float(np.median(t_plain)), decode_guess_median_ms=1e3 * float(np.median(t_guess)),
            guess_over_blocks=float(np.median(t_guess) / np.median(t_plain)), tried=int(tried.sum()), rescued=int(rescued.sum()), still_failed=int((tried & (st != 0)).sum()),
            wrong_keys_accepted=wrong, ambiguous=int(guess["ambiguous"].sum()), trials=trials, zero_syndrome_trials=int(guess["n_ok"].sum()),
            passing_trials=int(guess["n_pass"].sum()), trial_iterations_mean=(float(guess["trial_iterations"].sum()) / trials) if trials else None,
            leaked_bits_added=0)
    # the other remedy: the withheld parity of the same failed blocks
    extra, recovered = 0, 0
    for i in failed0:
        if msgs[i].n_punct == 0:
            continue
        m2, p2 = r.encode_planned(aw[i], KEY_BITS, msgs[i], 0)
        good, fixed, _, _, _ = r.decode(bw[i], KEY_BITS, float(plan_q[i]), m2, p2)
        extra += q.Recon.leaked_bits(m2) - q.Recon.leaked_bits(msgs[i])
        recovered += bool(good and (fixed == aw[i]).all())
    out["second_round_with_withheld_parity"] = dict(blocks=int(failed0.size), recovered=int(recovered), leaked_bits_added=int(extra),
                                                    leaked_bits_added_per_block=(extra / failed0.size) if failed0.size else None, round_trips_added=1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recon_guess_cost.json"))
    ap.add_argument("--bits", type=int, nargs="+", default=[0, 4, 8])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--low", type=int, default=10, help="blocks planned too low (10 of 512 is about one in fifty)")
    ap.add_argument("--under", type=float, nargs="+", default=[0.8, 0.84, 0.86, 0.88, 0.9, 0.95], help="their planned QBER over their true one, a measurement per value")
    args = ap.parse_args()
    import _qldpc_loader
    q = _qldpc_loader.load()
    out = dict(points={"under %.2f" % u: measure(q, args.bits, args.reps, args.low, u) for u in args.under})
    out["what"] = ("guessing rounds in a reconciliation session on a config-3-like call: qldpc_recon_decode_guess beside qldpc_recon_decode_blocks on the same blocks in one "
                   "process, alternating, wall time of the C call; blocks rescued, trials run, and the leak a second round with the withheld parity would have added")
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
