#!/usr/bin/env python3
"""What the stages of a polar reconciliation session cost on the device: hipEvent ms per stage (median of 7 after a warm-up call, one process) at
N = 2^10 x 20 000 blocks in both message types around an SC context of the lanes' form and around a list-4 context with CRC 11, and at
N = 2^16 x 4 096 blocks, int8, SC lanes.  Stages: Alice's encode launch, her whole call (mask + encode + syndrome and crc; the syndrome stage is the
difference), Bob's prior, the bare decode of the same context on the rows the prior wrote, his verdict, and his whole call.  Bob's keys are
Alice's through a BSC of 2 %.  Writes profiles/polar_recon_cost.json.

    python tools/polar_recon_cost.py [--out profiles/polar_recon_cost.json] [--runs 7]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import _qldpc_loader  # noqa: E402
from polar_common import event_ms  # noqa: E402

SHAPES = [(10, 20000, "i8", 0), (10, 20000, "f32", 0), (10, 20000, "i8", 4), (10, 20000, "f32", 4), (16, 4096, "i8", 0)]
CRC11 = (11, 0x621)
QBER = 0.02


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "polar_recon_cost.json"))
    ap.add_argument("--runs", type=int, default=7)
    args = ap.parse_args()
    import torch
    q = _qldpc_loader.load()
    rng = np.random.default_rng(1)
    vp = lambda t: q._vp(t.data_ptr())
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32) if a.dtype == np.uint32 else np.ascontiguousarray(a)).cuda()
    res = {"what": "hipEvent ms, median of %d after a warm-up call; syndrome_ms = alice_call_ms - encode_launch_ms (the mask and the syndrome / crc kernel); "
                   "not_decoder_share = 1 - decode_ms / bob_call_ms; Bob's keys are Alice's through a BSC of %g" % (args.runs, QBER), "shapes": {}}
    for n, B, messages, L in SHAPES:
        N, W = 1 << n, (1 << n) // 32
        pos = np.sort(q.polar_pw_order(n)[N // 2:]).astype(np.int32)
        sc = q.Polar(n, pos, messages, 31, max_frames=B)
        dec = q.PolarList(n, pos, messages, 31, L, *CRC11, max_frames=B) if L else sc
        sess = q.PolarRecon(dec, max_blocks=B) if L else q.PolarRecon(dec, *CRC11, max_blocks=B)
        alice = rng.integers(0, 1 << 32, (B, W), dtype=np.uint64).astype(np.uint32)
        flips = np.packbits(rng.random((B, N), dtype=np.float32) < QBER, axis=1, bitorder="big").view(">u4").astype(np.uint32)
        d_alice, d_bob, d_row = dev(alice), dev(alice ^ flips), dev(alice)
        mask, prefix, _ = q.polar_recon_tables(n, pos)
        d_mask, d_prefix = dev(mask), dev(prefix)
        syn, crc = sess.encode(d_alice)
        d_llr = torch.empty((B, N), dtype=torch.int8 if messages == "i8" else torch.float32, device="cuda")
        d_frozen = torch.empty((B, W), dtype=torch.int32, device="cuda")
        d_status, d_corrected = torch.empty(B, dtype=torch.int32, device="cuda"), torch.empty(B, dtype=torch.int32, device="cuda")
        stream = q._stream_arg(None, 0)

        def prior():
            q._chk(q._L.qldpc_polar_recon_prior_dev(stream, n, N - pos.size, vp(d_mask), vp(d_prefix), sc.messages, 31, sess.prior, sess.pin, B, vp(d_bob), None, vp(syn),
                                                    vp(d_llr), vp(d_frozen)), "prior")

        prior()
        want = ("info", "x", "pick") if L else ("info", "x")
        decode = (lambda: dec.decode(d_llr, d_frozen, crc, want=want)) if L else (lambda: dec.decode(d_llr, d_frozen, want=want))
        out = decode()

        def verdict():
            q._chk(q._L.qldpc_polar_recon_verdict_dev(stream, n, pos.size, CRC11[0], CRC11[1], B, vp(out["info"]), vp(out["x"]), vp(out["pick"]) if L else None, vp(d_bob), None,
                                                      vp(crc), vp(d_status), vp(d_corrected)), "verdict")

        row = {"log2_n": n, "blocks": B, "messages": messages, "list_size": L, "n_info": int(pos.size), "syndrome_words": sess.syndrome_words,
               "leaked_bits": sess.leaked_bits, "session_device_bytes": sess.device_bytes(), "context_device_bytes": dec.device_bytes(),
               "encode_launch_ms": event_ms(torch, lambda: sc.encode(d_row, out=d_row), args.runs),
               "alice_call_ms": event_ms(torch, lambda: sess.encode(d_alice), args.runs),
               "prior_ms": event_ms(torch, prior, args.runs),
               "decode_ms": event_ms(torch, decode, args.runs),
               "verdict_ms": event_ms(torch, verdict, args.runs),
               "bob_call_ms": event_ms(torch, lambda: sess.decode(d_bob, syn, crc), args.runs)}
        med = lambda k: row[k]["median"]
        row["syndrome_ms"] = med("alice_call_ms") - med("encode_launch_ms")
        row["not_decoder_share"] = 1.0 - med("decode_ms") / med("bob_call_ms")
        row["stages_over_decode"] = (row["syndrome_ms"] + med("prior_ms") + med("verdict_ms")) / med("decode_ms")
        row["ok_blocks"] = int((sess.decode(dev(alice ^ flips), syn, crc)["status"] == 0).sum().item())
        res["shapes"]["n=%d x %d %s %s" % (n, B, messages, "list %d" % L if L else "sc")] = row
        print(json.dumps({k: (round(med(k), 4) if isinstance(row[k], dict) else row[k]) for k in row}), flush=True)
        del sess, dec, sc, d_llr, d_frozen, out
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
