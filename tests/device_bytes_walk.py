"""What every *_device_bytes getter of libqldpc reports along the life of its context: walk(q) builds each kind of context at the smallest shapes
that reach every allocation path, makes the calls that allocate lazily, and returns {step name: device_bytes}.  It uses the package alone, so it
runs on any build of the library (QLDPC_LIB): tests/golden/device_bytes.json is its output on the library of the commit before the contexts moved
to one allocation ledger (csrc/qldpc_devmem.h), and tests/test_device_bytes_gpu.py holds every later build to those numbers.

    python tests/device_bytes_walk.py --out FILE

No step reads a count after an early-exit run with compaction on: how many generations such a run opens depends on when the host polls."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEG = os.path.join(ROOT, "tests", "golden", "PEGReg504x1008.alist")

# (schedule, message types the schedule takes)
DECODERS = (("flooding", ("f32", "f16", "i8")), ("hlayered", ("f32", "i8")), ("vlayered", ("f32",)))
CRC11 = (11, 0x621)


def _bytes(ctx):
    """device_bytes is a property of some classes and a method of the others"""
    v = ctx.device_bytes
    return int(v() if callable(v) else v)


def _decoder_steps(q, torch, out, name, dec, F):
    """after create, then after each call that allocates on first use, in turn"""
    Wn, Wm = (dec.N + 31) // 32, (dec.code.M + 31) // 32
    dev = "cuda:%d" % dec.device
    rows = torch.zeros((F, Wn), dtype=torch.int32, device=dev)
    out[name + "/create"] = _bytes(dec)
    dec.load_bits(rows, torch.full((F,), 2.0, dtype=torch.float32, device=dev), torch.zeros(dec.N, dtype=torch.uint8, device=dev))
    out[name + "/load_bits"] = _bytes(dec)
    dec.load_erasures(rows)
    out[name + "/load_erasures"] = _bytes(dec)
    dec.load_known(rows, rows)
    out[name + "/load_known"] = _bytes(dec)
    dec.load_syndrome(torch.zeros((F, Wm), dtype=torch.int32, device=dev))
    out[name + "/load_syndrome"] = _bytes(dec)
    q._chk(q._L.qldpc_decoder_reserve(dec._h), "reserve")
    out[name + "/reserve"] = _bytes(dec)
    dec.run()                                # the all-zero word at |LLR| 2 and syndrome 0; fewer than four groups, so nothing compacts
    dec.fetch_post()
    dec.sync()
    out[name + "/fetch_post"] = _bytes(dec)


def _walk_decoders(q, torch, out):
    code = q.Code.from_alist(PEG)
    for schedule, dtypes in DECODERS:
        for dtype in dtypes:
            for F in (64, 65):
                dec = q.Decoder(code, 504, 10, rule="NMS", rule_param=0.75, n_frames=F, schedule=schedule, msg_dtype=dtype, engine="frames")
                _decoder_steps(q, torch, out, "decoder/%s/%s/%d" % (schedule, dtype, F), dec, F)
    dec = q.Decoder(code, 504, 10, rule="NMS", rule_param=0.75, n_frames=64, engine="frames")      # reserve() before any load: the erasure ballots are its own to allocate
    out["decoder/reserve_first/create"] = _bytes(dec)
    q._chk(q._L.qldpc_decoder_reserve(dec._h), "reserve")
    out["decoder/reserve_first/reserve"] = _bytes(dec)
    for F in (1, 8):
        dec = q.Decoder(code, 504, 10, rule="NMS", rule_param=0.75, n_frames=F, engine="edges")
        _decoder_steps(q, torch, out, "decoder/edges/%d" % F, dec, F)
    ira = q.Code.ira(1024, 512)
    dec = q.Decoder(ira, 512, 50, rule="NMS", rule_param=0.75, n_frames=64, enable_syndrome=False, engine="frames")      # the posterior form
    assert dec.flood_post
    _decoder_steps(q, torch, out, "decoder/flood_post/64", dec, 64)


def _walk_mc(q, out):
    code = q.Code.ira(1024, 512)
    enc = q.Encoder(code, "IRA")
    dec = q.Decoder(code, enc.K, 20, info_bits_pos=enc.info_bits_pos, rule="NMS", rule_param=0.75, n_frames=64, engine="frames")
    mc = q.MonteCarlo(dec, enc, seed=3, batch=64)
    out["mc/create"] = _bytes(mc)
    mc.set_puncture([1000, 1010])
    mc.search(0.02, 4, 8)
    out["mc/puncture_search"] = _bytes(mc)
    mc.set_puncture([])
    mc.sweep((0.02, 0.03))
    out["mc/sweep"] = _bytes(mc)
    mc.strata((5, 10), 0.02)
    out["mc/strata"] = _bytes(mc)
    mc.blind(0.05, 8, 1)
    out["mc/blind_1"] = _bytes(mc)
    mc.blind(0.05, 8, 3)                     # the pools grow, the old ones are released
    out["mc/blind_3"] = _bytes(mc)
    mc.guess(0.05, 2)
    out["mc/guess_2"] = _bytes(mc)
    mc.set_awgn(sigma=0.8)
    out["mc/set_awgn"] = _bytes(mc)
    mc.sweep_tables([q.mc_awgn_table(0.8), q.mc_awgn_table(0.9)])
    out["mc/sweep_tables_2"] = _bytes(mc)
    out["mc/decoder"] = _bytes(dec)          # what the loop's calls reserved in its decoder


def _walk_qber(q, out):
    est = q.QberEstimator(q.Code.ira(1024, 512), 4)
    out["qber/create"] = _bytes(est)
    est.set_merge(True)
    out["qber/set_merge"] = _bytes(est)


def _walk_hashes(q, out):
    out["privamp/create"] = _bytes(q.PrivAmp(max_blocks=2, max_key_bits=1000, max_final_bits=1000))
    out["toeplitz/direct/create"] = _bytes(q.Toeplitz(max_blocks=2, max_key_bits=1000, max_out_bits=1000))
    out["toeplitz/ntt/create"] = _bytes(q.Toeplitz(max_blocks=2, max_key_bits=16, max_out_bits=16, method="ntt"))      # L = 32, the shortest transform
    out["polyhash/create"] = _bytes(q.PolyHash(max_blocks=2, max_key_bits=1000))


def _walk_polar(q, out):
    pos8, pos14 = q.polar_pw_order(8)[128:], q.polar_pw_order(14)[1 << 13:]
    lanes = q.Polar(8, pos8, "i8", 31, max_frames=70)
    out["polar/lanes/i8/create"] = _bytes(lanes)
    out["polar/lanes/f32/create"] = _bytes(q.Polar(8, pos8, "f32", 31, max_frames=70))
    out["polar/wide/create"] = _bytes(q.Polar(14, pos14, "i8", 31, max_frames=3, form="wide"))
    plist = q.PolarList(8, pos8, "i8", 31, 4, *CRC11, max_frames=64)
    out["polar_list/create"] = _bytes(plist)
    wide = q.Polar(14, pos14, "i8", 31, max_frames=64, form="wide")
    for name, ctx in (("lanes", lanes), ("wide", wide), ("list", plist)):      # around the lanes' form the loop has the tally accumulator
        out["polar_mc/%s/create" % name] = _bytes(q.PolarMonteCarlo(ctx, seed=1, batch=64))


def walk(q):
    """{step name: device_bytes}, in the order of the walk"""
    import torch
    out = {}
    _walk_decoders(q, torch, out)
    _walk_mc(q, out)
    _walk_qber(q, out)
    _walk_hashes(q, out)
    _walk_polar(q, out)
    torch.cuda.synchronize()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", required=True, help="the JSON file to write")
    args = ap.parse_args()
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import _qldpc_loader
    counts = walk(_qldpc_loader.load())
    with open(args.out, "w") as f:
        json.dump(counts, f, indent=1)
        f.write("\n")
    print("%d steps, %d bytes in all" % (len(counts), int(np.sum(list(counts.values())))))
