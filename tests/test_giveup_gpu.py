"""Early exit that gives up on frames whose syndrome weight has stopped falling (qldpc_decoder_cfg.giveup_patience, csrc/qldpc_kernels_giveup.h) --
GPU parity (-m gpu).  Everything compares exactly with tests/giveup_ref.py: the CPU oracle's trajectory of the batch and the rule restated in
Python.  PEGReg504x1008, NMS 0.75, 30 iterations, BSC at 0.07; 576 frames (9 groups of 64: one XCD per group) and their first 130 (3 groups,
the last with 2 frames: round-robin placement); M = 504 is no multiple of the 256-thread workgroup.  Every test asserts on the REFERENCE that
its frames hold converged, given-up and ran-out frames and a false give-up before it looks at the device.
"""
import numpy as np
import pytest

import giveup_ref as R
import mc_ref
from mc_blind_ref import got_rows
from mc_oracle import SEED, bsc_llrs, setups  # noqa: F401 (setups is a fixture)

pytestmark = pytest.mark.gpu
FIELDS = ("hard", "iters", "ok", "gave", "last", "best")

# name -> (trajectory kind, patience, decoder arguments)
CASES = {
    "flood_v1": ("flood", 6, dict(frames_per_lane=1)),
    "flood_v2": ("flood", 6, dict(frames_per_lane=2)),
    "flood_v4": ("flood", 6, dict(frames_per_lane=4)),
    "flood_f16": ("flood_f16", 6, dict(msg_dtype="f16")),
    "flood_i8": ("flood_i8", 6, dict(msg_dtype="i8")),
    "hlay_cst": ("hlay", 8, dict(schedule="hlayered")),                          # the compressed check state
    "hlay_chain": ("hlay", 8, dict(schedule="hlayered", layer_chain="on")),      # the one-launch sweep on explicit messages
    # patience 10: the smallest of 3 .. 14 at which the reference's 130 frames hold every outcome (97 / 31 / 2; the 576: 431 / 132 / 13 and 3 false
    # give-ups).  No patience gives the 130 frames a false give-up as well, so that one case asserts the three outcomes only
    "hlay_i8": ("hlay_i8", 10, dict(schedule="hlayered", msg_dtype="i8")),
}


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def i32(a):
    return np.ascontiguousarray(a).view(np.int32)


def decoder(q, F, patience, **kw):
    code = R.code(q)
    return q.Decoder(code, code.N, R.N_ITE, rule="NMS", rule_param=0.75, n_frames=F, giveup=patience, **kw)


def run(q, torch, dec, y, form="llr", target=None, load=True):
    if load and form == "llr":
        dec.load_llr(torch.from_numpy(R.llr_of(y)).cuda())
    elif load:
        dec.load_bits(torch.from_numpy(i32(q.pack_bits(y))).cuda(), torch.from_numpy(np.full(len(y), R.MAG, np.float32)).cuda())
    if load and target is not None:
        dec.load_syndrome(torch.from_numpy(i32(q.pack_bits(target))).cuda())
    dec.run()
    it, ok = dec.fetch_status()
    out = dict(hard=q.unpack_bits(dec.fetch_packed().cpu().numpy().view(np.uint32), dec.N), iters=it.cpu().numpy(), ok=ok.cpu().numpy())
    if dec.giveup:
        out.update(zip(("gave", "last", "best"), (t.cpu().numpy() for t in dec.fetch_giveup())))
    return out


def same(got, exp, fields=FIELDS):
    for k in fields:
        bad = np.nonzero((got[k] != exp[k]).reshape(len(exp[k]), -1).any(1))[0]
        assert bad.size == 0, (k, bad[:8], got[k][bad[:8]], exp[k][bad[:8]])


def reference(q, O, kind, patience, F, depth=1, full_mix=True):
    R.graphs(q, O)
    exp = R.expected(R.trajectory(q, O, kind), patience, depth, frames=np.arange(F))
    counts = np.bincount(exp["outcome"], minlength=3)
    print(kind, patience, F, "converged / given up / ran out", counts, "false give-ups", int(exp["false"].sum()), "iteration sum", int(exp["iters"].sum()))
    if full_mix:
        R.assert_mix(exp)
    else:
        assert (counts >= 1).all(), counts
    return exp


# ---- 1. exactness ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["llr", "bits"])
@pytest.mark.parametrize("F", [R.SMALL, R.LARGE])
@pytest.mark.parametrize("case", sorted(CASES))
def test_run_equals_the_reference(q, O, torch, case, F, form):
    kind, patience, kw = CASES[case]
    exp = reference(q, O, kind, patience, F, full_mix=not (case == "hlay_i8" and F == R.SMALL))
    dec = decoder(q, F, patience, **kw)
    same(run(q, torch, dec, R.flips()[:F], form), exp)


# ---- 2. syndrome form, 3. syndrome_depth = 2 ------------------------------------------------------------------------------------------

def test_syndrome_form(q, O, torch):
    F = R.SMALL
    _, og, _, _ = R.graphs(q, O)
    rng = np.random.default_rng(5)
    xa = (rng.random((F, og.N)) < 0.5).astype(np.uint8)
    s = np.stack([og.syndrome(x)[1] for x in xa]).astype(np.uint8)
    y = xa ^ R.flips()[:F]
    exp = R.expected(R.trajectory(q, O, "flood", llr=R.llr_of(y), target=s.astype(np.int32)), 6)
    R.assert_mix(exp)
    assert exp["ok"].sum() > 0 and (exp["hard"][exp["ok"] == 1] == xa[exp["ok"] == 1]).all()      # what converges is Alice's word
    same(run(q, torch, decoder(q, F, 6), y, target=s), exp)


def test_syndrome_depth_two(q, O, torch):
    F = R.SMALL
    exp = reference(q, O, "flood", 6, F, depth=2)
    assert (exp["iters"] != reference(q, O, "flood", 6, F)["iters"]).any()
    same(run(q, torch, decoder(q, F, 6, syndrome_depth=2), R.flips()[:F]), exp)


# ---- 4. compaction ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["flood_v1", "hlay_cst"])
def test_compacted_run_equals_the_reference_and_the_uncompacted_run(q, O, torch, case):
    kind, patience, kw = CASES[case]
    F = R.LARGE
    exp = reference(q, O, kind, patience, F)
    out = {}
    for mode in ("off", "on"):
        dec = decoder(q, F, patience, compact=mode, **kw)
        out[mode] = run(q, torch, dec, R.flips()[:F])
        st = dec.last_run_stats()
        print(case, mode, st)
        same(out[mode], exp)
        assert (st["compactions"] >= 1) == (mode == "on"), st
        if mode == "on":      # ... and once more: the fetch reads every generation again
            same(dict(zip(("gave", "last", "best"), (t.cpu().numpy() for t in dec.fetch_giveup()))), exp, ("gave", "last", "best"))
    same(out["on"], out["off"])


# ---- 5. frozen messages: the posteriors of a frame given up are the ones it stopped with ------------------------------------------------------------

def test_frozen_messages_keep_the_posteriors_of_a_frame_given_up(q, O, torch):
    F = R.SMALL
    exp = reference(q, O, "flood", 6, F)
    traj = R.trajectory(q, O, "flood")
    dec = decoder(q, F, 6, freeze_messages=True)
    same(run(q, torch, dec, R.flips()[:F]), exp)
    post = dec.fetch_post().cpu().numpy()
    for f in np.nonzero(exp["gave"])[0]:
        assert (post[f].view(np.uint32) == traj["post"][exp["iters"][f] - 1, f].view(np.uint32)).all(), f


# ---- 6. counting only ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["flood_v1", "hlay_cst"])
def test_patience_of_n_ite_only_counts(q, O, torch, case):
    kind, _, kw = CASES[case]
    F = R.SMALL
    reference(q, O, kind, CASES[case][1], F)
    exp = R.expected(R.trajectory(q, O, kind), R.N_ITE, frames=np.arange(F))
    got = run(q, torch, decoder(q, F, R.N_ITE, **kw), R.flips()[:F])
    off = run(q, torch, decoder(q, F, 0, **kw), R.flips()[:F])
    same(got, off, ("hard", "iters", "ok"))
    assert not got["gave"].any() and (exp["last"] > 0).any() and (exp["best"] < exp["last"]).any()
    same(got, exp)


# ---- 7. reuse --------------------------------------------------------------------------------------------------------------------------

def test_decoder_is_reusable(q, O, torch):
    F = R.SMALL
    exp = reference(q, O, "flood", 6, F)
    dec = decoder(q, F, 6)
    same(run(q, torch, dec, R.flips()[:F]), exp)
    same(run(q, torch, dec, R.flips()[:F], load=False), exp)
    same(run(q, torch, dec, R.flips()[:70]), {k: v[:70] for k, v in exp.items()})
    assert dec.giveup_total() == 2 * int(exp["gave"].sum()) + int(exp["gave"][:70].sum())      # every run since the decoder was created
    assert decoder(q, F, 0).giveup_total() == 0


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------------

def refused(q, status, words, call):
    """the call is refused with that status and a message that names the remedy"""
    with pytest.raises(q.QldpcError) as e:
        call()
    assert e.value.status == status, str(e.value)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_refusals(q, torch, setups):
    refused(q, -7, ["engine = FRAMES"], lambda: decoder(q, 4, 6, engine="edges"))
    refused(q, -1, ["enable_syndrome = 1"], lambda: decoder(q, 64, 6, enable_syndrome=False))
    refused(q, -7, ["QLDPC_SCHED_HLAYERED", "QLDPC_SCHED_FLOODING"], lambda: decoder(q, 64, 6, schedule="vlayered"))
    refused(q, -1, ["giveup_patience"], lambda: decoder(q, 64, -1))
    members = [decoder(q, 64, 0, schedule="hlayered", compact="off"), decoder(q, 64, 6, schedule="hlayered", compact="off")]
    assert q.DecoderGang(members[:1]) is not None
    refused(q, -7, ["member 1", "giveup_patience = 0"], lambda: q.DecoderGang(members))
    refused(q, -7, ["giveup_patience >= 1"], lambda: decoder(q, 64, 0).fetch_giveup())
    refused(q, -8, ["qldpc_run"], lambda: decoder(q, 64, 6).fetch_giveup())
    assert decoder(q, 4, 6, engine="auto") is not None      # auto picks FRAMES for a batch the edge engine would have taken
    s = setups("peg")
    loose = q.Decoder(s.code, s.K, R.N_ITE, info_bits_pos=s.pos, rule="NMS", rule_param=0.75, n_frames=64, giveup=6, compact="off")
    refused(q, -7, ["freeze_messages = 1"], lambda: q.MonteCarlo(loose, s.enc, seed=SEED, batch=64).blind(0.26, 8, 2, 0, 64))


# ---- 9. Monte-Carlo ------------------------------------------------------------------------------------------------------------------------

def mc_decoder(q, s, F):
    return q.Decoder(s.code, s.K, R.N_ITE, info_bits_pos=s.pos, rule="NMS", rule_param=0.75, n_frames=F, giveup=6, freeze_messages=True, compact="off")


def test_blind_rounds_do_not_depend_on_the_pooling(q, setups):
    s = setups("peg")
    res, opened = {}, {}
    for batch in (64, 256):
        mc = q.MonteCarlo(mc_decoder(q, s, batch), s.enc, seed=SEED, batch=batch)
        res[batch] = mc.blind(0.26, 8, 3, 0, 512)
        opened[batch] = mc.blind_open()
    a, b = res[64], res[256]
    print(got_rows(a), a["disclosed"], a["decodes"], a["open"])
    assert got_rows(a) == got_rows(b) and a["frames"] == b["frames"] == 512
    assert all(r["frames"] > 0 for r in got_rows(a))
    for k in ("disclosed", "decodes", "open", "frame_errors", "undetected"):
        assert a[k] == b[k], k
    assert (opened[64][0] == opened[256][0]).all() and (opened[64][1] == opened[256][1]).all() and opened[64][0].size == a["open"]


def test_monte_carlo_run_counts_the_frames_given_up(q, O, setups):
    s = setups("peg")
    n, qber = 256, 0.26
    info_w, flip_w = q.mc_frames_host(s.K, s.N, SEED, qber, 0, n, info_bits_pos=s.pos)
    cw = s.codewords(info_w)
    llr = bsc_llrs(q, cw ^ mc_ref.unpack(flip_w, s.N), s.cls, qber)
    exp = R.expected(R.trajectory(q, O, "flood", llr=llr, graphs_of=(s.og, s.ogl, s.code.layer_order()[0])), 6)
    R.assert_mix(exp)
    be = (exp["hard"][:, s.pos] != cw[:, s.pos]).sum(1)
    print("converged / given up / ran out", np.bincount(exp["outcome"], minlength=3), "frames not ok", int((exp["ok"] == 0).sum()), "frame errors", int((be > 0).sum()))
    res = q.MonteCarlo(mc_decoder(q, s, n), s.enc, seed=SEED, batch=n).run(qber, 0, n)
    # frames with ok = 0 are the loop's not_converged; its frame errors are the frames with a wrong information bit (with the all-zero codeword
    # and info_bits_pos = 0 .. K - 1 on the CPU: 128 / 103 / 25 frames, 127 of either kind)
    assert res["frames"] == n and res["not_converged"] == int((exp["ok"] == 0).sum()) and res["frame_errors"] == int((be > 0).sum())
    assert res["bit_errors"] == int(be.sum()) and res["iter_sum"] == int(exp["iters"].sum()) and res["undetected"] == 0
