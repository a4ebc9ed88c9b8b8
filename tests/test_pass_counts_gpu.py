"""GPU suite (-m gpu): the bookkeeping of an early-exit run on the FRAMES engine -- how many passes of each kind a run launches, what the
profile counts for them, and the iteration count it reports -- for the three schedules.

512 frames are eight 64-frame groups, the smallest batch at which the engine polls (every 2 iterations).  Frames 0-255 carry +4.0 everywhere
and converge at iteration 1; frames 256-511 are coin flips of +-1.0 and never converge in 6 iterations (CPU oracle, flooding and hlayered: 0 of
256).  So the poll after iteration 2 finds four of eight groups still running, and no later poll finds fewer.  The expected counts follow from
the loops of qldpc_engine.hip:

  flooding   check pass per iteration, variable-node pass FIRST + one between iterations + POST; after each of the first n_ite - 1
             iterations one syndrome and one status pass; the profile's bytes follow the lanes of the groups still running at each poll
  layered    after EVERY sweep: sign ballots (counted as a syndrome pass) + syndrome + status; with compaction off the live lanes are not tracked
  all        one status pass at run start (initialisation), one syndrome pass at run end (success flag)
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, E, F, ITE = 1008, 3024, 512, 6
PASS = {"flooding": "cn_update", "hlayered": "layer_update", "vlayered": "vn_vlayer"}


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def code(q, gold):
    c = q.Code.from_alist(os.path.join(gold, "PEGReg504x1008.alist"))
    assert (c.N, c.M, c.E) == (N, 504, E)
    return c


@pytest.fixture(scope="module")
def frames():
    clean = np.full((256, N), 4.0, np.float32)
    noise = np.where(np.random.default_rng(11).random((256, N)) < 0.5, -1.0, 1.0).astype(np.float32)
    return {"half": np.concatenate([clean, noise]), "clean": np.concatenate([clean, clean])}


def run(q, torch, code, schedule, llr, enable_syndrome=True):
    dec = q.Decoder(code, N, ITE, rule="NMS", rule_param=0.75, n_frames=F, schedule=schedule, engine="frames", compact="off", enable_syndrome=enable_syndrome)
    dec.profile(True)
    dec.load_llr(torch.from_numpy(llr).cuda())
    dec.run()
    it, ok = dec.fetch_status()
    st = {s["name"]: s for s in dec.profile_read()}
    print(schedule, "last_run_iterations", dec.last_run_iterations, {k: (v["launches"], v["alg_bytes"]) for k, v in st.items()})
    return dec, st, it.cpu().numpy(), ok.cpu().numpy()


def launches(st, name):
    return st[name]["launches"] if name in st else 0


@pytest.mark.parametrize("schedule", ["flooding", "hlayered", "vlayered"])
def test_pass_counts_half_the_batch_converges(q, torch, code, frames, schedule):
    dec, st, it, ok = run(q, torch, code, schedule, frames["half"])
    assert (ok[:256] == 1).all() and (it[:256] == 1).all()        # precondition: the clean half converges at iteration 1 ...
    assert (ok[256:] == 0).all()                                  # ... and none of the coin-flip frames does
    assert dec.last_run_iterations == ITE
    assert launches(st, PASS[schedule]) == ITE
    if schedule == "flooding":
        assert launches(st, "vn_update") == ITE + 1
        assert launches(st, "syndrome") == 6 and launches(st, "status") == 6
        assert st["cn_update"]["alg_bytes"] == 2.0 * E * 4 * (2 * 512 + 4 * 256)      # two iterations at 512 live lanes, four at 256
    else:
        assert launches(st, "vn_update") == 0 and launches(st, "cn_update") == 0
        assert launches(st, "syndrome") == 13 and launches(st, "status") == 7
        assert st[PASS[schedule]]["alg_bytes"] == ITE * 4.0 * E * 4 * 512              # compaction off: live lanes are not tracked
    assert set(st) <= {PASS[schedule], "vn_update", "syndrome", "status", "load", "fetch"}


@pytest.mark.parametrize("schedule", ["flooding", "hlayered"])
def test_pass_counts_without_syndrome(q, torch, code, frames, schedule):
    dec, st, _, _ = run(q, torch, code, schedule, frames["half"], enable_syndrome=False)
    assert dec.last_run_iterations == ITE
    assert launches(st, PASS[schedule]) == ITE
    assert launches(st, "vn_update") == (ITE + 1 if schedule == "flooding" else 0)
    assert launches(st, "syndrome") == 1 and launches(st, "status") == 1


@pytest.mark.parametrize("schedule", ["flooding", "hlayered"])
def test_pass_counts_early_stop_through_the_poll(q, torch, code, frames, schedule):
    dec, st, it, ok = run(q, torch, code, schedule, frames["clean"])
    assert (ok == 1).all() and (it == 1).all()
    assert dec.last_run_iterations == 2                           # the first poll, after iteration 2, finds no group running
    assert launches(st, PASS[schedule]) == 2
    if schedule == "flooding":
        assert launches(st, "vn_update") == 4
        assert launches(st, "syndrome") == 3 and launches(st, "status") == 3
    else:
        assert launches(st, "syndrome") == 5 and launches(st, "status") == 3
