"""Guessing rounds inside the Monte-Carlo loop on the device (qldpc_mc_guess): the three counter rows, the sums, `trials`, `n_ok_sum`,
`ambiguous`, the open list with its guess rows and the launch count against numpy over mc_frames_host -> encoder -> LLRs -> CPU oracle, the loop
restated in tests/mc_guess_ref.py.  Exact equality everywhere."""
import os

import numpy as np
import pytest

import mc_guess_ref
import mc_ref
from mc_guess_ref import got_rows
from mc_oracle import COUNTERS, KINDS, QBER, ROOT, SEED, counters, setups, sim_rows, stage_times  # noqa: F401 (setups is a fixture)

pytestmark = pytest.mark.gpu
G, FRAMES = 3, 192
FRESH_STAGES = ("source", "encode", "channel", "load", "decode", "advance")      # every stage that launches a kernel in every call
SUMS = ("rescued", "open", "trials", "trial_iter_sum", "n_ok_sum", "ambiguous")


def check(q, mc, res, ref, g, n, batch, sel=None):
    """a result against the reference's frames sel (None: all n): rows, sums, decodes, the open list with its guess rows, the launch count"""
    w = ref["winner"]
    sel = np.arange(w.size) if sel is None else np.asarray(sel)
    first = int(res["next_frame"]) - n
    rows = mc_guess_ref.rows_of(ref, sel)
    assert got_rows(res) == rows, (got_rows(res), rows)
    assert res["frames"] == n == sum(r["frames"] for r in rows)
    assert res["frame_errors"] == sum(r["frame_errors"] for r in rows) and res["undetected"] == sum(r["undetected"] for r in rows)
    sums = mc_guess_ref.sums_of(ref, g, sel)
    assert {k: int(res[k]) for k in SUMS} == sums, (res, sums)
    assert res["decodes"] == n + sums["trials"]
    launches, peak, _ = mc_guess_ref.replay(w[sel] != -2, g, batch, schedule=q.mc_guess_next)
    assert res["launches"] == len(launches) and peak < (batch >> g) + batch
    assert res["trials"] == sum(len(x["frames"]) << g for x in launches if x["kind"] == mc_guess_ref.TRIALS)
    frames, weak = mc.guess_open()
    want = sel[w[sel] == -1]
    assert frames.size == want.size and (frames == (first + want - sel[0]).astype(np.uint64)).all()
    assert (weak == mc_ref.pack(ref["weak"][want])).all()
    stage_times(res, FRESH_STAGES + (("select", "expand", "pick") if g and sums["trials"] else ()))
    return launches


def monte_carlo(q, s, kind, batch=192):
    return q.MonteCarlo(s.decoder(kind, 192 if batch == 192 else 64), s.enc, seed=SEED, batch=batch)


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("name", ["peg", "ira"])
def test_rows_equal_the_oracle_loop(q, setups, name, kind):
    """Frames [0, 192) of SEED at the loop's QBERs, guess_bits 3: rows 0, 1 and 2 are all non-empty on the reference (asserted first).
    Scan with the oracle on the CPU (NMS 0.75, 20 iterations, the all-zero codeword in place of the source's: the float decoders are sign-symmetric;
    frames closed at once / rescued / open, then the trials that ended with a zero syndrome):
          code  qber   flood                hlay                 i8
          peg   0.26   77 / 32 / 83, 32     130 / 16 / 46, 23    66 / 33 / 93, 33   (i8 with the source's codewords: 66 / 32 / 94, 32)
          ira   0.03   72 / 30 / 90, 30     126 / 16 / 50, 17    75 / 25 / 92, 29
    No rescue was wrong and none was ambiguous anywhere in the scan, so those counters are compared at zero here; tests/test_guess_gpu.py holds the
    flag against synthetic rows."""
    s = setups(name)
    ref = mc_guess_ref.reference(s, kind, QBER[name], 0, FRAMES, G)
    print(name, kind, [r["frames"] for r in ref["rows"]], mc_guess_ref.sums_of(ref, G))
    assert all(r["frames"] > 0 for r in ref["rows"])
    mc = monte_carlo(q, s, kind)
    bytes_before = mc.device_bytes
    res = mc.guess(QBER[name], G, 0, FRAMES)
    check(q, mc, res, ref, G, FRAMES, 192)
    assert res["next_frame"] == FRAMES and res["total_ms"] > 0
    grown = mc.device_bytes
    Wn = (s.N + 31) // 32
    assert grown - bytes_before >= (192 + 96) * (8 + 8 * Wn) + 2 * 192 * 4 * Wn      # the pool and the trial rows are counted
    mc.guess(QBER[name], G - 1, 0, 64)
    mc.guess(QBER[name], G + 2, 0, 64)
    assert mc.device_bytes == grown                                                # no later call allocates


@pytest.mark.parametrize("name,kind", [("peg", "flood"), ("ira", "hlay"), ("peg", "i8")])
def test_rows_do_not_depend_on_the_pooling(q, setups, name, kind):
    """batch 192, 64 and 40 (decoders of 192, 64 and 64 frames): S = 24, 8 and 5 sources per trial launch, the last ragged inside a group of 64
    frames; the same rows, sums and open list, and the launch count is what mc_guess_next replays from the reference's failed first decodes.  With
    batch 64 a trial launch holds frames of two different fresh launches (from the replay).  A run split into [0, 96) and [96, 192) adds up to
    the one call."""
    s = setups(name)
    ref = mc_guess_ref.reference(s, kind, QBER[name], 0, FRAMES, G)
    results = {}
    for batch in (192, 64, 40):
        mc = monte_carlo(q, s, kind, batch)
        results[batch] = mc.guess(QBER[name], G, 0, FRAMES)
        launches = check(q, mc, results[batch], ref, G, FRAMES, batch)
        trials = [x for x in launches if x["kind"] == mc_guess_ref.TRIALS]
        assert any(len(x["frames"]) == batch >> G for x in trials)
        if batch == 64:
            assert any(len(set(x["src"])) >= 2 for x in trials), [len(x["frames"]) for x in launches]
    assert got_rows(results[192]) == got_rows(results[64]) == got_rows(results[40])
    mc = monte_carlo(q, s, kind, 64)
    a = mc.guess(QBER[name], G, 0, 96)
    check(q, mc, a, ref, G, 96, 64, np.arange(96))
    b = mc.guess(QBER[name], G, 96, 96)
    check(q, mc, b, ref, G, 96, 64, np.arange(96, 192))
    assert a["next_frame"] == 96 and b["next_frame"] == 192
    assert mc_guess_ref.add_rows(got_rows(a), got_rows(b)) == got_rows(results[192])
    for k in ("frames", "frame_errors", "undetected", "decodes") + SUMS:
        assert a[k] + b[k] == results[192][k], k


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_no_guess_bits_is_the_run_split_by_the_syndrome(q, setups, kind):
    s = setups("peg")
    mc = monte_carlo(q, s, kind, 64)
    run = counters(mc.run(QBER["peg"], 5, 150))
    res = mc.guess(QBER["peg"], 0, 5, 150)
    rows = got_rows(res)
    assert len(rows) == 3 and rows[0]["frames"] > 0 and rows[1]["frames"] == 0 and rows[2]["frames"] > 0
    assert not any(rows[1].values())
    assert {k: mc_guess_ref.add_rows(rows[:1], rows[2:])[0][k] for k in COUNTERS} == run
    assert rows[0]["not_converged"] == 0 and rows[2]["not_converged"] == rows[2]["frames"] == res["open"]
    assert res["trials"] == res["rescued"] == res["n_ok_sum"] == res["trial_iter_sum"] == 0 and res["decodes"] == 150 and res["launches"] == 3
    assert res["expand_ms"] == 0 and res["pick_ms"] == 0
    frames, weak = mc.guess_open()
    assert frames.size == res["open"] and not weak.any() and (np.diff(frames.astype(np.int64)) > 0).all()
    assert counters(mc.run(QBER["peg"], 5, 150)) == run                           # the loop's own counters were not touched


def test_max_frame_errors_ends_the_input_and_flushes(q, setups):
    """batch 40 (S = 5), limit 3: the input ends at the launch boundary at which the errors tallied so far -- frames closed or rescued wrong, frames
    that ended open; failed first decodes still pooled do not count -- reach the limit, by the replay of the reference.  What is pooled then is flushed."""
    s = setups("peg")
    ref = mc_guess_ref.reference(s, "flood", QBER["peg"], 0, FRAMES, G)
    w, be = ref["winner"], ref["f"]["be"]
    limit, tallied = 3, [0]

    def stop(launch):
        idx = np.array(launch["frames"])
        if launch["kind"] == mc_guess_ref.FRESH:
            tallied[0] += int(((w[idx] == -2) & (be[idx] > 0)).sum())
        else:
            tallied[0] += int(((w[idx] == -1) | (be[idx] > 0)).sum())
        return tallied[0] >= limit

    launches, _, drawn = mc_guess_ref.replay(w != -2, G, 40, schedule=q.mc_guess_next, stop=stop)
    print(drawn, [(x["kind"], len(x["frames"])) for x in launches])
    assert 40 <= drawn < FRAMES and drawn % 40 == 0 and launches[-1]["kind"] == mc_guess_ref.TRIALS
    mc = monte_carlo(q, s, "flood", 40)
    res = mc.guess(QBER["peg"], G, 0, FRAMES, max_frame_errors=limit)
    assert res["frames"] == drawn and res["next_frame"] == drawn and res["launches"] == len(launches)
    rows = mc_guess_ref.rows_of(ref, np.arange(drawn))
    assert got_rows(res) == rows and mc_guess_ref.errors_of(rows) >= limit
    assert sum(r["frames"] for r in got_rows(res)) == drawn                        # no pooled frame was dropped


def test_fixed_puncture_set(q, setups):
    s = setups("peg")
    erased = np.flatnonzero(s.cls == 1)[::9][:8]
    ref = mc_guess_ref.reference(s, "flood", QBER["peg"], 0, 96, G, erased)
    plain = mc_guess_ref.reference(s, "flood", QBER["peg"], 0, FRAMES, G)
    assert (ref["winner"] != plain["winner"][:96]).any()                           # the erased VNs change what the frames do
    mc = monte_carlo(q, s, "flood", 64)
    mc.set_puncture(erased)
    check(q, mc, mc.guess(QBER["peg"], G, 0, 96), ref, G, 96, 64)
    mc.set_puncture([])
    check(q, mc, mc.guess(QBER["peg"], G, 0, 96), plain, G, 96, 64, np.arange(96))


def test_refusals_queue_nothing(q, setups):
    s = setups("peg")
    ref = mc_guess_ref.reference(s, "flood", QBER["peg"], 0, FRAMES, G)
    mc = monte_carlo(q, s, "flood")
    rows = got_rows(mc.guess(QBER["peg"], G, 0, FRAMES))
    blind_rows = mc.blind(QBER["peg"], 8, 1, 0, 64)["rounds"].copy()

    def refused(m, status, word, **kw):
        args = dict(qber=QBER["peg"], guess_bits=G, first_frame=0, max_frames=FRAMES)
        args.update(kw)
        with pytest.raises(q.QldpcError) as e:
            m.guess(**args)
        assert e.value.status == status and word in str(e.value), str(e.value)

    for kw in (dict(qber=0.0), dict(qber=0.5), dict(guess_bits=-1), dict(guess_bits=11), dict(guess_bits=8)):      # 256 trials do not fit 192 frames
        refused(mc, -6, "mc_guess", **kw)
    few = np.full(s.N, 1, np.uint8)
    few[s.pos[:2]] = 0
    refused(q.MonteCarlo(s.decoder("flood"), s.enc, vn_class=few, seed=SEED), -6, "channel VNs")
    mc.set_awgn(sigma=0.8)
    held = mc.device_bytes
    refused(mc, -7, "qldpc_mc_set_channel(mc, NULL)")
    assert got_rows(dict(rows=mc.guess_stats())) == rows                           # the last call's rows stay readable
    mc.set_channel()
    edges = q.MonteCarlo(q.Decoder(s.code, s.K, 20, info_bits_pos=s.pos, rule="NMS", rule_param=0.75, n_frames=16, engine="edges"), s.enc, seed=SEED)
    refused(edges, -7, "engine = FRAMES", max_frames=16)
    wide = q.MonteCarlo(q.Decoder(s.code, s.K, 20, info_bits_pos=s.pos, rule="NMS", rule_param=0.75, n_frames=256, schedule="flooding"), s.enc, seed=SEED)
    before = wide.device_bytes
    refused(wide, -7, "compact = 2")
    gives_up = q.MonteCarlo(q.Decoder(s.code, s.K, 20, info_bits_pos=s.pos, rule="NMS", rule_param=0.75, n_frames=64, schedule="flooding", giveup=3), s.enc, seed=SEED)
    refused(gives_up, -7, "freeze_messages = 1", max_frames=64)
    assert wide.device_bytes == before and mc.device_bytes == held                 # refused before anything was reserved or queued
    res = mc.guess(QBER["peg"], G, 0, FRAMES)
    check(q, mc, res, ref, G, FRAMES, 192)
    assert got_rows(res) == rows
    assert (mc.blind_stats() == blind_rows).all()                                  # a call touches no other front end's rows
    off = q.MonteCarlo(q.Decoder(s.code, s.K, 20, info_bits_pos=s.pos, rule="NMS", rule_param=0.75, n_frames=256, schedule="flooding", compact="off"), s.enc, seed=SEED)
    assert got_rows(off.guess(QBER["peg"], G, 0, FRAMES)) == rows                  # the remedy the message names


def test_qldpc_sim_prints_the_rows(q, setups):
    s = setups("peg")
    mc = monte_carlo(q, s, "flood", 64)
    res = mc.guess(QBER["peg"], G, 0, FRAMES)
    rows, text = sim_rows(["-a", os.path.join(ROOT, "tests", "golden", "PEGReg504x1008.alist"), "-r", "NMS", "-p", "0.75", "-i", "20", "-f", str(FRAMES), "-b", "64",
                           "-s", "%g:%g:1" % (QBER["peg"], QBER["peg"]), "-S", str(SEED), "-D", "-G", str(G)])
    assert len(rows) == 3, text
    for name, row, want in zip(("closed", "rescued", "open"), rows, got_rows(res)):
        assert row[0] == name, row
        assert [int(x) for x in row[1:4]] == [want["frames"], want["bit_errors"], want["frame_errors"]] and int(row[4]) == want["undetected"], (row, want)
    assert "# guess: %d frames, %d rescued, %d open, %d ambiguous, %d trials (%d ok) in %d launches" % (
        res["frames"], res["rescued"], res["open"], res["ambiguous"], res["trials"], res["n_ok_sum"], res["launches"]) in text
