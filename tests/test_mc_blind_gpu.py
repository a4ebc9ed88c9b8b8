"""Blind reconciliation rounds inside the Monte-Carlo loop on the device (qldpc_mc_blind): every counter row, `disclosed`, `decodes`, the
open list and the launch count against numpy over mc_frames_host -> encoder -> LLRs -> CPU oracle, the round loop restated in
tests/mc_blind_ref.py with the candidate set "channel VNs not yet known".  Exact equality everywhere."""
import numpy as np
import pytest

import mc_blind_ref
import mc_ref
from mc_blind_ref import got_rows
from mc_oracle import COUNTERS, KINDS, QBER, ROOT, SEED, bsc_llrs, counters, setups, sim_rows, stage_times, verdicts  # noqa: F401 (setups is a fixture)

pytestmark = pytest.mark.gpu
ASK, ROUNDS, FRAMES = 8, 3, 192
BLIND_STAGES = ("source", "encode", "channel", "load", "decode", "advance")      # every stage that launches a kernel in every call


def check(q, mc, res, ref, R, n, batch, sel=None):
    """a result against the reference's frames sel (None: all n): rows, sums, decodes, the open list with its known rows, the launch count"""
    close, known = ref["close"], ref["known"]
    sel = np.arange(close.size) if sel is None else np.asarray(sel)
    first = int(res["next_frame"]) - n
    rows = mc_blind_ref.rows_of(close, known, ref["f"], ref["n_chan"], R, sel)
    assert got_rows(res) == rows, (got_rows(res), rows)
    assert res["frames"] == n == sum(r["frames"] for r in rows)
    assert res["frame_errors"] == sum(r["frame_errors"] for r in rows) and res["undetected"] == sum(r["undetected"] for r in rows)
    assert res["open"] == rows[-1]["frames"] == int((close[sel] < 0).sum()) and res["disclosed"] == int(known[sel].sum())
    assert res["decodes"] == sum((r + 1) * rows[r]["frames"] for r in range(R + 1)) + (R + 1) * rows[-1]["frames"]
    launches, peak, _ = mc_blind_ref.replay(close[sel], R, batch, schedule=lambda pool, left, b: q.mc_blind_next(pool, left, b))
    assert res["launches"] == len(launches) and res["decodes"] == sum(len(x["frames"]) for x in launches)
    frames, rows_known = mc.blind_open()
    want = sel[close[sel] < 0]
    assert (frames == (first + want - sel[0]).astype(np.uint64)).all() and frames.size == want.size
    assert (rows_known == mc_ref.pack(known[want])).all()
    stage_times(res, BLIND_STAGES + (("select",) if R else ()))
    return launches


def monte_carlo(q, s, kind, batch=192):
    return q.MonteCarlo(s.decoder(kind, 192 if batch == 192 else 64), s.enc, seed=SEED, batch=batch)


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("name", ["peg", "ira"])
def test_rows_equal_the_oracle_loop(q, setups, name, kind):
    """Frames [0, 192) of SEED at the loop's QBERs, ask_bits 8, max_rounds 3: every row 0 .. 4 is non-empty on the reference (asserted first).
    Scan with the oracle on the CPU (NMS 0.75, 20 iterations, the source's codewords; frames closed in rounds 0 / 1 / 2 / 3, still open):
          code  qber   flood                      hlay                       i8
          peg   0.26   77 / 61 / 34 / 17, open  3  130 / 36 / 20 /  5, open  1   66 / 67 / 32 / 20, open  7
          ira   0.03   72 / 62 / 20 / 13, open 25  126 / 29 / 13 / 10, open 14   75 / 56 / 22 / 19, open 20
    key bits asked by the frames of rounds 1 / 2 / 3 / open: peg flood 488 / 544 / 408 / 72 (7.9 per frame over the 192), ira flood 496 / 320 / 312 / 600 (9.0).
    Round 0 closes what the scan of test_mc_gpu.test_run_equals_the_oracle_counter_for_counter leaves without a frame error (115 / 62 / 126 and 120 / 66 / 117
    failed frames).  With the all-zero codeword the float kinds give the same rows (the decoders are sign-symmetric) and peg i8 66 / 68 / 31 / 20, open 7.
    No undetected error occurred anywhere in the scan."""
    s = setups(name)
    ref = mc_blind_ref.reference(s, kind, QBER[name], 0, FRAMES, ASK, ROUNDS)
    print(name, kind, [r["frames"] for r in ref["rows"]], [r["disclosed"] for r in ref["rows"]])
    assert all(r["frames"] > 0 for r in ref["rows"])
    mc = monte_carlo(q, s, kind)
    bytes_before = mc.device_bytes
    res = mc.blind(QBER[name], ASK, ROUNDS, 0, FRAMES)
    check(q, mc, res, ref, ROUNDS, FRAMES, 192)
    assert res["next_frame"] == FRAMES and res["total_ms"] > 0
    grown = mc.device_bytes
    Wn = (s.N + 31) // 32
    assert grown - bytes_before >= ROUNDS * (2 * 192 - 1) * (8 + 4 * Wn)           # the pools are counted
    mc.blind(QBER[name], ASK, ROUNDS - 1, 0, 64)
    assert mc.device_bytes == grown                                                # a smaller max_rounds allocates nothing


@pytest.mark.parametrize("name,kind", [("peg", "flood"), ("ira", "hlay"), ("peg", "i8")])
def test_rows_do_not_depend_on_the_pooling(q, setups, name, kind):
    """batch 192, 64 and 40 (decoders of 192, 64 and 64 frames; 40 is ragged inside a group): the same rows, sums, decodes and open list; the launch
    count is what mc_blind_next replays from the reference's open counts.  With batch 64 a level >= 1 launch is full and holds frames of two
    different level-0 launches (from the replay).  A run split into [0, 96) and [96, 192) adds up to the one call."""
    s = setups(name)
    ref = mc_blind_ref.reference(s, kind, QBER[name], 0, FRAMES, ASK, ROUNDS)
    results = {}
    for batch in (192, 64, 40):
        mc = monte_carlo(q, s, kind, batch)
        results[batch] = mc.blind(QBER[name], ASK, ROUNDS, 0, FRAMES)
        launches = check(q, mc, results[batch], ref, ROUNDS, FRAMES, batch)
        if batch == 64:
            assert any(x["level"] >= 1 and len(x["frames"]) == 64 and len(set(x["src"])) >= 2 for x in launches), [(x["level"], len(x["frames"])) for x in launches]
        if batch == 40:
            assert any(len(x["frames"]) % 64 not in (0, 40) for x in launches)
    assert got_rows(results[192]) == got_rows(results[64]) == got_rows(results[40])
    mc = monte_carlo(q, s, kind, 64)
    a = mc.blind(QBER[name], ASK, ROUNDS, 0, 96)
    check(q, mc, a, ref, ROUNDS, 96, 64, np.arange(96))
    b = mc.blind(QBER[name], ASK, ROUNDS, 96, 96)
    check(q, mc, b, ref, ROUNDS, 96, 64, np.arange(96, 192))
    assert a["next_frame"] == 96 and b["next_frame"] == 192
    assert mc_blind_ref.add_rows(got_rows(a), got_rows(b)) == got_rows(results[192])
    for k in ("frames", "frame_errors", "undetected", "open", "disclosed", "decodes"):
        assert a[k] + b[k] == results[192][k], k


@pytest.mark.parametrize("kind", sorted(KINDS))
def test_no_rounds_is_the_run_split_by_the_syndrome(q, setups, kind):
    s = setups("peg")
    mc = monte_carlo(q, s, kind, 64)
    run = counters(mc.run(QBER["peg"], 5, 150))
    res = mc.blind(QBER["peg"], ASK, 0, 5, 150)
    rows = got_rows(res)
    assert len(rows) == 2 and rows[0]["frames"] > 0 and rows[1]["frames"] > 0
    assert {k: mc_blind_ref.add_rows(rows[:1], rows[1:])[0][k] for k in COUNTERS} == run
    assert rows[0]["not_converged"] == 0 and rows[1]["not_converged"] == rows[1]["frames"] == res["open"]
    assert res["disclosed"] == 0 == rows[0]["disclosed"] == rows[1]["disclosed"] and res["decodes"] == 150 and res["launches"] == 3
    frames, known = mc.blind_open()
    assert frames.size == res["open"] and not known.any() and (np.diff(frames.astype(np.int64)) > 0).all()
    assert counters(mc.run(QBER["peg"], 5, 150)) == run


def test_row_loops_in_several_trips(q, O):
    """N = 8300: 260 words per row, so the row loops of a wave (the popcount of the known row, the append's copy) take four full trips and a fifth with
    four live lanes.  Two NMS iterations leave every frame open, 16 frames across the carry of the frame index, ask_bits 40, max_rounds 2, with
    batch 16 and batch 5: the open list holds all 16 frames and their known rows are the oracle loop's word for word, and so is row 3.
    Asserted on the reference alone: asked positions beyond word 64, and in word 206, the last that holds channel VNs (8 of them: VNs 6592 .. 6599).
    QBER 0.02 by a scan with the oracle on the CPU over these 16 frames (all-zero codeword; asked positions past word 64 / in word 206):
        qber   0.020  0.025  0.030  0.035  0.040  0.050
        asked   1007 / 1   706 / 1   473 / 0   4 / 0   495 / 1   0 / 0
    every frame stays open at every one of them."""
    code = q.Code.ira(8300, 6600)
    enc = q.Encoder(code, "IRA")
    K, N, pos, first, qber, R, d = enc.K, code.N, enc.info_bits_pos, 2 ** 32 - 10, 0.02, 2, 40
    assert (K, N, (N + 31) // 32) == (6600, 8300, 260) and (pos == np.arange(K)).all()
    cls = mc_ref.classes(K, N, pos)
    var, chk = code.edges()
    og = O.Graph.from_edges(N, code.M, var, chk)
    info_w, flip_w = q.mc_frames_host(K, N, SEED, qber, first, 16, info_bits_pos=pos)
    cw = enc.encode(mc_ref.unpack(info_w, K))
    flips = mc_ref.unpack(flip_w, N)
    close, known, last = mc_blind_ref.loop(lambda rows: O.decode(og, rows, "NMS", 0.75, 2, n_threads=8), bsc_llrs(q, cw ^ flips, cls, qber), cw, cls == 0, d, R)
    assert (close < 0).all() and (known.sum(1) == R * d).all() and not known[:, K:].any()
    assert known[:, 65 * 32:].any() and known[:, 206 * 32:K].any()
    ref = dict(close=close, known=known, f=verdicts(last, cw, pos, flips, cls == 0), n_chan=K)
    dec = q.Decoder(code, K, 2, info_bits_pos=pos, rule="NMS", rule_param=0.75, n_frames=16, schedule="flooding")
    for batch in (16, 5):
        mc = q.MonteCarlo(dec, enc, seed=SEED, batch=batch)
        res = mc.blind(qber, d, R, first, 16)
        check(q, mc, res, ref, R, 16, batch)
        assert res["open"] == 16 and res["disclosed"] == 16 * R * d and res["next_frame"] == first + 16
        frames, _ = mc.blind_open()
        assert frames[0] == first and frames[-1] == 2 ** 32 + 5


def test_max_frame_errors_ends_the_input_and_flushes(q, setups):
    """max_rounds 1, batch 40, limit 2: the input ends at the launch boundary at which the frame errors tallied so far (over the frames that ended:
    closed, or open after the last round) reach the limit, by the replay of the reference: after the first level-1 launch, 80 frames drawn
    (two level-0 launches fill pool 1, its launch ends frames open).  The 10 frames left in pool 1 are flushed."""
    s = setups("peg")
    R = 1
    ref = mc_blind_ref.reference(s, "flood", QBER["peg"], 0, FRAMES, ASK, R)
    close, be = ref["close"], ref["f"]["be"]
    limit, tallied = 2, [0]

    def stop(launch):
        ended = [i for i in launch["frames"] if close[i] == launch["level"] or (launch["level"] == R and close[i] < 0)]
        tallied[0] += int((be[ended] > 0).sum())
        return tallied[0] >= limit

    launches, _, drawn = mc_blind_ref.replay(close, R, 40, schedule=lambda pool, left, b: q.mc_blind_next(pool, left, b), stop=stop)
    print(drawn, [(x["level"], len(x["frames"])) for x in launches])
    assert 40 <= drawn < FRAMES and drawn % 40 == 0 and launches[-1]["level"] == 1 and len(launches[-1]["frames"]) < 40
    mc = monte_carlo(q, s, "flood", 40)
    res = mc.blind(QBER["peg"], ASK, R, 0, FRAMES, max_frame_errors=limit)
    assert res["frames"] == drawn and res["next_frame"] == drawn and res["launches"] == len(launches) and res["frame_errors"] >= limit
    assert got_rows(res) == mc_blind_ref.rows_of(close, ref["known"], ref["f"], ref["n_chan"], R, np.arange(drawn))
    assert sum(r["frames"] for r in got_rows(res)) == drawn                        # no frame in flight was dropped


def test_fixed_puncture_set(q, setups):
    s = setups("peg")
    erased = np.flatnonzero(s.cls == 1)[::9][:8]
    ref = mc_blind_ref.reference(s, "flood", QBER["peg"], 0, 96, ASK, ROUNDS, erased)
    plain = mc_blind_ref.reference(s, "flood", QBER["peg"], 0, FRAMES, ASK, ROUNDS)
    assert (ref["close"] != plain["close"][:96]).any()                             # the erased VNs change what the frames do
    mc = monte_carlo(q, s, "flood", 64)
    mc.set_puncture(erased)
    res = mc.blind(QBER["peg"], ASK, ROUNDS, 0, 96)
    check(q, mc, res, ref, ROUNDS, 96, 64)
    mc.set_puncture([])
    check(q, mc, mc.blind(QBER["peg"], ASK, ROUNDS, 0, 96), plain, ROUNDS, 96, 64, np.arange(96))


def test_refusals_queue_nothing(q, setups):
    s = setups("peg")
    ref = mc_blind_ref.reference(s, "flood", QBER["peg"], 0, FRAMES, ASK, ROUNDS)
    mc = monte_carlo(q, s, "flood")
    first = mc.blind(QBER["peg"], ASK, ROUNDS, 0, FRAMES)
    rows = got_rows(first)

    def refused(m, status, word, **kw):
        args = dict(qber=QBER["peg"], ask_bits=ASK, max_rounds=ROUNDS, first_frame=0, max_frames=FRAMES)
        args.update(kw)
        with pytest.raises(q.QldpcError) as e:
            m.blind(**args)
        assert e.value.status == status and word in str(e.value), str(e.value)

    for kw in (dict(qber=0.0), dict(qber=0.5), dict(ask_bits=0), dict(max_rounds=-1), dict(max_rounds=65)):
        refused(mc, -6, "mc_blind", **kw)
    mc.set_awgn(sigma=0.8)
    held = mc.device_bytes
    refused(mc, -7, "qldpc_mc_set_channel(mc, NULL)")
    assert got_rows(dict(rounds=mc.blind_stats())) == rows                         # the last call's rows stay readable
    mc.set_channel()
    edges = q.MonteCarlo(q.Decoder(s.code, s.K, 20, info_bits_pos=s.pos, rule="NMS", rule_param=0.75, n_frames=4, engine="edges"), s.enc, seed=SEED)
    refused(edges, -7, "engine = FRAMES", max_frames=4)
    wide = q.MonteCarlo(q.Decoder(s.code, s.K, 20, info_bits_pos=s.pos, rule="NMS", rule_param=0.75, n_frames=256, schedule="flooding"), s.enc, seed=SEED)
    before = wide.device_bytes
    refused(wide, -7, "compact = 2")
    assert wide.device_bytes == before and mc.device_bytes == held                 # refused before anything was reserved or queued
    res = mc.blind(QBER["peg"], ASK, ROUNDS, 0, FRAMES)
    check(q, mc, res, ref, ROUNDS, FRAMES, 192)
    assert got_rows(res) == rows
    off = q.MonteCarlo(q.Decoder(s.code, s.K, 20, info_bits_pos=s.pos, rule="NMS", rule_param=0.75, n_frames=256, schedule="flooding", compact="off"), s.enc, seed=SEED)
    assert got_rows(off.blind(QBER["peg"], ASK, ROUNDS, 0, FRAMES)) == rows        # the remedy the message names


def test_qldpc_sim_prints_the_rows(q, setups):
    import os
    s = setups("peg")
    mc = monte_carlo(q, s, "flood", 64)
    res = mc.blind(QBER["peg"], ASK, ROUNDS, 0, FRAMES)
    rows, text = sim_rows(["-a", os.path.join(ROOT, "tests", "golden", "PEGReg504x1008.alist"), "-r", "NMS", "-p", "0.75", "-i", "20", "-f", str(FRAMES), "-b", "64",
                           "-s", "%g:%g:1" % (QBER["peg"], QBER["peg"]), "-S", str(SEED), "-D", "-B", "%d:%d" % (ASK, ROUNDS)])
    assert len(rows) == ROUNDS + 2, text
    for r, (row, want) in enumerate(zip(rows, got_rows(res))):
        assert row[0] == ("open" if r == ROUNDS + 1 else str(r)), row
        assert [int(x) for x in row[1:4]] == [want["frames"], want["bit_errors"], want["frame_errors"]] and int(row[7]) == want["disclosed"], (row, want)
    f = q.mc_blind_efficiency(s.K, s.N - s.K, res["frames"], res["disclosed"], QBER["peg"])
    assert "# blind: %d frames, %d open, %d key bits disclosed, %d decodes in %d launches" % (res["frames"], res["open"], res["disclosed"], res["decodes"], res["launches"]) in text
    assert "f = %.4f" % f in text
