"""The QBER sweep of the Monte-Carlo loop on the device (qldpc_mc_sweep): every point row and histogram of MonteCarlo.sweep against numpy over
mc_frames_host -> CPU oracle -> the schedule of tests/mc_sweep_ref.py, and against MonteCarlo.run of the point alone.  Exact equality
everywhere."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mc_ref
import mc_sweep_ref
from mc_oracle import COUNTERS as ROW, KINDS, N_ITE, ROOT, SEED, SIM, frames_reference, row_of, same_rows, setups, sim_rows  # noqa: F401 (setups is a fixture)

pytestmark = pytest.mark.gpu
FAR = 2 ** 32 - 100
# four points per code from the ladders scanned in the docstring of test_mc_gpu.test_run_equals_the_oracle_counter_for_counter
POINTS = {"peg": (0.22, 0.26, 0.30, 0.36), "ira": (0.020, 0.030, 0.040, 0.045)}
# chosen by the scan recorded in the docstring of test_rows_equal_the_oracle_and_the_schedule
MAX_FE = {"flood": 75, "hlay": 55, "i8": 75}
MAX_FRAMES = 250
N_PUNCT = {"peg": (0, 20, 40, 60), "ira": (0, 30, 60, 100)}


def sweep_reference(s, kind, qbers, C_, S, max_frames, max_fe):
    """the schedule of mc_sweep_ref over the oracle's failures of frames [0, max_frames) of every point, and the rows it leads to"""
    per = [frames_reference(s, kind, ("bsc", qb), 0, max_frames) for qb in qbers]
    sch = mc_sweep_ref.schedule(np.array([f["be"] > 0 for f in per]), C_, S, max_frames, max_fe)
    rows = [row_of(s, f, int(n)) for f, n in zip(per, sch["frames"])]
    return sch, rows


def same_points(res, hist, sch, rows, qbers, n_punct=None):
    def points(pts):
        assert pts.shape == (len(qbers),) and (pts["qber"] == np.array(qbers)).all()
        assert (pts["n_punct"] == (np.zeros(len(qbers)) if n_punct is None else np.array(n_punct))).all()
    same_rows(res, "points", hist, sch, rows, points)


def run_row(mc, qber, first, n):
    r = mc.run(qber, first, n)
    return {k: int(r[k]) for k in ROW}, mc.iter_hist(), mc.failed_frames()


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("name", ["peg", "ira"])
def test_rows_equal_the_oracle_and_the_schedule(q, setups, name, kind):
    """Four points, batch 192, chunk 16 (12 slots), max_frames 250 = 15 chunks + 10 frames, no puncturing: every row, histogram, last round and
    closing reason against the oracle's frames [0, 250) of each point fed through mc_sweep_ref.schedule.  max_frame_errors per decoder kind was
    chosen by a scan with the oracle on the CPU (frames [0, 250) of SEED, NMS 0.75, 20 iterations, all-zero codeword); frame errors of each
    point after 48 / 96 / 144 / 192 / 250 frames:
      PEGReg504x1008   flood  3 30 48 48 | 4 56 96 96 | 6  85 142 144 |  9 115 187 192 | 11 151 243 250
                       hlay   0 15 44 48 | 0 32 90 96 | 0  43 132 144 |  0  62 172 192 |  0  81 228 250
                       i8     3 35 48 48 | 7 64 96 96 | 9  95 143 144 | 14 126 188 192 | 16 164 245 250
      IRA(2000, 1590)  flood  1 24 48 48 | 2 57 96 96 | 2  90 144 144 |  2 120 191 192 |  2 158 248 250
                       hlay   0 13 45 48 | 0 31 92 96 | 0  49 139 144 |  0  66 185 192 |  0  87 240 250
                       i8     1 23 48 48 | 2 55 96 96 | 2  88 144 144 |  2 117 191 192 |  2 153 248 250
    -> 75 (flood, i8) and 55 (hlay) give the same schedule everywhere: rounds of 3 3 3 3 | 3 3 3 3 | 6 6 0 0 | 4 0 0 0 chunks, points 2 and 3
    closed by max_fe after round 1 (96 frames), point 1 by max_fe after round 2 (192 frames), point 0 by max_frames in round 3 through the
    ragged chunk [240, 250); every threshold lies 7 or more failures away from the counts it separates.  The frames of the test carry the
    source's codewords instead of the all-zero one, so single counts may differ; the conditions are asserted on the test's own reference.

    The fourth condition, a round whose slots do not divide evenly among the open points: four points that start together hold equal `done`
    while they are open, and 12 slots split into equal shares among 4, 3, 2 or 1 of them, so no round of THIS configuration can give two open
    points different numbers of chunks.  What it does reach is the round in which the 12 slots exceed what the open points need (round 3: 4 of
    12 slots dealt); that is asserted here.  Shares that differ among open points are test_rows_with_unequal_shares (10 slots) and
    test_point_counts (7 points on 4 slots)."""
    s = setups(name)
    qbers, max_fe = POINTS[name], MAX_FE[kind]
    sch, rows = sweep_reference(s, kind, qbers, 16, 12, MAX_FRAMES, max_fe)
    print(name, kind, sch)
    assert len(set(sch["last_round"].tolist())) >= 3                                       # three different closing rounds
    assert (sch["closed_by"] == mc_sweep_ref.CLOSED_MAX_FE).any()
    ragged = (sch["closed_by"] == mc_sweep_ref.CLOSED_MAX_FRAMES) & (sch["frames"] == MAX_FRAMES)
    assert ragged.any() and MAX_FRAMES % 16 != 0                                           # closed by max_frames through a ragged last chunk
    assert any(int(g.sum()) != 12 or len(set(g[g > 0].tolist())) > 1 for g in sch["gives"])  # a round that is not 12 slots in equal shares
    mc = q.MonteCarlo(s.decoder(kind), s.enc, seed=SEED, batch=192)
    res = mc.sweep(qbers, max_frames=MAX_FRAMES, max_frame_errors=max_fe, chunk=16)
    same_points(res, mc.sweep_hist(), sch, rows, qbers)
    before = mc.device_bytes
    res = mc.sweep(qbers, max_frames=MAX_FRAMES, max_frame_errors=max_fe, chunk=16)          # again: the same, and nothing allocated
    same_points(res, mc.sweep_hist(), sch, rows, qbers)
    assert mc.device_bytes == before


@pytest.mark.parametrize("name,kind", [("peg", "flood"), ("ira", "hlay")])
def test_rows_with_unequal_shares(q, setups, name, kind):
    """the same points and frames on batch 160 = 10 slots: 3 3 2 2 chunks while four points are open, so the open points hold different `done`,
    the batch holds chunks of different frame ranges side by side, and the stop rule meets the points at different frame counts"""
    s = setups(name)
    qbers, max_fe = POINTS[name], MAX_FE[kind]
    sch, rows = sweep_reference(s, kind, qbers, 16, 10, MAX_FRAMES, max_fe)
    assert any(len(set(g[g > 0].tolist())) > 1 for g in sch["gives"]) and len(set(sch["frames"].tolist())) >= 3
    mc = q.MonteCarlo(s.decoder(kind), s.enc, seed=SEED, batch=160)
    res = mc.sweep(qbers, max_frames=MAX_FRAMES, max_frame_errors=max_fe, chunk=16)
    same_points(res, mc.sweep_hist(), sch, rows, qbers)


@pytest.mark.parametrize("name,kind", [("peg", "flood"), ("ira", "i8"), ("peg", "hlay")])
def test_a_row_is_the_points_own_run(q, setups, name, kind):
    """nested puncturing over a seeded permutation of the parity VNs on top of a fixed set, batch 96, chunk 8: every row and histogram equals
    set_puncture(fixed + prefix_q) + run(qber_q, first_frame, frames_q) on the same object; point 1 also against the oracle with those VNs
    at LLR 0; the run of a point is the same before and after the sweep, and the sweep leaves the last run's results alone"""
    s = setups(name)
    qbers, n_punct, first = POINTS[name], N_PUNCT[name], 1000
    perm = np.random.default_rng(7).permutation(np.nonzero(s.cls == 1)[0]).astype(np.int32)
    order, fixed = perm[:n_punct[-1]], np.sort(perm[-5:])
    mc = q.MonteCarlo(s.decoder(kind, 96), s.enc, seed=SEED, batch=96)

    def own(i, n):
        mc.set_puncture(np.sort(np.concatenate([fixed, order[:n_punct[i]]])))
        return run_row(mc, qbers[i], first, n)

    before = own(1, 100)
    mc.set_puncture(fixed)
    last_run = run_row(mc, qbers[0], first, 50)
    res = mc.sweep(qbers, n_punct, order, first_frame=first, max_frames=100, max_frame_errors=30, chunk=8)
    hist = mc.sweep_hist()
    assert (mc.iter_hist() == last_run[1]).all() and (mc.failed_frames() == last_run[2]).all()      # of the last run, untouched
    pts = res["points"]
    print(name, kind, pts)
    assert len(set(pts["frames"].tolist())) >= 2 and (pts["frames"] % 8 != 0).any()
    rows = []
    for i in range(4):
        row, h, _ = own(i, int(pts["frames"][i]))
        rows.append((row, h))
    same_points(res, hist, None, rows, qbers, n_punct)
    after = own(1, 100)
    assert before[0] == after[0] and (before[1] == after[1]).all() and (before[2] == after[2]).all()
    erased = np.sort(np.concatenate([fixed, order[:n_punct[1]]]))
    row, h = row_of(s, frames_reference(s, kind, ("bsc", qbers[1]), first, 100, erased), int(pts["frames"][1]))
    assert {k: int(pts[k][1]) for k in ROW} == row and (hist[1] == h).all()


def test_frame_index_carry(q, setups):
    s = setups("ira")
    qbers = POINTS["ira"][:3]
    mc = q.MonteCarlo(s.decoder("flood"), s.enc, seed=SEED, batch=192)
    res = mc.sweep(qbers, first_frame=FAR, max_frames=170, max_frame_errors=0, chunk=16)      # frames 2^32 - 100 .. 2^32 + 69
    hist = mc.sweep_hist()
    rows = [run_row(mc, qb, FAR, 170)[:2] for qb in qbers]
    same_points(res, hist, None, rows, qbers)
    for i, qb in enumerate(qbers):
        assert res["points"]["channel_flips"][i] == mc_ref.popcount(q.mc_frames_host(s.K, s.N, SEED, qb, FAR, 170, info_bits_pos=s.pos)[1])
    row, h = row_of(s, frames_reference(s, "flood", ("bsc", qbers[1]), FAR, 170), 170)
    assert {k: int(res["points"][k][1]) for k in ROW} == row and (hist[1] == h).all()


def test_point_counts(q, setups):
    s = setups("peg")
    mc = q.MonteCarlo(s.decoder("flood", 96), s.enc, seed=SEED, batch=32)
    # P = 1 equals run
    res = mc.sweep([0.26], max_frames=70, chunk=8)
    same_points(res, mc.sweep_hist(), None, [run_row(mc, 0.26, 0, 70)[:2]], [0.26])
    assert res["rounds"] == 3 and res["points"]["closed_by"][0] == q.MC_CLOSED_MAX_FRAMES
    # P = 7 on 4 slots: the failure table of every point from its own run over [0, 44), the schedule from mc_sweep_ref
    qbers = (0.20, 0.24, 0.26, 0.28, 0.30, 0.33, 0.36)
    fail = np.zeros((7, 44), bool)
    for i, qb in enumerate(qbers):
        mc.run(qb, 0, 44)
        fail[i, mc.failed_frames().astype(np.int64)] = True
    sch = mc_sweep_ref.schedule(fail, 8, 4, 44, 12)
    print(sch)
    assert (sch["gives"][0] == [1, 1, 1, 1, 0, 0, 0]).all()                                # the lowest open points first
    assert any(len(set(g[g > 0].tolist())) > 1 for g in sch["gives"]) and all(g[4:].any() for g in sch["gives"][2:])      # unequal shares; slots pass on
    assert set(sch["closed_by"].tolist()) == {1, 2}
    res = mc.sweep(qbers, max_frames=44, max_frame_errors=12, chunk=8)
    hist = mc.sweep_hist()
    rows = [run_row(mc, qb, 0, int(n))[:2] for qb, n in zip(qbers, sch["frames"])]
    same_points(res, hist, sch, rows, qbers)
    assert ((res["points"]["frames"] == 44) | (res["points"]["frame_errors"] >= 12)).all()      # every point closed
    # chunk = batch: one slot, the points one after the other
    res = mc.sweep(qbers[2:5], max_frames=40, max_frame_errors=0, chunk=32)
    same_points(res, mc.sweep_hist(), None, [run_row(mc, qb, 0, 40)[:2] for qb in qbers[2:5]], qbers[2:5])
    assert res["rounds"] == 6 and res["points"]["last_round"].tolist() == [1, 3, 5]


def test_no_stop_rule(q, setups):
    s = setups("ira")
    qbers = POINTS["ira"]
    mc = q.MonteCarlo(s.decoder("hlay", 96), s.enc, seed=SEED, batch=96)
    res = mc.sweep(qbers, max_frames=100, max_frame_errors=0)                                # chunk 0 = min(64, batch): one slot
    pts, hist = res["points"], mc.sweep_hist()
    assert (pts["frames"] == 100).all() and (pts["closed_by"] == q.MC_CLOSED_MAX_FRAMES).all() and res["frames"] == 400
    assert (np.diff(pts["channel_flips"].astype(np.int64)) >= 0).all() and pts["channel_flips"][0] < pts["channel_flips"][-1]      # nested flip sets
    assert hist.shape == (4, N_ITE + 1) and (hist.sum(1) == 100).all()
    assert (pts["channel_bits"] == 100 * s.K).all()
    for i, qb in enumerate(qbers):
        assert pts["channel_flips"][i] == mc_ref.popcount(q.mc_frames_host(s.K, s.N, SEED, qb, 0, 100, info_bits_pos=s.pos)[1])


def test_refusals_leave_the_last_rows_readable(q, setups):
    s = setups("peg")
    qbers, max_fe = POINTS["peg"], MAX_FE["flood"]
    sch, rows = sweep_reference(s, "flood", qbers, 16, 12, MAX_FRAMES, max_fe)
    mc = q.MonteCarlo(s.decoder("flood"), s.enc, seed=SEED, batch=192)
    good = dict(max_frames=MAX_FRAMES, max_frame_errors=max_fe, chunk=16)
    assert mc.sweep_stats().size == 0
    res = mc.sweep(qbers, **good)
    hist = mc.sweep_hist()
    same_points(res, hist, sch, rows, qbers)
    order = np.nonzero(s.cls == 1)[0][:10].astype(np.int32)

    def refused(status, *args, **kw):
        with pytest.raises(q.QldpcError) as e:
            mc.sweep(*args, **kw)
        assert e.value.status == status, (args, kw, e.value)
        assert (mc.sweep_stats() == res["points"]).all() and (mc.sweep_hist() == hist).all()

    mc.set_awgn(sigma=0.8)
    refused(-8, qbers, **good)                                                             # a table in force
    mc.set_channel()
    refused(-6, (0.22, 0.5), **good)
    refused(-6, (0.22, 0.0), **good)
    refused(-6, qbers, (0, 1, 2, 11), order, **good)                                       # n_punct > n_order
    refused(-6, qbers, (0, 1, 2, 3), None, **good)                                         # n_order = 0: every n_punct must be 0
    refused(-6, qbers, (0, -1, 2, 3), order, **good)
    refused(-1, qbers, (0, 1, 2, 3), np.concatenate([order, order[:1]]), **good)           # a repeated VN
    refused(-1, qbers, (0, 1, 2, 3), np.concatenate([order, [s.N]]), **good)               # a VN outside [0, N)
    refused(-6, [], **good)                                                                # P = 0
    refused(-6, [0.1] * (q.MC_SWEEP_MAX_POINTS + 1), **good)
    refused(-6, qbers, max_frames=MAX_FRAMES, chunk=193)                                   # chunk > batch
    refused(-6, qbers, max_frames=MAX_FRAMES, chunk=-1)
    refused(-6, qbers, max_frames=0)
    # non-zero reserved fields and a missing array, through the C structures
    pts = (q.McPoint * 2)()
    pts[0].qber = pts[1].qber = 0.26
    for where in ("cfg", "point", "points"):
        cfg, out = q.McSweepCfg(), q.McSweepResult()
        cfg.points, cfg.n_points, cfg.max_frames = pts, 2, 10
        pts[1].reserved = int(where == "point")
        cfg.reserved[1] = int(where == "cfg")
        if where == "points":
            cfg.points = None
        assert q._L.qldpc_mc_sweep(mc._h, C.byref(cfg), C.byref(out)) == -1, where
        assert (mc.sweep_stats() == res["points"]).all() and (mc.sweep_hist() == hist).all()
    with pytest.raises(q.QldpcError) as e:
        q._chk(q._L.qldpc_mc_sweep_hist(mc._h, 4, None, 0), "sweep_hist")                  # a point the last sweep did not have
    assert e.value.status == -6
    again = mc.sweep(qbers, **good)
    same_points(again, mc.sweep_hist(), sch, rows, qbers)


def test_qldpc_sim_sweep_prints_the_same_rows(q, setups):
    alist = os.path.join(ROOT, "tests", "golden", "PEGReg504x1008.alist")
    args = ["-a", alist, "-r", "NMS", "-p", "0.75", "-i", str(N_ITE), "-b", "192", "-S", str(SEED), "-f", "250"]

    def rows(extra):
        got, text = sim_rows(args + extra)
        return [r[:6] for r in got], text

    table = ["-s", "0.22:0.30:0.04", "-E", "0"]
    one, _ = rows(["-D"] + table)
    swept, text = rows(["-D", "-W"] + table)
    assert len(one) == 3 and swept == one and all(int(r[1]) == 250 for r in one) and "# sweep: 3 points" in text      # EP FRA BE FE BER FER
    s = setups("peg")
    mc = q.MonteCarlo(s.decoder("flood"), s.enc, seed=SEED)
    res = mc.sweep((0.22, 0.26, 0.30), max_frames=250, max_frame_errors=40)
    got, _ = rows(["-D", "-W", "-s", "0.22:0.30:0.04", "-E", "40"])                        # -E is the stop rule of every row
    assert [(int(r[1]), int(r[2]), int(r[3])) for r in got] == [(int(p["frames"]), int(p["bit_errors"]), int(p["frame_errors"])) for p in res["points"]]
    assert len(set(r[1] for r in got)) > 1
    # -e under -D -W: a prefix of one order of the parity VNs per row
    punct, text = rows(["-D", "-W", "-e", "1.05", "-s", "0.02:0.04:0.01", "-E", "0"])
    assert len(punct) == text.count(": puncturing ") >= 1 and len(punct) + text.count("nothing to puncture") == 3
    for refused in (["-W"], ["-D", "-W", "-X", "1.6"], ["-D", "-W", "-A", "2.0"]):
        p = subprocess.run([SIM] + args + refused + table, capture_output=True, text=True, timeout=60)
        assert p.returncode == 2 and "-W" in p.stderr, refused
