"""Monte-Carlo FER loop on the device (qldpc_mc_*): the frames against the host mirror word for word, and every counter of
MonteCarlo.run against numpy over mc_frames_host -> CPU oracle -> compare.  Exact equality everywhere."""
import os
import subprocess

import numpy as np
import pytest

import mc_ref
from mc_oracle import COUNTERS, KINDS, N_ITE, QBER, ROOT, SEED, SIM, bsc_llrs, counters, setups, sim_rows, stage_times, tally, u32, verdicts  # noqa: F401 (setups is a fixture)

pytestmark = pytest.mark.gpu
FAR = 2 ** 32 - 100
# chosen by the scan recorded in the docstring of test_run_equals_the_oracle_counter_for_counter
QBER_DEAD = {"peg": 0.40, "ira": 0.06}     # every frame fails


@pytest.mark.parametrize("name", ["peg", "ira"])
@pytest.mark.parametrize("first,n", [(0, 192), (FAR, 192), (3, 70)])
def test_device_frames_equal_the_host_mirror(q, setups, name, first, n):
    s = setups(name)
    mc = q.MonteCarlo(s.decoder("flood"), s.enc, seed=SEED)
    info, cw, rx = (u32(t) for t in mc.frames(first, n, 0.07))
    ref_info, ref_flips = q.mc_frames_host(s.K, s.N, SEED, 0.07, first, n, info_bits_pos=s.pos)
    ref_cw = mc_ref.pack(s.codewords(ref_info))
    assert info.shape == ref_info.shape and (info == ref_info).all()
    assert cw.shape == ref_cw.shape and (cw == ref_cw).all()
    assert (rx == ref_cw ^ ref_flips).all() and ref_flips.any()


@pytest.mark.parametrize("name", ["peg", "ira"])
def test_device_frames_with_punctured_vns_and_dirty_parity(q, setups, name):
    s = setups(name)
    cls = s.cls.copy()
    cls[np.nonzero(cls == 1)[0][::5]] = q.VN_PUNCTURED
    mc = q.MonteCarlo(s.decoder("flood"), s.enc, vn_class=cls, seed=SEED + 1, parity_ber=0.25)
    info, cw, rx = (u32(t) for t in mc.frames(FAR + 90, 33, 0.11))
    ref_info, ref_flips = q.mc_frames_host(s.K, s.N, SEED + 1, 0.11, FAR + 90, 33, vn_class=cls, parity_ber=0.25)
    assert (info == ref_info).all() and (rx ^ cw == ref_flips).all()
    f = mc_ref.unpack(ref_flips, s.N)
    assert f[:, cls == 1].any() and not f[:, cls == 2].any()


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("name", ["peg", "ira"])
def test_run_equals_the_oracle_counter_for_counter(q, setups, name, kind):
    """Every counter, the histogram and the failed-frame list against numpy over mc_frames_host -> oracle -> compare; the oracle must fail
    between 10 % and 90 % of the 192 frames (asserted first).  QBER per code:
    Chosen by a scan with the oracle on the CPU (frames [0, 192) of SEED, NMS 0.75, 20 iterations, all-zero codeword; failed frames of 192):
      PEGReg504x1008, IDENTITY encoder (the 504 parity VNs pinned, so the waterfall lies far above the code's BSC threshold):
          qber   0.22  0.24  0.26  0.28  0.30  0.36
          flood     9    52   115   166   187   192
          hlay      0    14    62   135   172   192
          i8       14    56   126   171   188   192
      IRA(2000, 1590), the 410 parity VNs pinned:
          qber   0.020 0.025 0.030 0.035 0.040 0.045
          flood     2    33   120   175   191   192
          hlay      0    13    66   146   185   192
          i8        2    34   117   173   191   192
    -> 0.26 (PEG) and 0.03 (IRA); the frames of the test carry the source's codewords instead of the all-zero one."""
    s = setups(name)
    ctr, hist, failed = s.reference(kind, QBER[name], 0, 192)
    print(name, kind, ctr)
    assert 0.1 * 192 <= ctr["frame_errors"] <= 0.9 * 192
    mc = q.MonteCarlo(s.decoder(kind), s.enc, seed=SEED)
    res = mc.run(QBER[name], 0, 192)
    assert counters(res) == ctr
    assert res["batches"] == 1 and res["next_frame"] == 192 and res["decode_ms"] > 0 and res["total_ms"] > 0
    stage_times(res)
    assert (mc.iter_hist() == hist).all() and int(hist.sum()) == 192
    assert (mc.failed_frames() == failed).all()


def test_monitor_rows_in_several_trips(q, O):
    """N = 8300: 260 codeword words, so the word loop of a monitor wave (64 lanes) takes four full trips and a fifth with four live lanes, and the
    last word holds 12 VNs; every other monitor test stays inside one trip.  The class map of test_mc_strata_gpu.test_final_pass_in_several_trips
    (every fifth VN pinned, parity_ber 0.05) spreads the channel VNs over the whole frame.  16 frames across the carry of the frame index, two
    NMS iterations, through all three monitor kernels: run over the 16, search as 2 patterns x 8 frames (nothing punctured, so the frames are
    those of the run), sweep as 2 points x 8 frames in chunks of 4 (both points at the same QBER: each holds frames 0 .. 7); every counter row,
    histogram and the failed-frame list against mc_frames_host -> encoder -> LLRs -> CPU oracle.
    Asserted on the reference alone, among the first 8 frames, which all three paths see: a frame with info-bit errors beyond the first trip and
    in the last word that holds info bits, and a frame with channel flips beyond the first trip and in word 259.  The IRA encoder's info bits
    are VNs 0 .. 6599, so that last word is 206 (fourth trip) and no info bit lies in the fifth; the flips reach it.  The fifth trip is therefore
    seen through channel_flips alone: mc_monitor and mc_monitor_points count them, mc_monitor_patterns does not read rx, so a pattern monitor that
    stopped after four trips would still pass here (one that stopped after one, two or three would not).
    QBER 0.03 by a scan with the oracle on the CPU over these 16 frames (two iterations leave 390 .. 483 info-bit errors in every frame; of
    frames 0 .. 7, five have errors in word 206 and two have channel flips in word 259; 0.02 and 0.04 do as well)."""
    code = q.Code.ira(8300, 6600)
    enc = q.Encoder(code, "IRA")
    K, N, pos, first, qber, n_ite = enc.K, code.N, enc.info_bits_pos, FAR + 90, 0.03, 2
    Wn, last_info = (N + 31) // 32, (K - 1) // 32
    assert (K, N, Wn) == (6600, 8300, 260) and (pos == np.arange(K)).all() and last_info == 206
    cls = np.where(np.arange(N) % 5 == 4, 1, 0).astype(np.uint8)
    var, chk = code.edges()
    info_w, flip_w = q.mc_frames_host(K, N, SEED, qber, first, 16, vn_class=cls, parity_ber=0.05)
    info = mc_ref.unpack(info_w, K)
    cw = enc.encode(info)
    assert (cw[:, pos] == info).all()
    flips = mc_ref.unpack(flip_w, N)
    r = O.decode(O.Graph.from_edges(N, code.M, var, chk), bsc_llrs(q, cw ^ flips, cls, qber), "NMS", 0.75, n_ite, n_threads=8)
    err = np.zeros((16, N), bool)
    err[:, pos] = r["hard"][:, pos] != cw[:, pos]
    f, chan = verdicts(r, cw, pos, flips, cls == 0), flips.astype(bool) & (cls == 0)
    be, ok, it = f["be"], f["ok"], f["it"]
    assert (be == err.sum(1)).all() and (f["fl"] == chan.sum(1)).all()
    print(be.tolist(), ok.tolist(), it.tolist(), chan.sum(1).tolist())
    assert (err[:8, 64 * 32:].any(1) & err[:8, last_info * 32:].any(1)).any()                # info-bit errors past the first trip and in the last info word
    assert (chan[:8, 64 * 32:259 * 32].any(1) & chan[:8, 259 * 32:].any(1)).any()          # channel flips past the first trip and in the last word

    def row(a, b, part=0):
        return tally({k: v[a:b] for k, v in f.items()}, int((cls == 0).sum()), n_ite=n_ite)[part]

    def hist(a, b):
        return row(a, b, 1)

    dec = q.Decoder(code, K, n_ite, info_bits_pos=pos, rule="NMS", rule_param=0.75, n_frames=16)
    mc = q.MonteCarlo(dec, enc, vn_class=cls, seed=SEED, parity_ber=0.05)
    res = mc.run(qber, first, 16)
    assert counters(res) == row(0, 16) and (mc.iter_hist() == hist(0, 16)).all()
    assert (mc.failed_frames() == (first + np.nonzero(be > 0)[0]).astype(np.uint64)).all()
    stage_times(res)
    res = mc.search(qber, 0, 8, max_patterns=2, stop_at_goal=False, first_frame=first)
    assert res["patterns"] == 2 and res["batches"] == 1
    stage_times(res, ("pattern", "expand", "generate", "load", "decode", "monitor"))
    for p, (a, b) in enumerate(((0, 8), (8, 16))):
        ref = dict(row(a, b), pattern=p)
        assert {k: int(res["stats"][k][p]) for k in res["stats"].dtype.names} == {k: ref[k] for k in res["stats"].dtype.names}, p
    res = mc.sweep((qber, qber), first_frame=first, max_frames=8, chunk=4)
    sweep_hist = mc.sweep_hist()
    assert res["rounds"] == 1 and res["frames"] == 16
    stage_times(res)
    for p in range(2):
        assert {k: int(res["points"][k][p]) for k in COUNTERS} == row(0, 8) and (sweep_hist[p] == hist(0, 8)).all(), p


def test_spa_is_a_tolerance_class_frames_and_flips_only(q, setups):
    s = setups("peg")
    dec = q.Decoder(s.code, s.K, N_ITE, info_bits_pos=s.pos, rule="SPA", n_frames=192)
    res = q.MonteCarlo(dec, s.enc, seed=SEED).run(QBER["peg"], 0, 192)
    flips = q.mc_frames_host(s.K, s.N, SEED, QBER["peg"], 0, 192, info_bits_pos=s.pos)[1]
    assert res["frames"] == 192 and res["channel_flips"] == mc_ref.popcount(flips) and res["channel_bits"] == 192 * s.K


@pytest.mark.parametrize("name,kind", [("ira", "flood"), ("peg", "i8"), ("ira", "hlay")])
def test_batch_and_range_invariance(q, setups, name, kind):
    s = setups(name)
    qber = QBER[name]
    dec = s.decoder(kind, 512)
    one = q.MonteCarlo(dec, s.enc, seed=SEED, batch=512)
    r1 = one.run(qber, 0, 512)
    h1, f1 = one.iter_hist(), one.failed_frames()
    assert r1["batches"] == 1 and r1["frames"] == 512 and 0 < r1["frame_errors"] < 512
    assert r1["channel_flips"] == mc_ref.popcount(q.mc_frames_host(s.K, s.N, SEED, qber, 0, 512, info_bits_pos=s.pos)[1])
    three = q.MonteCarlo(dec, s.enc, seed=SEED, batch=192)
    r3 = three.run(qber, 0, 512)                                          # 192 + 192 + 128
    assert r3["batches"] == 3 and counters(r3) == counters(r1)
    assert (three.iter_hist() == h1).all() and (three.failed_frames() == f1).all()
    ra = three.run(qber, 0, 200)                                          # 192 + 8
    ha, fa = three.iter_hist(), three.failed_frames()
    rb = one.run(qber, ra["next_frame"], 312)
    assert ra["next_frame"] == 200 and ra["batches"] == 2 and rb["next_frame"] == 512
    for k in COUNTERS:
        assert (max(ra[k], rb[k]) if k == "iter_max" else ra[k] + rb[k]) == r1[k], k
    assert (ha + one.iter_hist() == h1).all() and (np.concatenate([fa, one.failed_frames()]) == f1).all()
    # the small decoder of the oracle test sees the same first 192 frames
    ctr, _, failed = s.reference(kind, qber, 0, 192)
    assert (f1[f1 < 192] == failed).all()


def test_stop_rule(q, setups):
    s = setups("peg")
    qber = QBER_DEAD["peg"]
    ctr, _, _ = s.reference("flood", qber, 0, 192)
    assert ctr["frame_errors"] == 192                                     # the oracle fails every frame here
    mc = q.MonteCarlo(s.decoder("flood"), s.enc, seed=SEED, batch=192, fail_cap=200)
    r = mc.run(qber, 0, 1920, max_frame_errors=1)
    assert r["batches"] == 1 and r["frames"] == 192 and r["next_frame"] == 192 and counters(r) == ctr
    r = mc.run(qber, 0, 1920, max_frame_errors=193)                       # reached inside the second batch: stops at its end
    assert r["batches"] == 2 and r["frames"] == 384
    r = mc.run(qber, 0, 1920, max_frame_errors=0)
    assert r["batches"] == 10 and r["frames"] == 1920 and r["frame_errors"] == 1920
    kept = mc.failed_frames()                                             # the first fail_cap failures, in batch order
    assert kept.size == 200 and (kept[:192] == np.arange(192)).all() and (kept[192:] >= 192).all() and (kept[192:] < 384).all()


def test_qldpc_sim_device_loop_prints_the_same_row(q, setups):
    s = setups("peg")
    alist = os.path.join(ROOT, "tests", "golden", "PEGReg504x1008.alist")
    args = ["-a", alist, "-r", "NMS", "-p", "0.75", "-i", str(N_ITE), "-b", "192", "-s", "0.26:0.26:0.01", "-S", str(SEED), "-D"]

    def row(extra):
        rows, _ = sim_rows(args + extra)
        assert len(rows) == 1
        f = rows[0]
        return dict(fra=int(f[1]), be=int(f[2]), fe=int(f[3]), thr=float(f[6]))

    mc = q.MonteCarlo(s.decoder("flood"), s.enc, seed=SEED)
    res = mc.run(0.26, 0, 500)                                            # 192 + 192 + 116
    got = row(["-f", "500"])
    assert (got["fra"], got["be"], got["fe"]) == (res["frames"], res["bit_errors"], res["frame_errors"]) and got["fra"] == 500 and got["thr"] > 0
    res = mc.run(0.26, 0, 1920, max_frame_errors=1)
    got = row(["-f", "1920", "-E", "1"])
    assert (got["fra"], got["be"], got["fe"]) == (res["frames"], res["bit_errors"], res["frame_errors"]) and got["fra"] == 192
    for refused in (["-e", "1.6"], ["-e", "1.6", "-R"]):                   # a random puncture pattern per batch stays host-only
        p = subprocess.run([SIM] + args + ["-f", "192"] + refused, capture_output=True, text=True, timeout=60)
        assert p.returncode != 0 and "-D" in p.stderr


def test_errors_leave_everything_usable(q, setups):
    s = setups("peg")
    dec = s.decoder("flood")
    ctr, _, _ = s.reference("flood", QBER["peg"], 0, 192)
    mc = q.MonteCarlo(dec, s.enc, seed=SEED)
    for bad in (0.0, 0.5, -0.1, 0.7, float("nan")):
        with pytest.raises(q.QldpcError) as e:
            mc.run(bad, 0, 192)
        assert e.value.status == -6, bad
    assert counters(mc.run(QBER["peg"], 0, 192)) == ctr
    for bad in (-0.01, 1.0):
        with pytest.raises(q.QldpcError) as e:
            mc.frames(0, 4, bad)
        assert e.value.status == -6
    assert mc.frames(0, 4, 0.0)[2].shape == (4, 32)                       # [0, 1) in the frame calls: 0 is no flips
    for kw in (dict(batch=193), dict(batch=-1), dict(fail_cap=0), dict(parity_ber=1.0)):
        with pytest.raises(q.QldpcError) as e:
            q.MonteCarlo(dec, s.enc, seed=SEED, **kw)
        assert e.value.status == -6, kw
    with pytest.raises(q.QldpcError):
        q.MonteCarlo(dec, setups("ira").enc, seed=SEED)                   # an encoder of another code
    small = q.MonteCarlo(dec, s.enc, seed=SEED, batch=100, fail_cap=5)    # the same decoder serves a following good object
    r = small.run(QBER["peg"], 0, 192)
    assert counters(r) == ctr and r["batches"] == 2 and small.device_bytes > 0
    kept = small.failed_frames()
    assert kept.size == 5 and r["frame_errors"] > 5 and (np.diff(kept.astype(np.int64)) > 0).all() and (kept < 100).all()
    assert counters(mc.run(QBER["peg"], 0, 192)) == ctr
