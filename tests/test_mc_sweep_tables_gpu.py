"""The sweep over operating points of a table channel on the device (qldpc_mc_sweep_tables, mc_soft_channel_slots): every point row and histogram
of MonteCarlo.sweep_tables against numpy over mc_llr_host -> CPU oracle -> the schedule of tests/mc_sweep_ref.py, and against set_channel +
set_puncture + run of the point alone; the state the call leaves; the reference's published fixed-point AWGN curve in one call; qldpc_sim -T.
Exact equality everywhere but the four 20 000-frame FERs, which are held against the band around the reference's published rows."""
import os
import subprocess

import numpy as np
import pytest

import matlab_fp
import mc_ref
import mc_soft_ref
import mc_sweep_ref
from mc_oracle import COUNTERS as ROW, KINDS, N_ITE, ROOT, SEED, SIM, counters, oracle, row_of, same_rows, setups, sim_rows, verdicts  # noqa: F401 (setups is a fixture)
from test_mc_soft_gpu import NR, _Nr

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden")
FAR = 2 ** 32 - 100
NAMES = ("q2", "awgn64", "awgn64b", "q256")          # 2, 64, 64 and 256 levels in one sweep
LABELS = (0.5, 1.5, 2.5, 3.5)
SIGMA_B = 1.5                                        # the second sigma of the 64-level table, see test_rows_equal_the_oracle_and_the_schedule
MAX_FE = {"peg": 40, "a1998": 100}


class _Case:
    """A code, its class map and its decoders, and the numpy reference of a table point over it: mc_frames_host -> encoder -> mc_llr_host(table) ->
    the erased VNs at 0 -> CPU oracle -> verdicts.  Computed once per argument set and left unchanged."""

    def __init__(self, q, O, name, code, enc, og, ogl, vn_class, parity_ber, decoder):
        self.q, self.O, self.name, self.code, self.enc, self.og, self.ogl = q, O, name, code, enc, og, ogl
        self.K, self.N, self.pos = enc.K, code.N, np.asarray(enc.info_bits_pos)
        self.vn_class, self.parity_ber, self.decoder = vn_class, parity_ber, decoder
        self.cls = mc_ref.classes(self.K, self.N, self.pos, vn_class)
        t = mc_soft_ref.tables(q)
        self.tables = {"q2": t["q2"], "awgn64": t["awgn64"], "awgn64b": q.mc_awgn_table(SIGMA_B), "q256": t["q256"]}
        self._ref = {}

    def frames(self, key, first, n):
        if ("llr", key, first, n) not in self._ref:
            q = self.q
            cw = self.enc.encode(mc_ref.unpack(q.mc_frames_host(self.K, self.N, SEED, 0.1, first, n, info_bits_pos=self.pos)[0], self.K))
            llr, flip_w = q.mc_llr_host(self.K, self.N, SEED, self.tables[key], first, n, cw_words=mc_ref.pack(cw), info_bits_pos=self.pos,
                                        vn_class=self.vn_class, parity_ber=self.parity_ber)
            self._ref["llr", key, first, n] = (cw, llr, mc_ref.unpack(flip_w, self.N))
        return self._ref["llr", key, first, n]

    def reference(self, kind, key, first, n, erased=()):
        erased = tuple(int(v) for v in erased)
        if (kind, key, first, n, erased) not in self._ref:
            cw, llr, flips = self.frames(key, first, n)
            llr = llr.copy()
            llr[:, list(erased)] = 0.0
            self._ref[kind, key, first, n, erased] = verdicts(oracle(self, kind, llr), cw, self.pos, flips, self.cls == 0)
        return self._ref[kind, key, first, n, erased]

    def sweep_reference(self, kind, first, C_, S, max_frames, max_fe):
        """the schedule of mc_sweep_ref over the oracle's failures of frames [first, first + max_frames) of every point, and the rows it leads to"""
        per = [self.reference(kind, key, first, max_frames) for key in NAMES]
        sch = mc_sweep_ref.schedule(np.array([f["be"] > 0 for f in per]), C_, S, max_frames, max_fe)
        return sch, [row_of(self, f, int(n)) for f, n in zip(per, sch["frames"])]

    def mc(self, kind, batch, n_frames=192):
        return self.q.MonteCarlo(self.decoder(kind, n_frames), self.enc, vn_class=self.vn_class, seed=SEED, batch=batch, parity_ber=self.parity_ber)

    def sweep(self, mc, **kw):
        return mc.sweep_tables([self.tables[k] for k in NAMES], labels=LABELS, **kw)


@pytest.fixture(scope="module")
def cases(q, O, setups):
    """"peg": PEGReg504x1008 with the harness's classes (N = 1 008: 256 quads, one workgroup per frame slot).  "a1998": 1998.5.3.2665.alist with the
    `mixed` class map of mc_soft_ref (channel, pinned with parity_ber 0.25, punctured): N % 4 = 2, so every other LLR row starts off a 16-byte
    boundary and its last quad is cut, and 504 quads are two workgroups per slot, the second ragged."""
    made = {}

    def get(name):
        if name in made:
            return made[name]
        if name == "peg":
            s = setups("peg")
            made[name] = _Case(q, O, name, s.code, s.enc, s.og, s.ogl, None, 0.0, s.decoder)
            return made[name]
        code = q.Code.from_alist(os.path.join(GOLD, "1998.5.3.2665.alist"))
        enc = q.Encoder(code, "IDENTITY")
        assert code.N == 1998 and code.N % 4 == 2 and 8 * ((code.N + 31) // 32) == 504
        var, chk = code.edges()
        order, _, _ = code.layer_order()                             # the layered oracle visits the checks in the code's layer order
        inv = np.empty(code.M, np.int32)
        inv[order] = np.arange(code.M, dtype=np.int32)
        idx = np.argsort(inv[chk], kind="stable")
        og, ogl = O.Graph.from_edges(code.N, code.M, var, chk), O.Graph.from_edges(code.N, code.M, var[idx], inv[chk][idx])
        decs = {}

        def decoder(kind, n_frames=192):
            if (kind, n_frames) not in decs:
                decs[kind, n_frames] = q.Decoder(code, enc.K, N_ITE, info_bits_pos=enc.info_bits_pos, rule="NMS", rule_param=0.75, n_frames=n_frames, **KINDS[kind])
            return decs[kind, n_frames]

        made[name] = _Case(q, O, name, code, enc, og, ogl, mc_soft_ref.mixed_classes(code.N), 0.25, decoder)
        return made[name]
    return get


def same_points(res, hist, sch, rows, labels=LABELS, n_punct=None):
    def points(pts):
        assert (pts["qber"] == np.array(labels)).all()                 # the label comes back in the qber field, uninterpreted
        assert (pts["n_punct"] == (np.zeros(len(labels)) if n_punct is None else np.array(n_punct))).all()
    same_rows(res, "points", hist, sch, rows, points)


def run_row(mc, first, n):
    r = mc.run(0.1, first, n)
    return {k: int(r[k]) for k in ROW}, mc.iter_hist()


@pytest.mark.parametrize("name,first,kind", [(n, 0, k) for n in ("peg", "a1998") for k in sorted(KINDS)] + [("a1998", FAR + 97, "flood")])
def test_rows_equal_the_oracle_and_the_schedule(cases, name, first, kind):
    """Four tables of different level counts in one sweep, batch 192, chunk 32 (6 slots: 2 2 1 1 chunks while four points are open), max_frames
    150 = 4 chunks + 22 frames: every row, histogram, last round and closing reason against numpy.  From FAR + 97 the frame indices carry across
    the 32-bit index words inside the first chunk (the carry is the channel kernel's and the slot table's, not the decoder's: one kind).

    The second sigma of the 64-level table and max_frame_errors come from a scan with the oracle on the CPU (frames [0, 150) of SEED, NMS 0.75, 20
    iterations, the encoder's codewords); failed frames of the points (q2, awgn64 at 0.8414, awgn64 at 1.5, q256) after 32 / 64 / 96 / 128 / 150:
      PEGReg504x1008, harness classes   flood  0 | 0 | 13 26 41  53  64 | 32 64 96 128 150
                                        hlay   0 | 0 |  6 12 22  33  38 | all
                                        i8     0 | 0 | 27 56 85 112 132 | all
      1998.5.3.2665, `mixed` classes    every frame of every point fails: a third of the VNs is punctured, 1.7 of the 5 VNs of a check on
                                        average, which belief propagation does not get past.  The rows there still pin every LLR through the
                                        bit errors, the iteration counts and the flips (a quarter of the pinned VNs among them)
    -> sigma 1.5 fails between a quarter and nine tenths of the frames for every kind.  max_frame_errors 40 on PEG: q256 closes after round 1 (64
    frames), the 8-bit decoder's third point with it, the others run to 150 through the ragged chunk in round 2.  100 on 1998: points 0 and 1
    (two chunks per round) close after round 1 at 128 frames, points 2 and 3 (one chunk per round until then) take three chunks each in round 2
    and close at 150.  What the shape is meant to reach is asserted on the test's own reference before the device is asked."""
    s = cases(name)
    sch, rows = s.sweep_reference(kind, first, 32, 6, 150, MAX_FE[name])
    print(name, kind, first, sch, [r[0]["frame_errors"] for r in rows])
    assert (sch["closed_by"] == mc_sweep_ref.CLOSED_MAX_FE).any() and sch["rounds"] >= 3       # the noisiest point closes early; several rounds
    assert ((sch["closed_by"] == mc_sweep_ref.CLOSED_MAX_FRAMES) & (sch["frames"] == 150)).any()      # ... and one ends through the ragged chunk
    assert all(r[0]["channel_flips"] > 0 for r in rows)
    mc = s.mc(kind, 192)
    res = s.sweep(mc, first_frame=first, max_frames=150, max_frame_errors=MAX_FE[name], chunk=32)
    same_points(res, mc.sweep_hist(), sch, rows)
    before = mc.device_bytes
    res = s.sweep(mc, first_frame=first, max_frames=150, max_frame_errors=MAX_FE[name], chunk=32)      # again: the same, and nothing allocated
    same_points(res, mc.sweep_hist(), sch, rows)
    assert mc.device_bytes == before


@pytest.mark.parametrize("kind,chunk,P", [("flood", 1, 4), ("hlay", 96, 4), ("i8", 32, 7)])
def test_a_row_is_the_points_own_run(cases, kind, chunk, P):
    """nested puncture prefixes (0, 20, 40, 60 VNs; 0 .. 60 in tens for seven points) of a seeded permutation of the parity VNs on top of a fixed
    set, batch 96: chunk 1 (96 slots), chunk = batch (one slot: the points one after the other) and seven points on three slots, so that points
    wait a round.  Every row and histogram equals set_channel(table_q) + set_puncture(fixed + prefix_q) + run(., first_frame, frames_q) on the same
    object; the third point also against the oracle with those VNs at LLR 0."""
    s = cases("peg")
    first = 1000
    keys = [NAMES[i % 4] for i in range(P)]
    labels, n_punct = np.arange(P) * 0.25 - 1.0, ((0, 20, 40, 60) if P == 4 else tuple(range(0, 70, 10)))
    perm = np.random.default_rng(7).permutation(np.nonzero(s.cls == 1)[0]).astype(np.int32)
    order, fixed = perm[:n_punct[-1]], np.sort(perm[-5:])
    mc = s.mc(kind, 96, 96)
    mc.set_puncture(fixed)
    res = mc.sweep_tables([s.tables[k] for k in keys], labels, n_punct, order, first_frame=first, max_frames=100, max_frame_errors=30, chunk=chunk)
    hist, pts = mc.sweep_hist(), res["points"]
    print(kind, chunk, pts)
    assert len(set(pts["frames"].tolist())) >= 2 and res["rounds"] >= 3
    if chunk != 1:
        assert len(set(pts["last_round"].tolist())) >= 3              # points waited for a slot
    rows = []
    for i in range(P):
        mc.set_channel(*s.tables[keys[i]])
        mc.set_puncture(np.sort(np.concatenate([fixed, order[:n_punct[i]]])))
        rows.append(run_row(mc, first, int(pts["frames"][i])))
    same_points(res, hist, None, rows, labels, n_punct)
    erased = np.sort(np.concatenate([fixed, order[:n_punct[2]]]))
    row, h = row_of(s, s.reference(kind, keys[2], first, 100, erased), int(pts["frames"][2]))
    assert {k: int(pts[k][2]) for k in ROW} == row and (hist[2] == h).all()


def test_state_around_a_table_sweep(q, cases):
    """the call neither needs nor changes the table of set_channel; whose rows the device holds; refusals"""
    s = cases("peg")
    tabs = [s.tables[k] for k in NAMES]
    fresh = s.mc("flood", 96, 96)
    bsc = run_row(fresh, 0, 96)
    mc = s.mc("flood", 96, 96)
    strata = mc.strata([100, 130], 0.26, max_frames=40)
    assert mc.strata_hist().shape == (2, N_ITE + 1)
    mc.set_channel(*s.tables["awgn64b"])
    soft = run_row(mc, 0, 96)
    assert soft[0] != bsc[0] and 0 < soft[0]["frame_errors"] < 96
    before = mc.device_bytes
    res = s.sweep(mc, max_frames=100, max_frame_errors=30, chunk=16)
    hist = mc.sweep_hist()
    assert hist.shape == (4, N_ITE + 1) and (hist.sum(1) == res["points"]["frames"]).all()
    table_bytes = 12 + 2 * 255 * 4 + 256 * 4
    assert mc.device_bytes - before >= 4 * table_bytes                    # the tables (the LLR rows were set_channel's, the sweep's own rows come on top)
    again = run_row(mc, 0, 96)
    assert again[0] == soft[0] and (again[1] == soft[1]).all()            # the table in force still drives run
    with pytest.raises(q.QldpcError) as e:
        mc.sweep((0.22, 0.26), max_frames=50)                             # ... and still refuses the BSC sweep
    assert e.value.status == -8
    with pytest.raises(q.QldpcError) as e:
        mc.strata_hist()                                                  # the device rows hold the sweep
    assert e.value.status == -8
    assert (mc.strata_stats() == strata["strata"]).all()
    grown = mc.device_bytes
    assert s.sweep(mc, max_frames=100, max_frame_errors=30, chunk=16)["points"].tolist() == res["points"].tolist() and mc.device_bytes == grown
    four = res
    res = mc.sweep_tables(tabs + tabs[:2], max_frames=100, max_frame_errors=30, chunk=16)      # P = 6: the tables grow by two
    assert mc.device_bytes == grown + 2 * table_bytes and res["points"].size == 6
    hist = mc.sweep_hist()

    def refused(status, *args, **kw):
        with pytest.raises(q.QldpcError) as e:
            mc.sweep_tables(*args, **kw)
        assert e.value.status == status, (args, kw, e.value)
        assert (mc.sweep_stats() == res["points"]).all() and (mc.sweep_hist() == hist).all()

    c0, c1, value = s.tables["awgn64"]
    falling = c0.copy()
    falling[5] = falling[4] - 1
    refused(-6, tabs + [(c0[:0], c1[:0], value[:1])], max_frames=50)
    refused(-1, tabs + [(falling, c1, value)], max_frames=50)
    refused(-6, tabs, max_frames=50, chunk=97)
    refused(-6, tabs, max_frames=0)
    refused(-6, tabs, n_punct=(0, 0, 0, 1), max_frames=50)
    refused(-1, tabs, n_punct=(0, 0, 0, 1), punct_order=[3, 3], max_frames=50)
    refused(-6, [], max_frames=50)
    mc.set_channel()                                                      # no table in force: run is the BSC's, the rows of the sweep stay
    back = run_row(mc, 0, 96)
    assert back[0] == bsc[0] and (back[1] == bsc[1]).all()
    assert (mc.sweep_stats() == res["points"]).all() and (mc.sweep_hist() == hist).all()
    none = s.mc("flood", 96, 96)                                          # an object that never had a table
    got = s.sweep(none, max_frames=100, max_frame_errors=30, chunk=16)
    assert got["points"].tolist() == four["points"].tolist()
    after = run_row(none, 0, 96)
    assert after[0] == bsc[0] and (after[1] == bsc[1]).all()
    with pytest.raises(q.QldpcError) as e:
        none.llr_frames(0, 2)                                             # still no table in force
    assert e.value.status == -8


@pytest.fixture(scope="module")
def nr(q, O):
    return _Nr(q, O)


def test_the_published_curve_in_one_call(q, nr):
    """The four Eb/N0 points the reference publishes for NR_2_6_52 (tests/golden/matlab_fp_fer.json), 20 000 frames each, from ONE call: every FER
    inside the project's band around the published row (matlab_fp.band; tests/matlab_fp.py records 0.844 / 0.359 / 0.030 / 0.0019 for the CPU
    decoder), and the 2.35 dB row counter for counter the run of that point alone."""
    s = nr
    ebno = [1.0, 1.5, 2.0, 2.35]
    res = s.mc.sweep_awgn(ebno, s.rate, max_frames=20000)
    pts, hist = res["points"], s.mc.sweep_hist()
    assert (pts["qber"] == np.array(ebno)).all() and (pts["frames"] == 20000).all() and (pts["closed_by"] == q.MC_CLOSED_MAX_FRAMES).all()
    for i, e in enumerate(ebno):
        lo, hi = matlab_fp.band(NR, e, 20000)
        print("NR_2_6_52 @ %.2f dB: %d frame errors of 20000 (published FER %g), band %g .. %g" % (e, pts["frame_errors"][i], matlab_fp.published(NR, e)["fer"], lo, hi))
    for i, e in enumerate(ebno):
        lo, hi = matlab_fp.band(NR, e, 20000)
        assert lo <= pts["frame_errors"][i] / 20000.0 <= hi, e
    s.mc.set_awgn(ebno_db=2.35, rate=s.rate)
    own = s.mc.run(0.1, 0, 20000)
    assert {k: int(pts[k][3]) for k in ROW} == counters(own) and (hist[3] == s.mc.iter_hist()).all()
    s.mc.set_channel()


def test_qldpc_sim_table_sweep_prints_the_same_rows(q, nr):
    s = nr
    args = ["-q", s.path, "-G", "QC", "-r", "OMS", "-p", "2", "-i", "20", "-l", "-n", "-Q", "8", "-c", "1", "-S", str(SEED), "-D", "-z", "-u", str(2 * s.z),
            "-b", "192", "-f", "192"]
    res = s.mc.sweep_awgn([1.5, 2.0], s.rate, max_frames=192)
    got, text = sim_rows(args + ["-T", "1.5:2.0:0.5"])
    assert "# table sweep: 2 points" in text and len(got) == 2
    assert [(float(r[0]), int(r[1]), int(r[2]), int(r[3])) for r in got] == [(float(p["qber"]), int(p["frames"]), int(p["bit_errors"]), int(p["frame_errors"]))
                                                                             for p in res["points"]]
    assert int(got[0][3]) > int(got[1][3]) > 0
    assert [r[:6] for r in sim_rows(args + ["-T", "1.5:2.0:0.5:3:31"])[0]] == [r[:6] for r in got]      # SIM_THR is a time
    one, _ = sim_rows(args + ["-A", "2.0"])                               # the row of -A at that point
    assert [r[:4] for r in one] == [got[1][:4]]
    for extra in (["-A", "1.5"], ["-W"], ["-X", "1.3"], ["-w", "1:2:1"], ["-B", "4:2"]):
        p = subprocess.run([SIM] + args + ["-T", "1.5:2.0:0.5"] + extra, capture_output=True, text=True, timeout=60)
        assert p.returncode != 0 and "-T" in p.stderr, extra
    p = subprocess.run([SIM] + [a for a in args if a != "-D"] + ["-T", "1.5:2.0:0.5"], capture_output=True, text=True, timeout=60)
    assert p.returncode != 0 and "-T" in p.stderr
