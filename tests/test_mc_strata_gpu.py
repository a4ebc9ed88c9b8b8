"""Fixed-weight error strata on the device (qldpc_mc_weight_frames_dev, qldpc_mc_strata): the rows of the kernel mc_channel_weight against the
host mirror word for word and against the BSC frames of MonteCarlo.frames, and every stratum row and histogram of MonteCarlo.strata against
numpy over mc_weight_frames_host -> encoder -> LLRs -> CPU oracle -> the schedule of tests/mc_sweep_ref.py.  Exact equality everywhere."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import mc_ref
import mc_strata_ref
import mc_sweep_ref
from mc_oracle import COUNTERS as ROW, KINDS, N_ITE, QBER, ROOT, SEED, SIM, frames_reference, row_of, same_rows, setups, sim_rows, u32  # noqa: F401 (setups is a fixture)

pytestmark = pytest.mark.gpu
FAR = 2 ** 32 - 100
# six weights per code across the step of P_f(w), chosen by the scan recorded in the docstring of test_rows_equal_the_oracle_and_the_schedule;
# every stratum is decoded with |LLR| = bsc_llr(QBER[name]), the operating points of test_mc_gpu
WEIGHTS = {"peg": (100, 124, 128, 132, 136, 170), "ira": (20, 40, 46, 52, 58, 90)}
MAX_FRAMES = 192


def strata_reference(s, kind, weights, C_, S, max_frames, max_fe, first=0, erased=()):
    """the schedule of mc_sweep_ref over the oracle's failures of frames [first, first + max_frames) of every weight, and the rows it leads to"""
    per = [frames_reference(s, kind, ("weight", w, QBER[s.name]), first, max_frames, erased) for w in weights]
    sch = mc_sweep_ref.schedule(np.array([f["be"] > 0 for f in per]), C_, S, max_frames, max_fe)
    rows = [row_of(s, f, int(n)) for f, n in zip(per, sch["frames"])]
    return sch, rows


def same_strata(res, hist, sch, rows, weights):
    def strata(st):
        assert st.shape == (len(weights),) and (st["weight"] == np.array(weights)).all()
        assert (st["channel_flips"] == st["frames"] * st["weight"].astype(np.uint64)).all()      # the kernel's weight, counted by the monitor kernel
        assert res["channel_ms"] > 0
    same_rows(res, "strata", hist, sch, rows, strata)


@pytest.mark.parametrize("name", ["peg", "ira"])
@pytest.mark.parametrize("first,n", [(0, 192), (FAR, 192), (3, 70)])
def test_device_rows_equal_the_host_mirror(q, setups, name, first, n):
    s = setups(name)
    mc = q.MonteCarlo(s.decoder("flood"), s.enc, seed=SEED)
    ref_cw = None
    for weight in (0, 1, 48, s.K):                                                        # s.K = every channel VN
        for key_bits in (32, 4, 1):
            info, cw, rx = (u32(t) for t in mc.weight_frames(first, n, weight, key_bits))
            ref_info, ref_flips = q.mc_weight_frames_host(s.K, s.N, SEED, weight, first, n, key_bits, info_bits_pos=s.pos)
            if ref_cw is None:
                ref_cw = mc_ref.pack(s.codewords(ref_info))
            assert info.shape == ref_info.shape and (info == ref_info).all()
            assert cw.shape == ref_cw.shape and (cw == ref_cw).all()
            assert (rx ^ cw == ref_flips).all(), (weight, key_bits)
            assert mc_ref.popcount(rx ^ cw) == n * weight
    # the identity with the BSC: the flip row of a frame with c flips is the fixed-weight row of that frame at weight c
    _, cw, rx = (u32(t) for t in mc.frames(first, n, QBER[name]))
    bsc = cw ^ rx
    counts = np.unpackbits(bsc.view(np.uint8), axis=1).sum(1)
    some = sorted(set(counts.tolist()))[::4]
    assert len(some) >= 3
    for c in some:
        _, wcw, wrx = (u32(t) for t in mc.weight_frames(first, n, c))
        assert ((wcw ^ wrx)[counts == c] == bsc[counts == c]).all() and (wcw == cw).all()


def test_final_pass_in_several_trips(q):
    """N = 8300: 260 codeword words, so the final pass of a workgroup of 256 lanes takes two trips, the second with four live lanes, and the
    last word holds 12 VNs.  The class map spreads 6640 channel VNs over the whole frame (every fifth VN is pinned, with dirty parity), so the
    second trip holds channel VNs too: at key_bits = 2 a group of equal keys holds about 1660 VNs and spans lanes, waves and both trips, and
    the running count of equal keys has to cross the trip boundary.  Generation only."""
    code = q.Code.ira(8300, 6600)
    enc = q.Encoder(code, "IRA")
    K, N, first = enc.K, code.N, FAR + 90
    assert (K, N) == (6600, 8300) and N % 32 != 0 and (N + 31) // 32 > 256
    cls = np.where(np.arange(N) % 5 == 4, 1, 0).astype(np.uint8)
    chan = np.nonzero(cls == 0)[0]
    mask = mc_ref.pack((cls == 0)[None, :])
    dec = q.Decoder(code, K, 2, info_bits_pos=enc.info_bits_pos, rule="NMS", rule_param=0.75, n_frames=16)
    mc = q.MonteCarlo(dec, enc, vn_class=cls, seed=SEED, parity_ber=0.05)
    for weight in (0, 7, 166, 6600):
        for key_bits in (32, 2):
            _, cw, rx = (u32(t) for t in mc.weight_frames(first, 16, weight, key_bits))
            ref = q.mc_weight_frames_host(K, N, SEED, weight, first, 16, key_bits, vn_class=cls, parity_ber=0.05)[1]
            assert (rx ^ cw == ref).all(), (weight, key_bits)
            assert mc_ref.popcount(ref & mask) == 16 * weight and mc_ref.popcount(ref[:, 256:] & ~mask[:, 256:]) > 0      # pinned flips in the second trip
    key = mc_strata_ref.keys(N, SEED, first, 16, 2)[1]
    taken = mc_ref.unpack(q.mc_weight_frames_host(K, N, SEED, 166, first, 16, 2, vn_class=cls)[1], N)
    for f in range(16):                                                                   # the boundary groups at key_bits = 2 span both trips
        for weight in (166, 6600):
            at = chan[key[f, chan] == np.sort(key[f, chan])[weight - 1]]
            assert at.size > 1000 and at.min() < 64 * 32 and at.max() >= 256 * 32
        assert taken[f, chan].sum() == 166 and not taken[f, 256 * 32:].any()               # weight 166: the lowest VNs of the group, none from the second trip


@pytest.mark.parametrize("max_fe", [0, 5])
@pytest.mark.parametrize("batch,chunk", [(192, 8), (70, 64)])
@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("name", ["peg", "ira"])
def test_rows_equal_the_oracle_and_the_schedule(q, setups, name, kind, batch, chunk, max_fe):
    """Six weights, frames [0, 192) of each, |LLR| of QBER[name]: every counter, every histogram row, last round and closing reason against the
    oracle's frames fed through mc_sweep_ref.schedule, on batch 192 with chunk 8 (24 slots) and on batch 70 with chunk 64 (one slot, six
    lanes of the batch idle), without a stop rule and with max_frame_errors = 5.  The weights were chosen by a scan with the CPU oracle over the
    frames of this test (frames [0, 192) of SEED, the encoder's codewords, NMS 0.75, 20 iterations, the layered kind in the code's layer order);
    frame errors of 192 per weight:
      PEGReg504x1008   w      96 100 104 108 112 116 120 124 128 132 136 140 144 150 160 170      (|LLR| of QBER 0.26)
                       flood   0   0   0   0   0   3   8  32  75 147 182 192 192 192 192 192
                       hlay    0   0   0   0   0   0   0   0  16  43  98 155 187 192 192 192
                       i8      0   0   0   0   0   4  11  45 103 161 189 192 192 192 192 192
      IRA(2000, 1590)  w      20  30  36  40  43  46  49  52  55  58  62  66  70  80  90 100      (|LLR| of QBER 0.03)
                       flood   0   0   0   4  20  82 155 184 192 192 192 192 192 192 192 192
                       hlay    0   0   0   1   3  24  56 120 172 192 192 192 192 192 192 192
                       i8      0   0   0   3  18  84 152 182 191 192 192 192 192 192 192 192
    -> {100, 124, 128, 132, 136, 170} and {20, 40, 46, 52, 58, 90} give every kind a stratum without a failure, one where every frame fails and
    at least two in between; the conditions are asserted on the test's own reference."""
    s = setups(name)
    weights = WEIGHTS[name]
    full = [row_of(s, frames_reference(s, kind, ("weight", w, QBER[s.name]), 0, MAX_FRAMES), MAX_FRAMES)[0]["frame_errors"] for w in weights]
    print(name, kind, "frame errors of 192 per weight:", dict(zip(weights, full)))
    assert min(full) == 0 and max(full) == MAX_FRAMES and sum(0 < fe < MAX_FRAMES for fe in full) >= 2      # the rows are not trivial
    sch, rows = strata_reference(s, kind, weights, chunk, batch // chunk, MAX_FRAMES, max_fe)
    if max_fe:
        assert set(sch["closed_by"].tolist()) == {mc_sweep_ref.CLOSED_MAX_FE, mc_sweep_ref.CLOSED_MAX_FRAMES} and len(set(sch["frames"].tolist())) >= 2
    mc = q.MonteCarlo(s.decoder(kind), s.enc, seed=SEED, batch=batch)
    res = mc.strata(weights, QBER[name], max_frames=MAX_FRAMES, max_frame_errors=max_fe, chunk=chunk)
    same_strata(res, mc.strata_hist(), sch, rows, weights)
    before = mc.device_bytes
    res = mc.strata(weights, QBER[name], max_frames=MAX_FRAMES, max_frame_errors=max_fe, chunk=chunk)      # again: the same, and nothing allocated
    same_strata(res, mc.strata_hist(), sch, rows, weights)
    assert mc.device_bytes == before


@pytest.mark.parametrize("name,kind", [("peg", "flood"), ("ira", "hlay")])
def test_a_row_does_not_depend_on_its_neighbours(q, setups, name, kind):
    """a stratum's row alone, among other neighbours, with another batch and chunk, in another order and with repeated weights is the same row;
    two equal weights give two equal rows; a fixed puncture set is honoured and a frame index across 2^32 carried"""
    s = setups(name)
    weights = WEIGHTS[name]
    w = weights[2]
    ref = row_of(s, frames_reference(s, kind, ("weight", w, QBER[s.name]), 0, 100), 100)
    mc = q.MonteCarlo(s.decoder(kind), s.enc, seed=SEED, batch=192)

    def rows(ws, **kw):
        res = mc.strata(ws, QBER[name], max_frames=100, **kw)
        return res, mc.strata_hist()

    res, hist = rows([w])
    same_strata(res, hist, None, [ref], [w])
    assert res["rounds"] == 1 and res["strata"]["closed_by"][0] == q.MC_CLOSED_MAX_FRAMES      # chunk 0 = 64: 3 slots, the stratum needs 2
    res, hist = rows(weights, chunk=16)
    assert {k: int(res["strata"][k][2]) for k in ROW} == ref[0] and (hist[2] == ref[1]).all()
    mixed = [weights[5], w, weights[0], w, w]                                             # any order, repeats
    res, hist = rows(mixed, chunk=7)
    st = res["strata"]
    assert (st["weight"] == np.array(mixed)).all()
    for i in (1, 3, 4):
        assert {k: int(st[k][i]) for k in ROW} == ref[0] and (hist[i] == ref[1]).all()
    assert all(st[k][3] == st[k][4] == st[k][1] for k in ROW)                             # equal weights: equal rows
    small = q.MonteCarlo(s.decoder(kind, 96), s.enc, seed=SEED, batch=40)
    res = small.strata([weights[1], w], QBER[name], max_frames=100, chunk=13)
    assert {k: int(res["strata"][k][1]) for k in ROW} == ref[0] and (small.strata_hist()[1] == ref[1]).all()
    # the fixed set of set_puncture, and first_frame across 2^32
    fixed = np.nonzero(s.cls == 1)[0][::9].astype(np.int32)
    mc.set_puncture(fixed)
    res, hist = rows([weights[1], w], first_frame=FAR + 60, chunk=16)
    mc.set_puncture(None)
    far = row_of(s, frames_reference(s, kind, ("weight", w, QBER[s.name]), FAR + 60, 100, fixed), 100)
    assert {k: int(res["strata"][k][1]) for k in ROW} == far[0] and (hist[1] == far[1]).all()
    assert far[0] != ref[0]


def test_refusals_leave_the_last_rows_readable(q, setups):
    s = setups("peg")
    weights = WEIGHTS["peg"]
    sch, rows = strata_reference(s, "flood", weights, 8, 24, MAX_FRAMES, 5)
    mc = q.MonteCarlo(s.decoder("flood"), s.enc, seed=SEED, batch=192)
    good = dict(max_frames=MAX_FRAMES, max_frame_errors=5, chunk=8)
    assert mc.strata_stats().size == 0
    res = mc.strata(weights, 0.26, **good)
    hist = mc.strata_hist()
    same_strata(res, hist, sch, rows, weights)

    def refused(status, *args, **kw):
        with pytest.raises(q.QldpcError) as e:
            mc.strata(*args, **kw)
        assert e.value.status == status, (args, kw, e.value)
        assert (mc.strata_stats() == res["strata"]).all() and (mc.strata_hist() == hist).all()

    mc.set_awgn(sigma=0.8)
    refused(-8, weights, 0.26, **good)                                                    # a table in force
    mc.set_channel()
    refused(-6, (100, s.K + 1), 0.26, **good)                                             # a weight above the channel VNs
    refused(-6, (100, -1), 0.26, **good)
    refused(-6, weights, 0.5, **good)
    refused(-6, weights, 0.0, **good)
    refused(-6, [], 0.26, **good)
    refused(-6, [100] * (q.MC_SWEEP_MAX_POINTS + 1), 0.26, **good)
    refused(-6, weights, 0.26, max_frames=MAX_FRAMES, chunk=193)
    refused(-6, weights, 0.26, max_frames=MAX_FRAMES, chunk=-1)
    refused(-6, weights, 0.26, max_frames=0)
    refused(-6, weights, 0.26, key_bits=33, **good)
    refused(-6, weights, 0.26, key_bits=-1, **good)
    w = np.array(weights, np.int32)
    for where in ("reserved", "weights"):                                                 # through the C structure
        cfg, out = q.McStrataCfg(), q.McStrataResult()
        cfg.weights, cfg.n_strata, cfg.design_qber, cfg.max_frames = w.ctypes.data_as(q._ip), w.size, 0.26, 10
        if where == "reserved":
            cfg.reserved[1] = 1
        else:
            cfg.weights = None
        assert q._L.qldpc_mc_strata(mc._h, C.byref(cfg), C.byref(out)) == -1, where
        assert (mc.strata_stats() == res["strata"]).all() and (mc.strata_hist() == hist).all()
    with pytest.raises(q.QldpcError) as e:
        q._chk(q._L.qldpc_mc_strata_hist(mc._h, 6, None, 0), "strata_hist")                 # a stratum the last run did not have
    assert e.value.status == -6
    for bad, status in (((0, 4, s.K + 1, 0), -6), ((0, 4, -1, 0), -6), ((0, 4, 5, 33), -6), ((0, -1, 5, 0), -1)):
        with pytest.raises(q.QldpcError) as e:
            mc.weight_frames(*bad)
        assert e.value.status == status, bad
    again = mc.strata(weights, 0.26, **good)
    same_strata(again, mc.strata_hist(), sch, rows, weights)


def test_sweep_and_strata_keep_their_rows_apart(q, setups):
    """the two calls share the device rows: the histogram call of the one refuses after a run of the other and never returns its bins; the stat
    rows of both stay readable; a sweep gives the same rows before and after a strata run"""
    s = setups("peg")
    weights, qbers = WEIGHTS["peg"][1:4], (0.22, 0.26, 0.30)
    mc = q.MonteCarlo(s.decoder("flood"), s.enc, seed=SEED, batch=192)
    sweep = mc.sweep(qbers, max_frames=100, max_frame_errors=30, chunk=16)
    sweep_hist = mc.sweep_hist()
    with pytest.raises(q.QldpcError) as e:
        q._chk(q._L.qldpc_mc_strata_hist(mc._h, 0, None, 0), "strata_hist")
    assert e.value.status == -6                                                           # no strata run yet: no such stratum
    strata = mc.strata(weights, 0.26, max_frames=100, chunk=16)
    strata_hist = mc.strata_hist()
    assert (strata_hist.sum(1) == 100).all() and not (strata_hist == sweep_hist).all()
    with pytest.raises(q.QldpcError) as e:
        mc.sweep_hist()
    assert e.value.status == -8
    assert (mc.sweep_stats() == sweep["points"]).all() and (mc.strata_stats() == strata["strata"]).all()
    again = mc.sweep(qbers, max_frames=100, max_frame_errors=30, chunk=16)
    assert (again["points"] == sweep["points"]).all() and (mc.sweep_hist() == sweep_hist).all() and again["rounds"] == sweep["rounds"]
    with pytest.raises(q.QldpcError) as e:
        mc.strata_hist()
    assert e.value.status == -8
    assert (mc.strata_stats() == strata["strata"]).all()
    run = mc.run(0.26, 0, 100)                                                            # and the plain run next to both
    assert run["frames"] == 100
    redo = mc.strata(weights, 0.26, max_frames=100, chunk=16)
    assert (redo["strata"] == strata["strata"]).all() and (mc.strata_hist() == strata_hist).all()


def test_qldpc_sim_strata_prints_the_same_rows(q, setups):
    alist = os.path.join(ROOT, "tests", "golden", "PEGReg504x1008.alist")
    args = ["-a", alist, "-r", "NMS", "-p", "0.75", "-i", str(N_ITE), "-b", "192", "-S", str(SEED), "-f", "192", "-D"]
    got, text = sim_rows(args + ["-w", "120:140:4:0.26", "-E", "40", "-s", "0.20:0.26:0.03"])
    got = [r[:4] for r in got]                                                            # EP FRA BE FE
    s = setups("peg")
    mc = q.MonteCarlo(s.decoder("flood"), s.enc, seed=SEED)
    weights = list(range(120, 141, 4))
    res = mc.strata(weights, 0.26, max_frames=192, max_frame_errors=40)
    st = res["strata"]
    assert [tuple(int(x) for x in r) for r in got] == [(int(r["weight"]), int(r["frames"]), int(r["bit_errors"]), int(r["frame_errors"])) for r in st]
    assert len(set(r[1] for r in got)) > 1 and "# strata: 6 weights" in text
    lines = [l for l in text.splitlines() if l.startswith("# strata ber")]
    assert len(lines) == 3
    for l, qber in zip(lines, (0.20, 0.23, 0.26)):
        est = q.mc_strata_fer(s.K, weights, st["frames"], st["frame_errors"], qber)
        nums = [float(x.split()[0].rstrip(",")) for x in (l.split("FER ")[1], l.split("below ")[1], l.split("above ")[1], l.split("standard error ")[1])]
        assert nums == pytest.approx(list(est), rel=1e-5)                                 # the line prints seven digits
    for refused in (["-w", "120:140:4", "-W"], ["-w", "120:140:4", "-X", "1.6"], ["-w", "120:140:4", "-A", "2.0"], ["-w", "140:120:4"], ["-w", "1:2"]):
        r = subprocess.run([SIM] + args + refused, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "-w" in r.stderr, refused
    r = subprocess.run([SIM] + [a for a in args if a != "-D"] + ["-w", "120:140:4"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "-w" in r.stderr
