"""Quantised soft-output channels of the Monte-Carlo loop on the device (qldpc_mc_set_channel, mc_soft_channel): the LLR rows and the rx
rows against the host mirror float for float and word for word, every counter of MonteCarlo.run / .search against numpy over mc_llr_host ->
CPU oracle -> compare, and the reference's fixed-point MATLAB experiment run by the loop.  Exact equality everywhere but the one
20 000-frame FER, which is held against the band around the reference's published row."""
import os
import subprocess

import numpy as np
import pytest

import matlab_fp
import mc_ref
import mc_search_ref
import mc_soft_ref
from mc_oracle import N_ITE, PATTERN_ROW, ROOT, SEED, SIM, counters, oracle, setups, sim_rows, tally, u32, verdicts  # noqa: F401 (setups is a fixture)

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden")
FAR = 2 ** 32 - 100
SIGMA, SIGMA_DEAD = 0.8414, 1.0            # Eb/N0 1.5 dB at rate 1/2; the scan is in the docstring of test_run_equals_the_oracle_counter_for_counter
KINDS = {"flood": dict(schedule="flooding"), "hlay": dict(schedule="hlayered"), "i8": dict(schedule="flooding", msg_dtype="i8", quant_scale=1.0)}
ROW = PATTERN_ROW[1:]
NR = "NR_2_6_52"


class _Peg:
    """PEGReg504x1008 with the IDENTITY encoder, every VN through the channel: the shared setup "peg" with another class map"""

    def __init__(self, s):
        self.s, self.chan = s, np.zeros(s.N, np.uint8)

    def __getattr__(self, name):
        return getattr(self.s, name)

    def soft_decoder(self, kind, n_frames=64):
        key = ("soft", kind, n_frames)
        if key not in self._dec:
            self._dec[key] = self.q.Decoder(self.code, self.K, N_ITE, info_bits_pos=self.pos, rule="NMS", rule_param=0.75, n_frames=n_frames, **KINDS[kind])
        return self._dec[key]

    def oracle(self, kind, llr):
        return oracle(self.s, kind, llr, quant_scale=1.0)

    def frames(self, sigma, first, n):
        """(codeword bits, LLRs, flip bits) of frames [first, first + n) through the 6-bit AWGN table at sigma; computed once"""
        key = ("awgn", sigma, first, n)
        if key not in self._ref:
            q = self.q
            cw = self.codewords(q.mc_frames_host(self.K, self.N, SEED, 0.1, first, n, info_bits_pos=self.pos)[0])
            llr, flip_w = q.mc_llr_host(self.K, self.N, SEED, q.mc_awgn_table(sigma), first, n, cw_words=mc_ref.pack(cw), vn_class=self.chan)
            self._ref[key] = (cw, llr, mc_ref.unpack(flip_w, self.N))
        return self._ref[key]

    def soft_reference(self, kind, sigma, first, n):
        key = ("soft", kind, sigma, first, n)
        if key not in self._ref:
            cw, llr, flips = self.frames(sigma, first, n)
            self._ref[key] = tally(verdicts(self.oracle(kind, llr), cw, self.pos, flips, self.chan == 0), self.N, first)
        return self._ref[key]


@pytest.fixture(scope="module")
def peg(setups):
    return _Peg(setups("peg"))


@pytest.fixture(scope="module")
def a1998(q):
    """1998.5.3.2665.alist: N = 1998, so N % 4 = 2 (every other row starts off a 16-byte boundary, the last quad is cut) and N % 32 = 14"""
    class S:
        pass
    s = S()
    s.code = q.Code.from_alist(os.path.join(GOLD, "1998.5.3.2665.alist"))
    s.enc = q.Encoder(s.code, "IDENTITY")
    s.K, s.N, s.pos = s.enc.K, s.code.N, s.enc.info_bits_pos
    assert s.N == 1998 and s.N % 4 == 2 and s.N % 32
    s.dec = q.Decoder(s.code, s.K, N_ITE, info_bits_pos=s.pos, rule="NMS", rule_param=0.75, n_frames=8)
    s.codewords = lambda info_words: s.enc.encode(mc_ref.unpack(info_words, s.K))
    return s


@pytest.fixture(scope="module")
def tables(q):
    return mc_soft_ref.tables(q)


@pytest.mark.parametrize("name", ["peg", "a1998"])
@pytest.mark.parametrize("first", [0, FAR + 97])
@pytest.mark.parametrize("shape", ["awgn64", "q2", "q256", "mixed"])
def test_llr_frames_equal_the_host_mirror(q, peg, a1998, tables, name, first, shape):
    """5 frames (several workgroups; from FAR + 97 they cross 2^32) of the encoder's codewords: the harness's classes (info VNs through the
    channel, parity pinned) and, `mixed`, a class map of 0 / 1 / 2 with dirty parity through the 256-level table"""
    s = peg if name == "peg" else a1998
    dec = s.soft_decoder("flood") if name == "peg" else s.dec
    cls, parity_ber, table = (mc_soft_ref.mixed_classes(s.N), 0.25, tables["q256"]) if shape == "mixed" else (None, 0.0, tables[shape])
    mc = q.MonteCarlo(dec, s.enc, vn_class=cls, seed=SEED, parity_ber=parity_ber)
    mc.set_channel(*table)
    info, cw, rx, llr = mc.llr_frames(first, 5)
    info, cw, rx, llr = u32(info), u32(cw), u32(rx), llr.cpu().numpy()
    ref_info = q.mc_frames_host(s.K, s.N, SEED, 0.1, first, 5, info_bits_pos=s.pos)[0]
    ref_cw = mc_ref.pack(s.codewords(ref_info))
    ref_llr, ref_flips = q.mc_llr_host(s.K, s.N, SEED, table, first, 5, cw_words=ref_cw, info_bits_pos=s.pos, vn_class=cls, parity_ber=parity_ber)
    assert (info == ref_info).all() and (cw == ref_cw).all() and ref_cw.any()
    assert llr.shape == ref_llr.shape == (5, s.N) and (llr.view(np.uint32) == ref_llr.view(np.uint32)).all()
    assert rx.shape == ref_flips.shape and (rx == ref_cw ^ ref_flips).all() and ref_flips.any()
    if shape == "mixed":
        f = mc_ref.unpack(ref_flips, s.N)
        assert f[:, cls == 1].any() and not f[:, cls == 2].any() and (ref_llr[:, cls == 2] == 0).all()


@pytest.mark.parametrize("kind", sorted(KINDS))
@pytest.mark.parametrize("n", [192, 150])
def test_run_equals_the_oracle_counter_for_counter(q, peg, kind, n):
    """Every counter, the histogram and the failed-frame list of a run through the 6-bit AWGN table (sigma = 0.8414: Eb/N0 1.5 dB at rate 1/2;
    every VN a channel VN) in batches of 64 -- 192 = 3 batches, 150 ends ragged -- against numpy over mc_llr_host -> oracle -> compare.  Every
    decoder kind must fail between 10 % and 90 % of the 192 frames (asserted first).  The scan with the oracle on the CPU over the Philox
    frames [0, 192) of SEED (NMS 0.75, 20 iterations, the 8-bit decoder with quant_scale 1; failed frames of 192), with the codewords of the
    source's info words and, for comparison, the all-zero codeword, on which floor()'s bias towards negative values costs more:
          sigma            0.8414   1.0
          flood  random        96   192
          hlay   random        61   192
          i8     random       117   192
          flood  zero         165   192
          hlay   zero         143   192
          i8     zero         177   192
    -> 0.8414 for the counters, 1.0 as the point where every frame fails (test_stop_rule_with_a_table)."""
    s = peg
    ctr, hist, failed = s.soft_reference(kind, SIGMA, 0, n)
    print(kind, n, ctr)
    if n == 192:
        assert 0.1 * 192 <= ctr["frame_errors"] <= 0.9 * 192
    assert 0 < ctr["channel_flips"] < ctr["channel_bits"] == n * s.N
    mc = q.MonteCarlo(s.soft_decoder(kind), s.enc, vn_class=s.chan, seed=SEED, batch=64)
    assert mc.set_awgn(sigma=SIGMA) == SIGMA
    res = mc.run(0.1, 0, n)
    print(kind, n, counters(res))
    assert counters(res) == ctr
    assert res["batches"] == 3 and res["next_frame"] == n and res["decode_ms"] > 0
    assert (mc.iter_hist() == hist).all() and int(hist.sum()) == n
    assert (mc.failed_frames() == failed).all()
    if n == 150:                                                          # qber is validated as before, and otherwise ignored
        assert counters(mc.run(0.4, 0, n)) == ctr
        for bad in (0.0, 0.5, float("nan")):
            with pytest.raises(q.QldpcError) as e:
                mc.run(bad, 0, n)
            assert e.value.status == -6


def test_stop_rule_with_a_table(q, peg):
    s = peg
    ctr, _, _ = s.soft_reference("flood", SIGMA_DEAD, 0, 192)
    assert ctr["frame_errors"] == 192                                     # the oracle fails every frame here
    mc = q.MonteCarlo(s.soft_decoder("flood"), s.enc, vn_class=s.chan, seed=SEED, batch=64)
    mc.set_awgn(ebno_db=0.0, rate=0.5)
    assert abs(q.mc_awgn_sigma(0.0, 0.5) - SIGMA_DEAD) < 1e-12
    r = mc.run(0.1, 0, 640, max_frame_errors=1)
    assert r["batches"] == 1 and r["frames"] == 64 and r["frame_errors"] == 64 and r["next_frame"] == 64
    r = mc.run(0.1, 0, 640, max_frame_errors=65)                          # reached inside the second batch: stops at its end
    assert r["batches"] == 2 and r["frames"] == 128
    r = mc.run(0.1, 0, 192, max_frame_errors=0)
    assert r["batches"] == 3 and counters(r) == ctr


class _Nr:
    """The experiment of the reference's fixed-point MATLAB sims (tests/matlab_fp.py) as the loop runs it: NR_2_6_52 with the QC encoder, the first
    2 z = 104 VNs punctured, every other VN through the 6-bit AWGN table, the all-zero codeword, layered OMS offset 2 in 8 bits, 20 sweeps"""

    def __init__(self, q, O):
        path = os.path.join(GOLD, matlab_fp.PINS[NR]["qc"])
        self.path = path
        self.code, self.og = q.Code.from_qc(path), O.Graph.from_qc(path)
        assert self.code.layer_order()[2]                                 # natural order: the base rows are the layers, as in the script
        self.N, self.M, self.z = self.code.N, self.code.M, matlab_fp.PINS[NR]["z"]
        var, chk = self.code.edges()
        H = np.zeros((self.M, self.N), np.uint8)
        H[chk, var] = 1
        assert (self.N, self.M) == (1144, 624) and mc_soft_ref.gf2_rank(H[:, self.N - self.M:]) == self.M      # so K = 520 = the script's k
        self.enc = q.Encoder(self.code, "QC")
        self.K, self.pos = self.enc.K, np.asarray(self.enc.info_bits_pos)
        assert self.K == 520 == matlab_fp.PINS[NR]["kb"] * self.z and (self.pos == np.arange(520)).all()
        self.cls = np.zeros(self.N, np.uint8)
        self.cls[:2 * self.z] = q.VN_PUNCTURED
        self.rate = self.K / (self.N - 2 * self.z)
        self.dec = q.Decoder(self.code, self.K, matlab_fp.MAX_ITRS, info_bits_pos=self.pos, rule="OMS", rule_param=matlab_fp.OFFSET, n_frames=20000,
                             schedule="hlayered", enable_syndrome=False, msg_dtype="i8", quant_scale=1.0)
        self.mc = q.MonteCarlo(self.dec, self.enc, vn_class=self.cls, seed=SEED)
        self.mc.set_source("zero")


@pytest.fixture(scope="module")
def nr(q, O):
    return _Nr(q, O)


def test_matlab_experiment_exact_at_1p5_db(q, O, nr):
    """192 frames at 1.5 dB against mc_llr_host -> integer oracle, counter for counter.  The scan on the CPU over the Philox frames [0, 192) of
    SEED gave 73 failed frames of 192 (numpy normal draws: 64), inside the 10 % .. 90 % window (asserted first)."""
    s = nr
    sigma = s.mc.set_awgn(ebno_db=1.5, rate=s.rate)
    assert abs(sigma - 0.8414) < 1e-4
    llr, flip_w = q.mc_llr_host(s.K, s.N, SEED, q.mc_awgn_table(sigma), 0, 192, vn_class=s.cls)
    # the all-zero codeword sends +1 everywhere: the top level (r >= 3, 2.4 sigma) occurs, the bottom one (r < -3, 4.8 sigma) need not
    assert (llr[:, :2 * s.z] == 0).all() and (llr == np.rint(llr)).all() and -32 <= llr.min() < 0 and llr.max() == 31
    r = O.decode(s.og, llr, "OMS", matlab_fp.OFFSET, matlab_fp.MAX_ITRS, "hlayered", enable_syndrome=False, n_threads=8, msg_i8=True, quant_scale=1.0)
    f = verdicts(r, np.zeros((192, s.N), np.uint8), s.pos, mc_ref.unpack(flip_w, s.N), s.cls == 0)
    ctr, hist, failed = tally(f, int((s.cls == 0).sum()), n_ite=matlab_fp.MAX_ITRS)
    print("NR_2_6_52 @ 1.5 dB:", ctr)
    assert 0.1 * 192 <= ctr["frame_errors"] <= 0.9 * 192
    res = s.mc.run(0.1, 0, 192)
    print("NR_2_6_52 @ 1.5 dB:", counters(res))
    assert counters(res) == ctr and res["batches"] == 1
    assert (s.mc.iter_hist() == hist).all() and (s.mc.failed_frames() == failed).all()
    info, cw, _ = s.mc.frames(5, 3, 0.1)                                 # the zero source
    assert not u32(info).any() and not u32(cw).any()


def test_matlab_experiment_published_fer_at_2p35_db(q, nr):
    """20 000 frames at 2.35 dB in one run: the FER inside the project's band around the published 54 / 20 000 (matlab_fp.band: +-4 sigma of
    both estimates plus 20 % for the clamps).  The oracle on the CPU over the same Philox frames gave 57 of 20 000."""
    s = nr
    s.mc.set_awgn(ebno_db=2.35, rate=s.rate)
    res = s.mc.run(0.1, 0, 20000)
    lo, hi = matlab_fp.band(NR, 2.35, 20000)
    print("NR_2_6_52 @ 2.35 dB: %d frame errors of %d (published 54 of 20000), band %g .. %g" % (res["frame_errors"], res["frames"], lo, hi))
    assert res["frames"] == 20000 and res["batches"] == 1
    assert lo <= res["frame_errors"] / 20000.0 <= hi


def test_qldpc_sim_awgn_rows(q, nr):
    s = nr
    args = ["-q", s.path, "-G", "QC", "-r", "OMS", "-p", "2", "-i", "20", "-l", "-n", "-Q", "8", "-c", "1", "-S", str(SEED), "-D", "-z", "-u", str(2 * s.z)]

    def row(extra):
        rows, text = sim_rows(args + extra)
        assert len(rows) == 1, text
        f = rows[0]
        return dict(ep=float(f[0]), fra=int(f[1]), be=int(f[2]), fe=int(f[3]))

    s.mc.set_awgn(ebno_db=1.5, rate=s.rate)
    res = s.mc.run(0.1, 0, 192)
    got = row(["-b", "192", "-f", "192", "-A", "1.5"])
    assert (got["ep"], got["fra"], got["be"], got["fe"]) == (1.5, 192, res["bit_errors"], res["frame_errors"]) and got["fe"] > 0
    assert row(["-b", "192", "-f", "192", "-A", "1.5:3:31"]) == got
    got = row(["-b", "20000", "-f", "20000", "-A", "2.35"])
    lo, hi = matlab_fp.band(NR, 2.35, 20000)
    print("qldpc_sim -D -A 2.35 -z:", got)
    assert got["fra"] == 20000 and lo <= got["fe"] / 20000.0 <= hi
    for refused in ([a for a in args if a != "-D"] + ["-A", "1.5"], args + ["-A", "1.5", "-X", "1.3"], [a for a in args if a != "-D"]):
        p = subprocess.run([SIM] + refused + ["-f", "192", "-b", "192"], capture_output=True, text=True, timeout=60)
        assert p.returncode != 0 and ("-A" in p.stderr or "-u" in p.stderr)


def test_search_with_a_table_equals_the_oracle_row_for_row(q, peg):
    """4 patterns x 16 frames of the 8-bit PEG setup through the AWGN table, 16 of the 504 parity VNs erased per pattern (the class map has no
    pinned VN, so the candidates are given): the rows against numpy pattern -> mc_llr_host -> LLRs with the pattern's VNs at 0 -> oracle, and
    the pattern as a fixed puncture set of run() gives its row again.  Every pattern must fail between 10 % and 90 % of its 16 frames
    (asserted first).  The scan with the oracle on the CPU over patterns 0 .. 3 of SEED (failed frames of 16 per pattern):
          n_punct    0: 10 10 11  7      8: 11 10 12  8     16: 12 12 14 11     24: 13 12 14 13     32: 14 12 15 14     60: 15 14 16 15
    -> 16: the erasures move every row, and no row is full."""
    s = peg
    F, n_pat, n_punct = 16, 4, 16
    cand = np.arange(0, 504, dtype=np.int32)
    cw, llr, _ = s.frames(SIGMA, 0, n_pat * F)
    llr = llr.copy()
    vns = [cand[mc_search_ref.pattern(SEED, p, cand.size, n_punct)] for p in range(n_pat)]
    for p in range(n_pat):
        llr[p * F:(p + 1) * F, vns[p]] = 0.0
    f = verdicts(s.oracle("i8", llr), cw, s.pos, np.zeros_like(cw), s.chan == 0)
    be, ok, it = (f[k].reshape(n_pat, F) for k in ("be", "ok", "it"))
    ref = dict(frames=np.full(n_pat, F), frame_errors=(be > 0).sum(1), bit_errors=be.sum(1), undetected=((be > 0) & ok).sum(1),
               not_converged=(~ok).sum(1), iter_sum=it.sum(1))
    print(ref)
    assert (0.1 * F <= ref["frame_errors"]).all() and (ref["frame_errors"] <= 0.9 * F).all()
    mc = q.MonteCarlo(s.soft_decoder("i8"), s.enc, vn_class=s.chan, seed=SEED, batch=64)
    mc.set_awgn(sigma=SIGMA)
    mc.set_candidates(cand)
    res = mc.search(0.1, n_punct, F, max_patterns=n_pat, stop_at_goal=False)
    assert res["patterns"] == n_pat and res["batches"] == 1 and (res["stats"]["pattern"] == np.arange(n_pat)).all()
    for k in ROW:
        assert (res["stats"][k] == ref[k]).all(), (k, res["stats"][k], ref[k])
    for p in range(n_pat):
        assert (mc.pattern_vns(p, n_punct) == vns[p]).all()
        mc.set_puncture(vns[p])
        r = mc.run(0.1, p * F, F)
        for k in ROW:
            assert int(r[k]) == int(ref[k][p]), (p, k)
    mc.set_puncture([])
    assert counters(mc.run(0.1, 0, 192)) == s.soft_reference("i8", SIGMA, 0, 192)[0]


def test_table_removal_and_refused_tables(q, peg, tables):
    s = peg
    dec = s.soft_decoder("flood")
    fresh = q.MonteCarlo(dec, s.enc, seed=SEED, batch=64)
    bsc = fresh.run(0.26, 0, 64)
    bsc_hist, bsc_failed = fresh.iter_hist(), fresh.failed_frames()
    assert 0 < bsc["frame_errors"] < 64
    mc = q.MonteCarlo(dec, s.enc, seed=SEED, batch=64)
    with pytest.raises(q.QldpcError) as e:
        mc.llr_frames(0, 2)                                               # no table yet
    assert e.value.status == -8
    before = mc.device_bytes
    mc.set_channel(*tables["q256"])
    grown = mc.device_bytes
    assert grown >= before + 64 * s.N * 4
    soft = mc.run(0.26, 0, 64)
    llr = mc.llr_frames(0, 2)[3].cpu().numpy()
    assert counters(soft) != counters(bsc)
    c0, c1, value = tables["awgn64"]
    dec_row = c0.copy()
    dec_row[5] = dec_row[4] - 1
    over = c1.copy()
    over[-1] = 2 ** 32 + 1
    for status, bad in ((-6, (c0[:0], c1[:0], value[:1])), (-6, (np.zeros(256, np.uint64), np.zeros(256, np.uint64), np.zeros(257, np.float32))),
                        (-1, (dec_row, c1, value)), (-1, (c0, over, value))):
        with pytest.raises(q.QldpcError) as e:
            mc.set_channel(*bad)
        assert e.value.status == status
    t, keep = q._mc_channel_arg(c0, c1, value, "test")
    t.reserved[0] = 1
    assert q._L.qldpc_mc_set_channel(mc._h, t) == -1
    assert (mc.llr_frames(0, 2)[3].cpu().numpy().view(np.uint32) == llr.view(np.uint32)).all()      # the previous table is still in force
    assert counters(mc.run(0.26, 0, 64)) == counters(soft)
    mc.set_channel(*tables["awgn64"])
    assert mc.device_bytes == grown and counters(mc.run(0.26, 0, 64)) != counters(soft)
    mc.set_channel(None)                                                  # back to the BSC: the run of a fresh object
    assert counters(mc.run(0.26, 0, 64)) == counters(bsc)
    assert (mc.iter_hist() == bsc_hist).all() and (mc.failed_frames() == bsc_failed).all()
    with pytest.raises(q.QldpcError):
        mc.llr_frames(0, 2)
    with pytest.raises(q.QldpcError):
        mc.set_source("ones")
    with pytest.raises(q.QldpcError):
        mc.set_awgn(sigma=1.0, ebno_db=1.0, rate=0.5)
    mc.set_source("zero")
    info, cw, rx = mc.frames(0, 4, 0.1)
    assert not u32(info).any() and not u32(cw).any() and u32(rx).any()
    mc.set_source("random")
    assert counters(mc.run(0.26, 0, 64)) == counters(bsc)
