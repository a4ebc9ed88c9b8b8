"""What the GPU tests of the Monte-Carlo loop (tests/test_mc*_gpu.py) share, stated once: the two test codes with their CPU oracle graphs,
the per-frame reference host mirror -> encoder -> LLRs -> CPU oracle -> compare, the tallies of qldpc_mc_run over it, the comparison of
point / stratum rows, and the call of host/qldpc_sim.  Not a test module and not a conftest; only _Setup.decoder touches the device."""
import os
import subprocess

import numpy as np
import pytest

import mc_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIM = os.path.join(ROOT, "qcrypto-ldpc_amd", "host", "qldpc_sim")
SEED = 0x0123456789ABCDEF
N_ITE = 20
# chosen by the scan recorded in the docstring of test_mc_gpu.test_run_equals_the_oracle_counter_for_counter
QBER = {"peg": 0.26, "ira": 0.03}          # every class fails between 10 % and 90 % of 192 frames
KINDS = {"flood": dict(schedule="flooding"), "hlay": dict(schedule="hlayered"), "i8": dict(schedule="flooding", msg_dtype="i8")}
COUNTERS = ("frames", "bit_errors", "frame_errors", "undetected", "not_converged", "iter_sum", "iter_max", "channel_flips", "channel_bits")
PATTERN_ROW = ("pattern", "frames", "frame_errors", "bit_errors", "undetected", "not_converged", "iter_sum")      # MC_PATTERN_STAT, in its order
RUN_STAGES = ("source", "encode", "channel", "load", "decode", "monitor")      # every stage of run, sweep and strata that launches a kernel in every call


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def counters(res):
    return {k: int(res[k]) for k in COUNTERS}


def stage_times(res, launched=RUN_STAGES):
    """every stage time of a result is finite and not negative, and positive where the stage launched a kernel in that call"""
    for k, v in res.items():
        if k.endswith("_ms"):
            assert np.isfinite(v) and v >= 0, (k, v)
    for k in launched:
        assert res[k + "_ms"] > 0, (k, res)


class _Setup:
    def __init__(self, q, O, name):
        self.name = name
        self.code = q.Code.from_alist(os.path.join(ROOT, "tests", "golden", "PEGReg504x1008.alist")) if name == "peg" else q.Code.ira(2000, 1590)
        self.enc = q.Encoder(self.code, "IDENTITY" if name == "peg" else "IRA")
        self.K, self.N, self.pos = self.enc.K, self.code.N, self.enc.info_bits_pos
        assert (self.K, self.N) == ((504, 1008) if name == "peg" else (1590, 2000))
        self.cls = mc_ref.classes(self.K, self.N, self.pos)
        var, chk = self.code.edges()
        self.og = O.Graph.from_edges(self.N, self.code.M, var, chk)
        order, _, _ = self.code.layer_order()                        # the layered oracle visits the checks in the code's layer order
        inv = np.empty(self.code.M, np.int32)
        inv[order] = np.arange(self.code.M, dtype=np.int32)
        newc = inv[chk]
        idx = np.argsort(newc, kind="stable")
        self.ogl = O.Graph.from_edges(self.N, self.code.M, var[idx], newc[idx])
        self._ref, self._dec, self.q, self.O = {}, {}, q, O

    def decoder(self, kind, n_frames=192):
        key = (kind, n_frames)
        if key not in self._dec:
            self._dec[key] = self.q.Decoder(self.code, self.K, N_ITE, info_bits_pos=self.pos, rule="NMS", rule_param=0.75, n_frames=n_frames, **KINDS[kind])
        return self._dec[key]

    def codewords(self, info_words):
        info = mc_ref.unpack(info_words, self.K)
        cw = self.enc.encode(info)
        assert (cw[:, self.pos] == info).all()
        for x in cw[:3]:
            assert self.og.syndrome(x)[0] == 0
        return cw

    def reference(self, kind, qber, first, n):
        """counters, histogram and failed frames of frames [first, first + n) of the BSC at qber, by frames_reference"""
        return tally(frames_reference(self, kind, ("bsc", qber), first, n), int((self.cls == 0).sum()), first)


_SETUPS = {}


@pytest.fixture(scope="session")
def setups(q, O):
    """name ("peg" / "ira") -> its _Setup.  One per process, whichever module asks: its references are pure functions of their arguments, kept
    in _Setup._ref under keys that start with the frame source (frames_reference) or the mode's name, so no two modes share one."""
    def get(name):
        if name not in _SETUPS:
            _SETUPS[name] = _Setup(q, O, name)
        return _SETUPS[name]
    return get


def oracle(s, kind, llr, quant_scale=8.0):
    """the CPU oracle's decode of the LLR rows as the decoder of that kind runs it"""
    if kind == "hlay":
        return s.O.decode(s.ogl, llr, "NMS", 0.75, N_ITE, "hlayered", n_threads=8)
    extra = dict(msg_i8=True, quant_scale=quant_scale) if kind == "i8" else {}
    assert kind in ("flood", "i8")
    return s.O.decode(s.og, llr, "NMS", 0.75, N_ITE, n_threads=8, **extra)


def bsc_llrs(q, y, cls, qber, erased=()):
    """LLR rows of received words y: +-bsc_llr(qber), the pinned class (1) at +-CONFIRMED_BIT_LLR, the erased VNs at 0"""
    mag, pin = np.float32(q.bsc_llr(qber)), np.float32(q.CONFIRMED_BIT_LLR)
    llr = np.where(y == 1, -mag, mag).astype(np.float32)
    llr[:, cls == 1] = np.where(y[:, cls == 1] == 1, -pin, pin)
    llr[:, list(erased)] = 0.0
    return llr


def verdicts(r, cw, pos, flips, chan):
    """an oracle result per frame, read-only: info-bit errors `be`, syndrome verdict `ok`, iterations `it`, flips among the channel VNs `fl`"""
    out = dict(be=(r["hard"][:, pos] != cw[:, pos]).sum(1), ok=r["synd_ok"] != 0, it=r["iters"], fl=flips[:, chan].sum(1))
    for a in out.values():
        a.setflags(write=False)
    return out


def frames_reference(s, kind, source, first, n, erased=(), block=0):
    """verdicts of frames [first, first + n) by numpy: the host mirror's frames of `source` -- ("bsc", qber), or ("weight", w, design_qber) for
    exactly w flips -> encoder -> LLRs of that QBER, the erased VNs at 0 -> oracle -> compare.  erased: VNs, or with `block` one list of VNs
    per `block` consecutive frames.  Computed once per argument set and left unchanged."""
    erased = tuple(tuple(int(v) for v in e) for e in erased) if block else tuple(int(v) for v in erased)
    key = (source, kind, first, n, erased, block)
    if key in s._ref:
        return s._ref[key]
    host = s.q.mc_frames_host if source[0] == "bsc" else s.q.mc_weight_frames_host
    assert source[0] in ("bsc", "weight") and len(source) == (2 if source[0] == "bsc" else 3)
    info_w, flip_w = host(s.K, s.N, SEED, source[1], first, n, info_bits_pos=s.pos)
    cw = s.codewords(info_w)
    flips = mc_ref.unpack(flip_w, s.N)
    llr = bsc_llrs(s.q, cw ^ flips, s.cls, source[-1], () if block else erased)
    for i, vns in enumerate(erased if block else ()):
        llr[i * block:(i + 1) * block, list(vns)] = 0.0
    out = verdicts(oracle(s, kind, llr), cw, s.pos, flips, s.cls == 0)
    assert int(out["fl"].sum()) == mc_ref.popcount(flip_w)             # parity_ber = 0: every flip is a channel flip
    s._ref[key] = out
    return out


def tally(f, n_chan, first=0, n=None, n_ite=N_ITE):
    """counters, iteration histogram and failed-frame indices of the first n (None = all) of the frames of `verdicts`, the first of which is
    frame `first`, as qldpc_mc_run defines them"""
    n = f["be"].size if n is None else n
    be, ok, it = f["be"][:n], f["ok"][:n], f["it"][:n]
    ctr = dict(frames=n, bit_errors=int(be.sum()), frame_errors=int((be > 0).sum()), undetected=int(((be > 0) & ok).sum()), not_converged=int((~ok).sum()),
               iter_sum=int(it.sum()), iter_max=int(it.max()) if n else 0, channel_flips=int(f["fl"][:n].sum()), channel_bits=n * n_chan)
    return ctr, np.bincount(it, minlength=n_ite + 1).astype(np.uint64), (first + np.nonzero(be > 0)[0]).astype(np.uint64)


def row_of(s, f, n):
    """the counter row and the histogram of the first n frames of a frames_reference"""
    return tally(f, int((s.cls == 0).sum()), n=n)[:2]


def same_rows(res, key, hist, sch, rows, extra=None):
    """the rows res[key] ("points" of a sweep, "strata" of a strata run) and their histograms are `rows` = [(counter row, histogram)], and with
    a schedule of mc_sweep_ref also its rounds and closing reasons; extra(rows of the result) holds what only that mode asserts"""
    st = res[key]
    assert st.shape == (len(rows),)
    for i, (row, h) in enumerate(rows):
        assert {k: int(st[k][i]) for k in COUNTERS} == row, (i, st[i], row)
        assert (hist[i] == h).all() and int(hist[i].sum()) == row["frames"], i
    if extra is not None:
        extra(st)
    if sch is not None:
        assert (st["last_round"] == sch["last_round"]).all() and (st["closed_by"] == sch["closed_by"]).all(), (st, sch)
        assert res["rounds"] == res["batches"] == sch["rounds"] and res["frames"] == int(sch["frames"].sum())
    assert res["decode_ms"] > 0 and res["total_ms"] > 0
    stage_times(res)


def table_rows(text):
    """the result rows of qldpc_sim's output, each split into its stripped fields"""
    return [[x.strip() for x in l.split("|")] for l in text.splitlines() if not l.startswith("#") and "|" in l]


def sim_rows(args, timeout=300):
    """run host/qldpc_sim (built first where it is missing) -> (its result rows, the whole of stdout)"""
    if not os.path.exists(SIM):
        subprocess.check_call(["make", "-C", os.path.dirname(SIM)])
    p = subprocess.run([SIM] + list(args), capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stdout + p.stderr
    return table_rows(p.stdout), p.stdout
