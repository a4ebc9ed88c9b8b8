"""GPU suite: the decoder's own state -- what it allocates, what a load clears, what a call out of order answers.

Everything runs on PEGReg504x1008 (N = 1 008, regular: every check has degree 6, every VN degree 3) with n_ite = 5: the edge engine with 4 frames,
the frames engine with 70 (two groups at one frame per lane, the second ragged).  The byte figures are formulas read off qldpc_decoder_create
(the graph arrays, the lists and records of the buckets, the message and per-frame arrays of the configuration) and off the calls that allocate
on first use; they do not come from a run.  "Known wins over erased in either order" for the fp32 LLR array of the frames engine is asserted by
tests/test_blind_gpu.py::test_load_known_equals_the_oracle_on_pinned_llrs; here the edge engine and the coded form of load_bits.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_ITE = 5
F_EDGE, F_FRAMES = 4, 70
ESTATE, EUNSUPPORTED = -8, -7
IDX_PAD, REC_HDR, EDGE_CTL_WORDS = 64, 4, 64      # QK_IDX_PAD, QK_REC_HDR, QE_CTL_WORDS
CN_CAPS = (8, 12, 20, 40)


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def code(q, gold):
    return q.Code.from_alist(os.path.join(gold, "PEGReg504x1008.alist"))


def i32(words):
    return np.ascontiguousarray(words).astype(np.int64).astype(np.uint32).view(np.int32)


def dev_bits(q, torch, bits):
    return torch.from_numpy(i32(q.pack_bits(bits))).cuda()


class Batch:
    """F frames: received bits and one magnitude (the LLR array they stand for), target syndromes, erasure and known / value masks"""

    def __init__(self, q, torch, code, F, seed=5):
        rng = np.random.default_rng(seed)
        N = code.N
        self.F = F
        self.a = rng.integers(0, 2, (F, N)).astype(np.uint8)
        self.b = self.a ^ (rng.random((F, N)) < 0.05).astype(np.uint8)
        self.mag = np.float32(np.log(0.95 / 0.05))
        self.llr = np.where(self.b == 1, -self.mag, self.mag).astype(np.float32)
        self.erase = (rng.random((F, N)) < 0.05).astype(np.uint8)
        self.known = (rng.random((F, N)) < 0.06).astype(np.uint8)
        self.erase[:, :64] |= self.known[:, :64]      # the two overlap
        self.value = self.a.copy()
        self.synd = np.stack([code.syndrome(x)[1] for x in self.a]).astype(np.uint8)
        pin = np.float32(q.CONFIRMED_BIT_LLR)
        self.llr_erased_known = np.where(self.erase != 0, np.float32(0), self.llr).astype(np.float32)
        k = self.known != 0
        self.llr_erased_known[k] = np.where(self.value[k] != 0, -pin, pin)
        self.t_bits, self.t_synd, self.t_erase = dev_bits(q, torch, self.b), dev_bits(q, torch, self.synd), dev_bits(q, torch, self.erase)
        self.t_known, self.t_value = dev_bits(q, torch, self.known), dev_bits(q, torch, self.value)
        self.t_mag = torch.full((F,), float(self.mag), device="cuda")
        self.t_llr = torch.from_numpy(self.llr).cuda()


@pytest.fixture(scope="module")
def batches(q, torch, code):
    return {"edges": Batch(q, torch, code, F_EDGE), "frames": Batch(q, torch, code, F_FRAMES)}


def make(q, code, engine, **kw):
    kw.setdefault("rule", "NMS")
    kw.setdefault("rule_param", 0.75)
    return q.Decoder(code, code.N, N_ITE, n_frames=F_EDGE if engine == "edges" else F_FRAMES, engine=engine, **kw)


def result(dec):
    it, ok = dec.fetch_status()
    return dec.fetch_packed().cpu().numpy(), it.cpu().numpy(), ok.cpu().numpy()


def same(x, y):
    return all((a == b).all() for a, b in zip(x, y))


# ---------------------------------------------------------------- device bytes

def words32(n):
    return (n + 31) // 32


def graph_bytes(c, K):
    """cn_ptr, cn_tr and cn_var (padded), vn_ptr, info_pos, vn_tr (padded), cn_var transposed to [max_dc][M]: ints"""
    return 4 * ((c.M + 1) + 2 * (c.E + IDX_PAD) + (c.N + 1) + K + (c.E + IDX_PAD) + max(1, c.max_cn_degree) * c.M)


def edge_bytes(c, K, F):
    """llr [F][N]; v2c and two chk_to_var buffers [F][E]; sign and hard words [F][W]; unsat [F][n_ite + 2]; done_at [F]; the control words"""
    W = words32(c.N)
    return graph_bytes(c, K) + 4 * (F * c.N + 3 * F * c.E + 2 * F * W + F * (N_ITE + 2) + F + EDGE_CTL_WORDS)


def frame_state_bytes(c, G, V, i8=False, giveup=False, compact=False):
    """sign and hard ballots [G][N][V] (one array with 8-bit messages), unsat and done [G][V], depth and iters [G][FG], the give-up state, the
    counters {active[4], work}, and with compaction on the group counts and offsets"""
    FG = 64 * V
    b = 8 * G * c.N * V * (1 if i8 else 2) + 2 * 8 * G * V + 2 * 4 * G * FG + 4 * 4 + 8
    if giveup:
        b += 4 * 4 * G * FG + 8 * G * V + 8
    if compact:
        b += 4 * G + 4 * (G + 1)
    return b


def flooding_bytes(c, K, F, V, dtype="f32", **state):
    """a list entry per check and per VN (the buckets partition them); the coded form {ybits [G][N][V], fmag and fnch [G][FG], a class byte per VN,
    rounded up to dwords} unless the messages are 8-bit, which keep a quantised LLR array [G][N][64] dwords; v2c and c2v [G][E][FG] cells"""
    FG = 64 * V
    G = (F + FG - 1) // FG
    cell = {"f32": 4, "f16": 2, "i8": 1}[dtype]
    msgs = 4 * ((G * c.E * FG * cell + 3) // 4)
    b = graph_bytes(c, K) + 4 * (c.M + c.N) + 2 * msgs
    if dtype == "i8":
        b += 4 * G * c.N * 64
    else:
        b += 8 * G * c.N * V + 2 * 4 * G * FG + (c.N + 3) // 4 * 4
    return b + frame_state_bytes(c, G, V, i8=dtype == "i8", **state)


def check_degrees(c):
    _, chk = c.edges()
    return np.bincount(chk, minlength=c.M)


def hlayered_bytes(c, K, F, dtype="f32", **state):
    """a list entry per check and, for a check in a register-resident bucket, a record {header, cap VNs}; fp32: posteriors [G][N][64] and
    messages [G][E][64]; 8-bit (four frames to a dword, one group of 256): quantised LLRs, posteriors [G][N][64] and messages [G][E][64] dwords"""
    V = 4 if dtype == "i8" else 1
    FG = 64 * V
    G = (F + FG - 1) // FG
    caps = [next((cap for cap in CN_CAPS if d <= cap), 0) for d in check_degrees(c)]
    b = graph_bytes(c, K) + 4 * c.M + 4 * sum(REC_HDR + cap for cap in caps if cap > 0)
    b += 4 * G * 64 * ((2 if dtype == "i8" else 1) * c.N + c.E)
    return b + frame_state_bytes(c, G, V, i8=dtype == "i8", **state)


def vlayered_bytes(c, K, F):
    """a list entry per VN (the classes partition them), the check of every VN-major slot [E], posteriors [G][N][64] and messages [G][E][64]"""
    G = (F + 63) // 64
    return graph_bytes(c, K) + 4 * c.N + 4 * c.E + 4 * G * 64 * (c.N + c.E) + frame_state_bytes(c, G, 1)


CREATED = [
    ("edges", dict(engine="edges"), lambda c: edge_bytes(c, c.N, F_EDGE)),
    ("flooding-f32", dict(engine="frames"), lambda c: flooding_bytes(c, c.N, F_FRAMES, 1)),
    ("flooding-f16", dict(engine="frames", msg_dtype="f16"), lambda c: flooding_bytes(c, c.N, F_FRAMES, 2, "f16")),
    ("flooding-i8", dict(engine="frames", msg_dtype="i8"), lambda c: flooding_bytes(c, c.N, F_FRAMES, 4, "i8")),
    ("flooding-fixed-nms", dict(engine="frames", enable_syndrome=False), lambda c: flooding_bytes(c, c.N, F_FRAMES, 1)),
    ("hlayered-f32-compact", dict(engine="frames", schedule="hlayered", compact="on"), lambda c: hlayered_bytes(c, c.N, F_FRAMES, compact=True)),
    ("hlayered-i8", dict(engine="frames", schedule="hlayered", msg_dtype="i8"), lambda c: hlayered_bytes(c, c.N, F_FRAMES, "i8")),
    ("vlayered", dict(engine="frames", schedule="vlayered"), lambda c: vlayered_bytes(c, c.N, F_FRAMES)),
    ("flooding-giveup", dict(engine="frames", giveup=2), lambda c: flooding_bytes(c, c.N, F_FRAMES, 1, giveup=True)),
    ("flooding-fixed-spa", dict(engine="frames", enable_syndrome=False, rule="SPA", rule_param=0.0), lambda c: flooding_bytes(c, c.N, F_FRAMES, 1)),
]


@pytest.mark.parametrize("name,kw,expect", CREATED, ids=[c[0] for c in CREATED])
def test_device_bytes_after_creation(q, code, name, kw, expect):
    dec = make(q, code, **kw)
    assert not dec.flood_post      # the code has no IRA chain: no decoder here takes the posterior form, which would add its own arrays
    print(name, dec.device_bytes, expect(code))
    assert dec.device_bytes == expect(code)


def grows(dec, call, by):
    """the first call allocates exactly `by` bytes, the second nothing"""
    for want in (by, 0):
        before = dec.device_bytes
        call()
        print(call.__name__, dec.device_bytes - before, want)
        assert dec.device_bytes - before == want, call.__name__


@pytest.mark.parametrize("engine", ["edges", "frames"])
def test_device_bytes_grow_by_the_lazy_buffers_once(q, torch, code, batches, engine):
    c, bt = code, batches[engine]
    F, W, Wm = bt.F, words32(code.N), words32(code.M)
    G, V, FG = (F_FRAMES + 63) // 64, 1, 64
    dec = make(q, code, engine)
    created = dec.device_bytes
    edges = engine == "edges"

    def load_bits():
        dec.load_bits(bt.t_bits, bt.t_mag)

    def load_syndrome():
        dec.load_syndrome(bt.t_synd)

    def load_erasures():
        dec.load_erasures(bt.t_erase)

    def load_known():
        dec.load_known(bt.t_known, bt.t_value)

    def fetch_post():
        dec.fetch_post()

    def decode_siho():
        dec.decode_siho(bt.llr)

    grows(dec, load_bits, 0)                                         # the frames engine keeps the coded form: no LLR array yet
    grows(dec, load_syndrome, 4 * F * Wm if edges else 8 * G * c.M * V)
    grows(dec, load_erasures, 0 if edges else 8 * G * c.N * V)       # coded form: erasure ballots [G][N][V]
    # the masks [2][max_frames][W]; the frames engine writes the coded frames out as the LLR array [G][N][FG] they stand for
    grows(dec, load_known, 8 * F * W + (0 if edges else 4 * G * c.N * FG))
    dec.run()
    grows(dec, fetch_post, 0 if edges else 4 * G * c.N * FG)         # the edge engine writes into the caller's array
    grows(dec, decode_siho, 4 * F * (c.N + c.N))                     # staging of Y_N and V_K, K = N
    lazy = (4 * F * Wm + 8 * F * W) if edges else 8 * G * V * (c.M + c.N) + 8 * F * W + 2 * 4 * G * c.N * FG
    assert dec.device_bytes == created + lazy + 8 * F * c.N


# ---------------------------------------------------------------- per-batch state

@pytest.mark.parametrize("second", ["llr", "bits"])
@pytest.mark.parametrize("engine", ["edges", "frames"])
def test_the_next_load_clears_the_state_of_the_batch(q, torch, code, batches, engine, second):
    bt = batches[engine]

    def load(dec):
        if second == "llr":
            dec.load_llr(bt.t_llr)
        else:
            dec.load_bits(bt.t_bits, bt.t_mag)

    fresh = make(q, code, engine)
    load(fresh)
    fresh.run()
    want = result(fresh)
    dec = make(q, code, engine)
    dec.load_bits(bt.t_bits, bt.t_mag)
    dec.load_erasures(bt.t_erase)
    dec.load_known(bt.t_known, bt.t_value)
    dec.load_syndrome(bt.t_synd)
    dec.run()
    assert not same(result(dec), want)      # the erasures, known bits and target syndromes were part of that decode
    load(dec)
    dec.run()
    assert same(result(dec), want)
    assert dec.last_run_iterations == fresh.last_run_iterations


# ---------------------------------------------------------------- calls out of order

def status_of(q, call):
    with pytest.raises(q.QldpcError) as e:
        call()
    return e.value.status


@pytest.mark.parametrize("engine", ["edges", "frames"])
def test_calls_out_of_order_are_state_errors(q, torch, code, batches, engine):
    bt = batches[engine]
    dec = make(q, code, engine)
    side_loads = [lambda n: dec.load_syndrome(bt.t_synd[:n]), lambda n: dec.load_erasures(bt.t_erase[:n]), lambda n: dec.load_known(bt.t_known[:n], bt.t_value[:n])]
    for f in side_loads:
        assert status_of(q, lambda: f(bt.F)) == ESTATE                  # nothing loaded
    assert status_of(q, dec.run) == ESTATE
    dec.load_llr(bt.t_llr)
    for f in side_loads:
        assert status_of(q, lambda: f(bt.F - 1)) == ESTATE              # another frame count than the loaded one
    fetches = [dec.fetch_packed, dec.fetch_info, dec.fetch_status, dec.fetch_post, lambda: dec.fetch_weakest(4)]
    for f in fetches:
        assert status_of(q, f) == ESTATE                                # no run yet
    dec.run()
    dec.load_llr(bt.t_llr)
    for f in fetches:
        assert status_of(q, f) == ESTATE                                # a load after the run: its results are gone
    dec.run()
    if engine == "edges":
        assert status_of(q, lambda: dec.fetch_weakest(4)) == EUNSUPPORTED
    else:
        dec.fetch_weakest(4)
    result(dec)


# ---------------------------------------------------------------- known wins over erased

@pytest.mark.parametrize("engine,form", [("edges", "llr"), ("edges", "bits"), ("frames", "bits")])
def test_known_wins_over_erased_in_either_order(q, torch, code, batches, engine, form):
    """both orders of the two loads decode the LLR array with 0 written where erased and then +-23.03 where known (frames engine: from the coded
    form of load_bits; its fp32 array form is covered by tests/test_blind_gpu.py)"""
    bt = batches[engine]
    ref = make(q, code, engine)
    ref.load_llr(torch.from_numpy(bt.llr_erased_known).cuda())
    ref.load_syndrome(bt.t_synd)
    ref.run()
    want = result(ref)
    plain = make(q, code, engine)
    plain.load_llr(bt.t_llr)
    plain.load_syndrome(bt.t_synd)
    plain.run()
    assert not same(result(plain), want)
    dec = make(q, code, engine)
    for known_first in (True, False):
        if form == "llr":
            dec.load_llr(bt.t_llr)
        else:
            dec.load_bits(bt.t_bits, bt.t_mag)
        if known_first:
            dec.load_known(bt.t_known, bt.t_value)
        dec.load_erasures(bt.t_erase)
        if not known_first:
            dec.load_known(bt.t_known, bt.t_value)
        dec.load_syndrome(bt.t_synd)
        dec.run()
        assert same(result(dec), want), known_first
