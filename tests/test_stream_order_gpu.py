"""GPU suite (-m gpu): stream order.  Every context of the library is put on a side stream that the null stream does not wait for, behind a delay
kernel, while the device inputs hold a decoy; what it returns must be the independent reference of the TRUE inputs, bit for bit, in the outputs and
in their clones.  The method, what it catches and the conditions that make it a detector are in tests/stream_order.py.

References: the CPU oracle (min-sum family), tests/vlayered_ref.py, tests/giveup_ref.py, tests/polar_ref.py, tests/polar_ssc_ref.py,
tests/polar_tally_ref.py, tests/polar_list_ref.py, tests/qber_ref.py and tests/qber_merge_ref.py, the numpy GF(2) product (encoder, syndrome_of), the
host mirrors of the weakest select and of the guessing rounds, tests/recon_guess_ref.py and tests/recon_tag_ref.py.  Never a null-stream run of the
library.  Only rules that the other suites hold bit for bit appear (MS, OMS, NMS; polar int8 and float), so there is no tolerance anywhere.

Frames: a decoder's frame f is easy (it converges) in the true inputs and hopeless in the decoy, or the other way round, alternating with f, so that
hard words, success flags, iteration counts, posteriors and give-up records all differ in every frame.  Outputs that do not depend on the inputs
(the iteration count of a fixed-iteration run, the pick of a list decoder without a CRC) are compared as well but are no part of that condition.
Compaction and the give-up rule exist only in the early-exit run and the posterior form only in the fixed one; every other path runs both ways.
"""
import os
from types import SimpleNamespace

import numpy as np
import pytest

import giveup_ref
import polar_list_ref as LR
import polar_ref as PR
import polar_ssc_ref
import polar_tally_ref
import qber_merge_ref
import qber_ref
import recon_guess_ref
import recon_tag_ref
import vlayered_ref
from stream_order import Chain, Delay, differ_in_every_frame, same_bits

pytestmark = pytest.mark.gpu

PIN = np.float32(23.025850929840455)
LO, HI = 0.025, 0.13            # BSC crossovers of PEGReg504x1008: every rule here decodes the first within 8 iterations and never the second
N_FIXED, N_EARLY = 8, 30


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def delay(torch):
    return Delay(torch)


@pytest.fixture(scope="module")
def sides(torch):
    """two side streams; torch's streams are non-blocking: the null stream does not wait for them (the controls below show it)"""
    return torch.cuda.Stream(), torch.cuda.Stream()


def u32(words):
    return np.ascontiguousarray(words).astype(np.int64).astype(np.uint32)


def dev(torch, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def layer_graph(O, code, og):
    """the oracle's graph with the checks in the code's layer order (what the layered sweep visits), and that order"""
    order, _, _ = code.layer_order()
    var, chk = og.edges()
    inv = np.empty(code.M, np.int32)
    inv[order] = np.arange(code.M, dtype=np.int32)
    newc = inv[chk]
    idx = np.argsort(newc, kind="stable")
    return O.Graph.from_edges(code.N, code.M, var[idx], newc[idx]), order


def setup_of(q, O, code, og, pos):
    """a code, the oracle's graphs of it and the positions fetch_info returns"""
    ogl, order = layer_graph(O, code, og)
    vorder, vptr, _ = code.vlayer_order()
    return SimpleNamespace(code=code, og=og, ogl=ogl, order=order, ex=og.export(), vorder=vorder, vptr=vptr, N=code.N, M=code.M, pos=np.asarray(pos, np.int32))


@pytest.fixture(scope="module")
def peg(q, O, gold):
    p = os.path.join(gold, "PEGReg504x1008.alist")
    return setup_of(q, O, q.Code.from_alist(p), O.Graph.from_alist(p), np.arange(504, 1008))


@pytest.fixture(scope="module")
def ira(q, O):
    """the rate-0.5 code of tests/test_flood_post_gpu.py: its fixed-iteration flooding run takes the posterior form"""
    c = q.Code.ira(2048, 1024, 0.125, 11, 3, 7)
    var, chk = c.edges()
    return setup_of(q, O, c, O.Graph.from_edges(c.N, c.M, var, chk), np.arange(1024))


# ---------------------------------------------------------------- decoder frames

def frames_of(q, s, F, seed, phase, lo=LO, hi=HI):
    """F frames of set-up s in the reconciliation form: Alice's word x and its syndrome, Bob's word y = x through a BSC whose crossover is `lo` in the
    frames f with f % 2 == phase and `hi` in the others, one |LLR| per frame, the classes of the VNs (shared), a shortening length per frame, per-frame
    erasures and known bits"""
    rng = np.random.default_rng([seed, F, s.N])
    N = s.N
    p = np.where(np.arange(F) % 2 == phase, lo, hi)
    x = rng.integers(0, 2, (F, N)).astype(np.uint8)
    b = SimpleNamespace(F=F, x=x, p=p, synd=np.stack([s.og.syndrome(r)[1] for r in x]).astype(np.uint8))
    b.mag = np.array([q.bsc_llr(float(v)) for v in p], np.float32)
    b.nch = rng.integers(N - 48, N + 1, F).astype(np.int32)
    b.erase = (rng.random((F, N)) < 0.02).astype(np.uint8)
    b.known = (rng.random((F, N)) < 0.03).astype(np.uint8)
    b.value = x.copy()
    b.flips = (rng.random((F, N)) < p[:, None]).astype(np.uint8)
    return b


CLS_SEED = 77


def classes_of(N):
    """the VN classes of a code, the same for the true inputs and the decoy: 4 % pinned, 3 % punctured"""
    rng = np.random.default_rng([CLS_SEED, N])
    cls = np.zeros(N, np.uint8)
    cls[rng.random(N) < 0.04] = 1
    cls[(rng.random(N) < 0.03) & (cls == 0)] = 2
    return cls


def loaded(b, loads, N):
    """what the loads named in `loads` bring to the decoder -> (Bob's bits as loaded, the LLR array they stand for).  The rule of the coded form is that of
    tests/test_flood_post_gpu.py::coded_case: |LLR| is the frame's for a channel VN below its shortening length, the pin for a shortened or pinned VN, 0
    for a punctured or erased one, the sign is the bit's; a known bit is the pin with its value's sign and wins"""
    cls = classes_of(N) if "cls" in loads else np.zeros(N, np.uint8)
    nch = b.nch if "nch" in loads else np.full(b.F, N, np.int32)
    exact = (cls[None, :] == 1) | (np.arange(N)[None, :] >= nch[:, None])
    y = np.where(exact, b.x, b.x ^ b.flips).astype(np.uint8)
    m = np.where(cls[None, :] == 2, np.float32(0), np.where(exact, PIN, b.mag[:, None])).astype(np.float32)
    if "erase" in loads:
        m[b.erase == 1] = 0.0
    llr = np.where(y == 1, -m, m).astype(np.float32)
    if "known" in loads:
        k = b.known == 1
        llr[k] = np.where(b.value[k] == 1, -PIN, PIN)
    return y, llr


# name -> what a decoder of that run path is made with, what is loaded and what is fetched.  Posteriors are fetched where they are exact: after a fixed
# run, and after an early exit with frozen messages (asked for in the early-exit decoder only); "hlayered" keeps the compressed check state
PATHS = {
    "flood_f32": dict(kw=dict(freeze_messages=True), rule=("NMS", 0.75), loads=("bits", "cls", "nch", "erase", "known", "synd"),
                      fetch=("packed", "info", "status", "post", "weakest")),
    "flood_f16": dict(kw=dict(msg_dtype="f16"), rule=("NMS", 0.75), loads=("bits", "synd"), fetch=("packed", "info", "status")),
    "flood_i8": dict(kw=dict(msg_dtype="i8"), rule=("NMS", 0.8125), loads=("bits", "cls", "synd"), fetch=("packed", "info", "status")),
    "hlayered": dict(kw=dict(schedule="hlayered", layer_chain="off"), rule=("OMS", 0.35), loads=("llr", "synd"), fetch=("packed", "status", "post_if_fixed")),
    # the one-launch sweep reads its fault word back at the end of every run, a fixed one too: the run waits on the host
    "hlayered_chain": dict(kw=dict(schedule="hlayered", layer_chain="on"), rule=("NMS", 0.75), loads=("llr", "synd"), fetch=("packed", "info", "status"),
                           host_waits=True),
    "vlayered": dict(kw=dict(schedule="vlayered", freeze_messages=True), rule=("NMS", 0.75), loads=("llr", "synd"), fetch=("packed", "status", "post")),
    "posterior": dict(kw=dict(), rule=("MS", 0.0), loads=("bits", "cls", "nch", "erase", "synd"), fetch=("packed", "status", "post"), code="ira",
                      modes=("fixed",), lo=0.008, hi=0.16),
    "compact": dict(kw=dict(compact="on"), rule=("NMS", 0.75), loads=("bits", "synd"), fetch=("packed", "info", "status"), F=257, modes=("early",)),
    # patience 4 at a crossover of 0.2: of 3 / 4 / 6 and 0.13 / 0.16 / 0.2 / 0.25 the pairs (4, 0.16 and above) give every hopeless frame of the reference up and none
    # of the easy ones
    "giveup": dict(kw=dict(giveup=4), rule=("NMS", 0.75), loads=("llr", "synd"), fetch=("packed", "status", "giveup"), modes=("early",), hi=0.2),
    "edges": dict(kw=dict(engine="edges"), rule=("NMS", 0.75), loads=("bits", "cls", "nch", "erase", "known", "synd"), fetch=("packed", "info", "status", "post")),
}
WEAKEST_D = 24


def reference(q, O, s, p, llr, synd, early):
    """the outputs of run path p on the LLR rows `llr` with target syndromes `synd` -> name -> array, as the fetches return them"""
    rule, param = p["rule"]
    kw = p["kw"]
    sched = kw.get("schedule", "flooding")
    n_ite = N_EARLY if early else N_FIXED
    if "giveup" in kw:
        assert early and rule == "NMS" and param == 0.75 and n_ite == giveup_ref.N_ITE
        e = giveup_ref.expected(giveup_ref.trajectory(q, O, "flood", llr=llr, target=synd.astype(np.int32), graphs_of=(s.og, s.ogl, s.order)), kw["giveup"])
        r = dict(hard=e["hard"], iters=e["iters"], synd_ok=e["ok"], gave=e["gave"], last=e["last"], best=e["best"])
    elif sched == "vlayered":
        r = vlayered_ref.decode(s.ex, llr, rule, param, n_ite, "vlayered", order=s.vorder, class_ptr=s.vptr, enable_syndrome=early, target=synd)
    else:
        layered = sched == "hlayered"
        r = O.decode(s.ogl if layered else s.og, llr, rule, param, n_ite, sched, early, 1, n_threads=8, msg_fp16=kw.get("msg_dtype") == "f16",
                     msg_i8=kw.get("msg_dtype") == "i8", target=np.ascontiguousarray(synd[:, s.order]) if layered else synd)
    out = {}
    for f in fetches(p, early):
        if f == "packed":
            out["packed"] = u32(q.pack_bits(r["hard"]))
        elif f == "info":
            out["info"] = np.ascontiguousarray(r["hard"][:, s.pos]).astype(np.int32)
        elif f == "status":
            out["iters"], out["ok"] = np.asarray(r["iters"], np.int32), np.asarray(r["synd_ok"], np.int32)
        elif f == "post":
            out["post"] = np.asarray(r["post"], np.float32)
        elif f == "weakest":
            out["weakest"] = np.stack([q.weakest_host(row, WEAKEST_D)[0] for row in r["post"]]).astype(np.uint32)
        elif f == "giveup":
            out.update(gave=r["gave"], last=r["last"], best=r["best"])
    return out


def fetches(p, early):
    return tuple("post" if f == "post_if_fixed" else f for f in p["fetch"] if not (early and f == "post_if_fixed"))


class DecoderCase:
    """a run path at one frame count, fixed or early exit: the true inputs, the decoy, and the references of both"""

    def __init__(self, q, O, s, name, early, F=None, seed=1):
        p = self.p = PATHS[name]
        self.s, self.name, self.early = s, name, early
        self.F = F or p.get("F", 65)
        self.what = "%s %s F=%d" % (name, "early exit" if early else "fixed", self.F)
        lo, hi = p.get("lo", LO), p.get("hi", HI)
        self.true, self.decoy = frames_of(q, s, self.F, seed, 0, lo, hi), frames_of(q, s, self.F, seed + 100, 1, lo, hi)
        self.y, self.llr, self.ref = {}, {}, {}
        for k, b in (("true", self.true), ("decoy", self.decoy)):
            self.y[k], self.llr[k] = loaded(b, p["loads"], s.N)
            self.ref[k] = reference(q, O, s, p, self.llr[k], b.synd, early)
        constant = () if early else ("iters",)
        differ_in_every_frame(*({k: v for k, v in self.ref[w].items() if k not in constant} for w in ("true", "decoy")), self.what)
        # what syndrome_of must give for Bob's words as loaded: the plain GF(2) product
        var, chk = s.og.edges()
        H = np.zeros((s.M, s.N), np.uint8)
        H[chk, var] = 1
        self.synd_of = {k: u32(q.pack_bits((self.y[k].astype(np.int64) @ H.T.astype(np.int64)) & 1)) for k in ("true", "decoy")}

    def decoder(self, q):
        s, (rule, param) = self.s, self.p["rule"]
        kw = dict(self.p["kw"])
        kw.setdefault("engine", "frames")
        if not self.early:
            kw.pop("freeze_messages", None)
        return q.Decoder(s.code, len(s.pos), N_EARLY if self.early else N_FIXED, info_bits_pos=s.pos, rule=rule, rule_param=param, enable_syndrome=self.early,
                         n_frames=self.F, **kw)

    def inputs(self, torch, ch, q):
        """the device tensors of the loads: each holds the decoy now"""
        loads, t, d = self.p["loads"], self.true, self.decoy
        both = lambda f: ch.input(f("true"), f("decoy"))
        x = dict(cls=dev(torch, classes_of(self.s.N)) if "cls" in loads else None, nch=None)
        if "llr" in loads:
            x["llr"] = both(lambda k: self.llr[k])
        else:
            x["bits"] = both(lambda k: u32(q.pack_bits(self.y[k])))
            x["mag"] = ch.input(t.mag, d.mag)
        if "nch" in loads:
            x["nch"] = ch.input(t.nch, d.nch)
        for name in ("erase", "known", "value", "synd"):
            if name in loads or (name == "value" and "known" in loads):
                x[name] = ch.input(u32(q.pack_bits(getattr(t, name))), u32(q.pack_bits(getattr(d, name))))
        return x

    def load(self, dec, x):
        loads = self.p["loads"]
        if "llr" in loads:
            dec.load_llr(x["llr"])
        else:
            dec.load_bits(x["bits"], x["mag"], x["cls"], x["nch"])
        if "erase" in loads:
            dec.load_erasures(x["erase"])
        if "known" in loads:
            dec.load_known(x["known"], x["value"])
        if "synd" in loads:
            dec.load_syndrome(x["synd"])

    def fetch(self, dec, ch, tag=""):
        for f in fetches(self.p, self.early):
            if f == "packed":
                ch.keep(tag + "packed", dec.fetch_packed())
            elif f == "info":
                ch.keep(tag + "info", dec.fetch_info())
            elif f == "status":
                it, ok = dec.fetch_status()
                ch.keep(tag + "iters", it), ch.keep(tag + "ok", ok)
            elif f == "post":
                ch.keep(tag + "post", dec.fetch_post())
            elif f == "weakest":
                ch.keep(tag + "weakest", dec.fetch_weakest(WEAKEST_D))
            elif f == "giveup":
                for k, t in zip(("gave", "last", "best"), dec.fetch_giveup()):
                    ch.keep(tag + k, t)

    def expect(self, which, tag=""):
        return {tag + k: v for k, v in self.ref[which].items()}


_CASES = {}


def decoder_case(q, O, s, name, early, F=None, seed=1):
    key = (name, early, F, seed)
    if key not in _CASES:
        _CASES[key] = DecoderCase(q, O, s, name, early, F, seed)
    return _CASES[key]


def run_decoder_chain(q, torch, delay, side, case, dec, syndrome_of=False):
    """the decoder driven once on the decoy on the null stream, then put on `side`: a delay in front of the loads, of the run and of the fetches"""
    ch = Chain(torch, delay, side, case.what, host_waits=case.early or case.p.get("host_waits", False))
    x = case.inputs(torch, ch, q)
    case.load(dec, x)
    dec.run()
    with ch:
        dec.set_stream(side)
        ch.stage()
        case.load(dec, x)
        if syndrome_of and "bits" in x:
            ch.keep("syndrome_of", dec.syndrome_of(x["bits"]))
        ch.stage()
        dec.run()
        ch.stage()
        case.fetch(dec, ch)
    want = case.expect("true")
    if "syndrome_of" in ch.out:
        want["syndrome_of"] = case.synd_of["true"]
    ch.check_all(want)
    return ch


MODES = [(name, mode) for name, p in PATHS.items() if name != "edges" for mode in p.get("modes", ("fixed", "early"))]


@pytest.mark.parametrize("name,mode", MODES, ids=["%s-%s" % m for m in MODES])
def test_decoder_on_a_side_stream(q, O, torch, delay, sides, peg, ira, name, mode):
    s = ira if PATHS[name].get("code") == "ira" else peg
    case = decoder_case(q, O, s, name, mode == "early")
    dec = case.decoder(q)
    if name == "posterior":
        assert dec.flood_post
    run_decoder_chain(q, torch, delay, sides[0], case, dec, syndrome_of=True)
    if name == "compact":
        assert dec.last_run_stats()["compactions"] >= 1


# ---------------------------------------------------------------- the edge engine

@pytest.mark.parametrize("mode", ["fixed", "early"])
@pytest.mark.parametrize("how", ["launches", "graphs", "one_launch"])
def test_edge_engine_on_a_side_stream(q, O, torch, delay, sides, peg, monkeypatch, how, mode):
    """5 frames, then 3 on the same decoder: a launch per pass, the chunks replayed as graphs (the first call of a frame count captures them on the
    engine's private stream, the second frame count rebuilds them) and the whole decode as one launch, which reads its verdict back and so waits"""
    if how == "graphs":
        monkeypatch.setenv("QLDPC_GRAPH", "1")
    if how == "one_launch":
        monkeypatch.setenv("QLDPC_EDGE_PERSIST", "1")
    first = decoder_case(q, O, peg, "edges", mode == "early", 5, seed=3)
    dec = first.decoder(q)
    for case in (first, decoder_case(q, O, peg, "edges", mode == "early", 3, seed=4)):
        ch = Chain(torch, delay, sides[0], "%s %s" % (how, case.what), host_waits=mode == "early" or how == "one_launch")
        x = case.inputs(torch, ch, q)
        if how != "graphs" or case is not first:      # graphs: the first call on the side stream is the one that captures
            case.load(dec, x)
            dec.run()
        else:
            case.load(dec, x)                         # the decoy's LLR rows are the decoder's all the same
        with ch:
            dec.set_stream(sides[0])
            ch.stage()
            case.load(dec, x)
            ch.stage()
            dec.run()
            ch.stage()
            case.fetch(dec, ch)
        ch.check_all(case.expect("true"))
        dec.set_stream(None)


# ---------------------------------------------------------------- gangs

def gang_members(q, O, peg, early):
    """two horizontal-layered members of one gang (equal iteration counts and syndrome settings), 65 and 33 frames"""
    a = decoder_case(q, O, peg, "hlayered", early, 65, seed=11)
    b = decoder_case(q, O, peg, "hlayered", early, 33, seed=12)
    return [a, b], [a.decoder(q), b.decoder(q)]


@pytest.mark.parametrize("mode", ["fixed", "early"])
def test_gang_on_a_side_stream(q, O, torch, delay, sides, peg, mode):
    cases, decs = gang_members(q, O, peg, mode == "early")
    gang = q.DecoderGang(decs)
    ch = Chain(torch, delay, sides[0], "gang of two, %s" % mode, host_waits=mode == "early")
    xs = [c.inputs(torch, ch, q) for c in cases]
    for c, d, x in zip(cases, decs, xs):
        c.load(d, x)
    gang.run()
    with ch:
        gang.set_stream(sides[0])
        ch.stage()
        for c, d, x in zip(cases, decs, xs):
            c.load(d, x)
        ch.stage()
        gang.run()
        ch.stage()
        for i, (c, d) in enumerate(zip(cases, decs)):
            c.fetch(d, ch, "m%d " % i)
    want = {}
    for i, c in enumerate(cases):
        want.update(c.expect("true", "m%d " % i))
    ch.check_all(want)


def test_gang_takes_a_member_left_on_another_stream(q, O, torch, delay, sides, peg):
    """the gang is on A; member 1 has been moved to B and is loaded there behind two delays, member 0 on A behind one.  The run takes member 1 back:
    what it has queued on B comes first.  A alone is waited for before the results are read"""
    A, B = sides
    cases, decs = gang_members(q, O, peg, False)
    gang = q.DecoderGang(decs)
    on_b = Chain(torch, delay, B, "a member's loads on its own stream", host_waits=True)      # the wait for A falls inside its block
    on_a = Chain(torch, delay, A, "gang takes a member from another stream", behind=on_b)
    xa, xb = cases[0].inputs(torch, on_a, q), cases[1].inputs(torch, on_b, q)
    for c, d, x in zip(cases, decs, (xa, xb)):
        c.load(d, x)
    gang.run()
    gang.set_stream(A)
    decs[1].set_stream(B)
    with on_b:
        delay.queue()
        on_b.stage()
        cases[1].load(decs[1], xb)
        on_b.issued()
        with on_a:
            on_a.stage()
            cases[0].load(decs[0], xa)
            gang.run()
            for i, (c, d) in enumerate(zip(cases, decs)):
                c.fetch(d, on_a, "m%d " % i)
    assert on_b.issue_ms < delay.ms
    want = {}
    for i, c in enumerate(cases):
        want.update(c.expect("true", "m%d " % i))
    on_a.check_all(want)


# ---------------------------------------------------------------- polar

def polar_inputs(n, messages, seed, F=65):
    rng = np.random.default_rng([seed, n, messages == "i8"])
    N = 1 << n
    llr = PR.i8_inputs(rng, F, N, 31) if messages == "i8" else PR.f32_inputs(rng, F, N)
    llr = np.roll(llr, seed, axis=0)       # the special frames of the generators (all -32, all 0, +-0.0) land in other frames of the decoy
    fv = rng.integers(0, 2, (F, N), dtype=np.uint8)
    return SimpleNamespace(llr=llr, fv=fv, u_in=rng.integers(0, 2, (F, N), dtype=np.uint8), u_in2=rng.integers(0, 2, (F, N), dtype=np.uint8))


_POLAR = {}
POLAR_CODE_SEED = {(8, "ssc"): 1}      # the first clustered code of N = 256 holds a handful of information bits: two frames decode to the same row


def polar_case(n, messages, rule):
    """a random code of N = 2^n, true inputs and decoy, and the restatement's outputs of both: decode (SC or SSC), encode, tally"""
    key = (n, messages, rule)
    if key in _POLAR:
        return _POLAR[key]
    rng = np.random.default_rng([n, 9, POLAR_CODE_SEED.get((n, rule), 0)])
    N = 1 << n
    pos, mask = polar_ssc_ref.clustered_code(rng, n) if rule == "ssc" else PR.random_code(rng, N, N // 2)
    c = SimpleNamespace(n=n, N=N, pos=np.asarray(pos, np.int32), mask=mask, inp={}, ref={})
    for which, seed in (("true", 1), ("decoy", 2)):
        i = c.inp[which] = polar_inputs(n, messages, seed)
        if rule == "ssc":
            u, x, _ = polar_ssc_ref.decode(i.llr, mask, i.fv, messages, 31)
            r = dict(u=PR.pack(u), x=PR.pack(x), info=PR.pack(u[:, c.pos]))
        else:
            u, x, leaf = PR.decode(i.llr, mask, i.fv, messages, 31)
            r = dict(u=PR.pack(u), x=PR.pack(x), info=PR.pack(u[:, c.pos]), leaf=leaf.astype(np.int8 if messages == "i8" else np.float32))
        r["encode"], r["encode in place"] = PR.pack(PR.encode(i.u_in)), PR.pack(PR.encode(i.u_in2))
        c.ref[which] = r
    differ_in_every_frame(c.ref["true"], c.ref["decoy"], "polar n=%d %s %s" % key)
    _POLAR[key] = c
    return c


def polar_tensors(ch, c):
    t, d = c.inp["true"], c.inp["decoy"]
    return SimpleNamespace(llr=ch.input(t.llr, d.llr), fz=ch.input(PR.pack(t.fv), PR.pack(d.fv)), u_in=ch.input(PR.pack(t.u_in), PR.pack(d.u_in)),
                           u_in2=ch.input(PR.pack(t.u_in2), PR.pack(d.u_in2)))


def polar_calls(dec, ch, x, leaf, tag=""):
    for k, v in dec.decode(x.llr, x.fz, leaf=leaf).items():
        ch.keep(tag + k, v)
    ch.keep(tag + "encode", dec.encode(x.u_in))
    ch.keep(tag + "encode in place", dec.encode(x.u_in2, out=x.u_in2), in_place=True)


POLAR_CASES = [(8, "lanes", "sc"), (8, "wide", "sc"), (8, "lanes", "ssc"), (14, "lanes", "sc"), (14, "wide", "sc"), (14, "lanes", "ssc")]


@pytest.mark.parametrize("messages", ["i8", "f32"])
@pytest.mark.parametrize("n,form,rule", POLAR_CASES, ids=["n%d-%s-%s" % c for c in POLAR_CASES])
def test_polar_on_a_side_stream(q, torch, delay, sides, n, form, rule, messages):
    """decode (every output), encode and encode in place under torch.cuda.stream(side): the binding puts the context on torch's current stream.
    65 frames; n = 14: levels 6 .. 13 live in the context's scratch"""
    c = polar_case(n, messages, rule)
    dec = q.Polar(n, c.pos, messages, 31, max_frames=65, form=form, rule=rule)
    ch = Chain(torch, delay, sides[0], "polar n=%d %s %s %s" % (n, form, rule, messages))
    x = polar_tensors(ch, c)
    with ch:
        ch.stage()
        polar_calls(dec, ch, x, leaf=rule == "sc")
    ch.check_all(c.ref["true"])


@pytest.mark.parametrize("messages", ["i8", "f32"])
def test_polar_tally_on_a_side_stream(q, torch, delay, sides, messages):
    """the tally of the genie-aided construction, into a fresh row and added to a row that holds an earlier tally (what a construction does batch
    after batch); n = 8, 65 frames"""
    n, F = 8, 65
    c = polar_case(n, messages, "sc")
    ref = {k: polar_tally_ref.tally(c.inp[k].llr, c.inp[k].fv, messages, 31) for k in ("true", "decoy")}
    earlier = np.random.default_rng(4).integers(0, 1000, (2, c.N)).astype(np.uint64)
    want = {"tally": ref["true"].astype(np.int64), "tally added": (ref["true"] + earlier).astype(np.int64)}
    differ_in_every_frame({"tally": ref["true"]}, {"tally": ref["decoy"]}, "tally", whole=("tally",))
    dec = q.Polar(n, c.pos, messages, 31, max_frames=F)
    ch = Chain(torch, delay, sides[0], "polar tally %s" % messages)
    x = polar_tensors(ch, c)
    acc = dev(torch, earlier.astype(np.int64))
    with ch:
        ch.stage()
        ch.keep("tally", dec.tally(x.llr, x.fz))
        ch.keep("tally added", dec.tally(x.llr, x.fz, out=acc))
    ch.check_all(want)


_LIST = {}


def list_case(with_crc):
    """n = 8, list size 4, int8 messages, 65 frames.  With the CRC the expected remainder of frame f is that of the second path of the true list where f is
    even and one no path has where f is odd, and the other way round in the decoy: the pick differs in every frame"""
    if with_crc in _LIST:
        return _LIST[with_crc]
    n, L, F = 8, 4, 65
    base = polar_case(n, "i8", "sc")
    crc_len, crc_poly = LR.CRC11 if with_crc else (0, 0)
    c = SimpleNamespace(n=n, L=L, pos=base.pos, crc_len=crc_len, crc_poly=crc_poly, inp=base.inp, crc={}, ref={})
    for which, phase in (("true", 0), ("decoy", 1)):
        i = base.inp[which]
        crc = None
        if with_crc:
            free = LR.decode(i.llr, base.mask, i.fv, "i8", 31, L, c.pos, 0, 0)
            paths = np.stack([PR.encode(free["list_x"][:, k]) for k in range(L)], axis=1)                 # u of every path [F, L, N]
            rem = np.stack([LR.crc_bits(paths[:, k][:, c.pos], crc_len, crc_poly) for k in range(L)], axis=1)
            miss = np.array([next(v for v in range(1 << crc_len) if v not in set(row.tolist())) for row in rem], np.uint32)
            crc = np.where(np.arange(F) % 2 == phase, rem[:, 1], miss).astype(np.uint32)
        r = LR.decode(i.llr, base.mask, i.fv, "i8", 31, L, c.pos, crc_len, crc_poly, crc)
        c.crc[which] = crc
        c.ref[which] = dict(u=PR.pack(r["u"]), x=PR.pack(r["x"]), info=PR.pack(r["info"]), pick=r["pick"], metric=r["metric"],
                            list_x=PR.pack(r["list_x"].reshape(F * L, -1)).reshape(F, L, -1))
    constant = () if with_crc else ("pick",)
    differ_in_every_frame(*({k: v for k, v in c.ref[w].items() if k not in constant} for w in ("true", "decoy")), "polar list crc=%s" % with_crc)
    _LIST[with_crc] = c
    return c


@pytest.mark.parametrize("with_crc", [True, False], ids=["crc11", "no_crc"])
def test_polar_list_on_a_side_stream(q, torch, delay, sides, with_crc):
    c = list_case(with_crc)
    dec = q.PolarList(c.n, c.pos, "i8", 31, c.L, c.crc_len, c.crc_poly, max_frames=65)
    ch = Chain(torch, delay, sides[0], "polar list, crc %s" % with_crc)
    t, d = c.inp["true"], c.inp["decoy"]
    llr, fz = ch.input(t.llr, d.llr), ch.input(PR.pack(t.fv), PR.pack(d.fv))
    crc = ch.input(c.crc["true"], c.crc["decoy"]) if with_crc else None
    with ch:
        ch.stage()
        for k, v in dec.decode(llr, fz, crc).items():
            ch.keep(k, v)
    ch.check_all(c.ref["true"])


# ---------------------------------------------------------------- the QBER estimate

N_GRID = 64
# the QBERs of the even and the odd frames: they differ frame by frame and in the pool.  The checks of the rate-0.8 chain code have degree 17 and more
# and tell QBERs above a few per cent apart badly, so its levels are lower
QBER_LEVELS = {False: dict(true=(0.02, 0.12), decoy=(0.20, 0.05)), True: dict(true=(0.004, 0.05), decoy=(0.08, 0.01))}
_QBER = {}


def qber_case(q, name, merged):
    """65 frames of `name` with every input present (classes, shortening, syndrome, erasures, known bits) at the QBERs of QBER_LEVELS.  Counts by the
    restatement in Python integers, the argmax by its restatement over the library's tables"""
    key = (name, merged)
    if key in _QBER:
        return _QBER[key]
    F = 65
    code = qber_ref.make_code(q, name)
    N, M = code.N, code.M
    var, chk = code.edges()
    D = qber_merge_ref.MAX_DEGREE if merged else code.max_cn_degree
    L1, L0, qs, mags = q.qber_table_host(D, N_GRID)
    cls = classes_of(N)
    if merged:
        cls[N - M:] = 0
    c = SimpleNamespace(code=code, F=F, cls=cls, inp={}, ref={}, rows=D + 1)
    for which, phase in (("true", 0), ("decoy", 1)):
        rng = np.random.default_rng([5 + phase, N])
        p = np.where(np.arange(F) % 2 == 0, *QBER_LEVELS[merged][which])
        x = rng.integers(0, 2, (F, N)).astype(np.uint8)
        f = dict(bits=x ^ (rng.random((F, N)) < p[:, None]), cls=cls, nch=rng.integers(N - 40, N + 1, F).astype(np.int32),
                 synd=np.stack([code.syndrome(r)[1] for r in x]).astype(np.uint8), erase=(rng.random((F, N)) < 0.03).astype(np.uint8),
                 known=(rng.random((F, N)) < 0.04).astype(np.uint8), value=x.copy())
        f["bits"] = f["bits"].astype(np.uint8)
        if merged:
            f["erase"][:, N - M:] |= (rng.random((F, M)) < 0.3).astype(np.uint8)      # runs of checks across erased accumulator VNs
            cnt = np.array([qber_merge_ref.frame_counts(var, chk, N, M, f, i) for i in range(F)], np.int64)
        else:
            cnt = np.array([qber_ref.frame_counts(var, chk, N, M, D, f, i) for i in range(F)], np.int64)
        k = np.array([qber_ref.argmax(cnt[i].tolist(), L1.tolist(), L0.tolist()) for i in range(F)], np.int32)
        assert (k >= 0).all()
        pool = cnt.sum(axis=0)
        c.inp[which] = f
        c.ref[which] = dict(counts=cnt.astype(np.int32), index=k, qber=qs[k].astype(np.float32), llr_mag=mags[k].astype(np.float32), pool_counts=pool.astype(np.int64),
                            pool_index=np.array([qber_ref.argmax(pool.tolist(), L1.tolist(), L0.tolist())], np.int32))
    differ_in_every_frame(c.ref["true"], c.ref["decoy"], "qber %s merged=%s" % key, whole=("pool_counts", "pool_index"))
    _QBER[key] = c
    return c


def qber_tensors(torch, q, ch, c):
    t, d = c.inp["true"], c.inp["decoy"]
    x = {k: ch.input(u32(q.pack_bits(t[k])), u32(q.pack_bits(d[k]))) for k in ("bits", "synd", "erase", "known", "value")}
    x["nch"], x["cls"] = ch.input(t["nch"], d["nch"]), dev(torch, c.cls)
    return x


def qber_estimate(est, x, **kw):
    return est.estimate(x["bits"], x["cls"], x["nch"], x["synd"], x["erase"], x["known"], x["value"], **kw)


PER_FRAME, POOLED = ("counts", "index", "qber", "llr_mag"), ("pool_counts", "pool_index")


@pytest.mark.parametrize("form", ["plain", "merged", "pool"])
def test_qber_estimate_on_a_side_stream(q, torch, delay, sides, form):
    """plain: the per-frame estimates alone (PEGReg504x1008); merged: the merged count on an IRA chain; pool: with the pooled outputs"""
    c = qber_case(q, "ira1280" if form == "merged" else "peg504", form == "merged")
    est = q.QberEstimator(c.code, c.F, n_grid=N_GRID, merge=form == "merged")
    assert est.rows == c.rows
    ch = Chain(torch, delay, sides[0], "qber estimate, %s" % form)
    x = qber_tensors(torch, q, ch, c)
    names = PER_FRAME + (POOLED if form != "plain" else ())
    with ch:
        est.set_stream(sides[0])
        ch.stage()
        out = qber_estimate(est, x, pool=form != "plain")
        for k in names:
            ch.keep(k, out[k])
    ch.check_all({k: c.ref["true"][k] for k in names})


# ---------------------------------------------------------------- the encoder

def gf2_codewords(code, enc, info):
    """x with H x = 0 and x[info_bits_pos] = info, by Gaussian elimination over GF(2) on the parity columns: the numpy restatement of an encoder"""
    var, chk = code.edges()
    N, M = code.N, code.M
    H = np.zeros((M, N), np.uint8)
    H[chk, var] = 1
    par = np.setdiff1d(np.arange(N), enc.info_bits_pos)
    R = len(par)
    assert R == M
    A = np.concatenate([H[:, par], ((H[:, enc.info_bits_pos].astype(np.int64) @ info.T.astype(np.int64)) & 1).astype(np.uint8)], axis=1)      # [M, R + F]
    for col in range(R):
        hit = np.flatnonzero(A[col:, col]) + col
        assert hit.size, "the parity part of H is not invertible"
        A[[col, hit[0]]] = A[[hit[0], col]]
        others = np.flatnonzero(A[:, col])
        others = others[others != col]
        A[others] ^= A[col]
    x = np.zeros((info.shape[0], N), np.uint8)
    x[:, enc.info_bits_pos] = info
    x[:, par] = A[:, R:].T
    assert not ((H.astype(np.int64) @ x.T.astype(np.int64)) & 1).any()
    return x


@pytest.mark.parametrize("method", ["IRA", "IDENTITY"])
def test_encoder_on_a_side_stream(q, torch, delay, sides, method):
    """encode_packed(stream=side).  First chain: the call that first grows the workspace (3 frames) and a later, larger one (65); a growing call waits
    for the device, so each has its own delay.  Second chain: calls that fit (2 and 65 frames), which wait for nothing.  IRA: M = 504 (N = 1 008);
    IDENTITY: PEGReg504x1008"""
    code = q.Code.ira(1008, 504) if method == "IRA" else qber_ref.make_code(q, "peg504")
    enc = q.Encoder(code, method)
    chains = ((3, 65), (2, 65))
    rng = np.random.default_rng(8)
    info = rng.integers(0, 2, (2 * sum(sum(c) for c in chains), enc.K)).astype(np.uint8)
    cw = gf2_codewords(code, enc, info)
    at = 0
    for grows, sizes in zip((True, False), chains):
        ch = Chain(torch, delay, sides[0], "encode_packed %s, %s" % (method, "growing" if grows else "grown"), host_waits=grows)
        want, x = {}, []
        for i, F in enumerate(sizes):
            true, decoy = slice(at, at + F), slice(at + F, at + 2 * F)
            at += 2 * F
            differ_in_every_frame({"cw": cw[true]}, {"cw": cw[decoy]}, "encoder %s %d frames" % (method, F))
            want["call %d" % i] = u32(q.pack_bits(cw[true]))
            x.append(ch.input(u32(q.pack_bits(info[true])), u32(q.pack_bits(info[decoy]))))
        with ch:
            for i, t in enumerate(x):
                if grows or i == 0:
                    ch.stage()
                ch.keep("call %d" % i, enc.encode_packed(t, stream=sides[0]))
        ch.check_all(want)


# ---------------------------------------------------------------- the guess and verify helpers

def test_guess_helpers_on_a_side_stream(q, torch, delay, sides):
    """guess_expand and guess_pick with stream=side against their host mirrors (N = 1 008, g = 3, 5 sources: 40 trial slots)"""
    import blind_ref
    N, g, n = 1008, 3, 5
    T, W = 1 << g, (N + 31) // 32
    src = {}
    for which, seed in (("true", 1), ("decoy", 2)):
        rng = np.random.default_rng(seed)
        weak = np.zeros((n, N), np.uint8)
        for s in range(n):
            weak[s, rng.choice(N, g, replace=False)] = 1
        hard = rng.integers(0, 2, (n, N)).astype(np.uint8)
        ok = np.zeros((n, T), np.int32)
        ok[np.arange(n), rng.integers(0, T, n) if which == "true" else (src["true"]["win"] + 1) % T] = 1
        rows = rng.integers(0, 2 ** 32, (n * T, W), dtype=np.uint64).astype(np.uint32)
        weak_w, hard_w = np.stack([blind_ref.pack_row(r) for r in weak]), np.stack([blind_ref.pack_row(r) for r in hard])
        trials = [q.guess_trial_host(N, g, t, weak_w[s], hard_w[s]) for s in range(n) for t in range(T)]
        picks = [q.guess_pick_host(N, g, ok[s], rows[s * T:(s + 1) * T]) for s in range(n)]
        win = np.array([p[0] for p in picks], np.int32)
        src[which] = dict(weak=weak_w, hard=hard_w, ok=ok.reshape(-1), rows=rows, win=win,
                          ref=dict(known=np.stack([k for k, _ in trials]), value=np.stack([v for _, v in trials]), winner=win,
                                   out_hard=np.stack([rows[s * T + win[s]] for s in range(n)])))
    per_source = lambda r: {k: v.reshape(n, -1) for k, v in r.items()}      # the trials of a source together: a value row alone may be all zero in both
    differ_in_every_frame(per_source(src["true"]["ref"]), per_source(src["decoy"]["ref"]), "guess helpers")
    ch = Chain(torch, delay, sides[0], "guess_expand and guess_pick")
    x = {k: ch.input(src["true"][k], src["decoy"][k]) for k in ("weak", "hard", "ok", "rows")}
    out_hard = torch.zeros((n, W), dtype=torch.int32, device="cuda")
    with ch:
        ch.stage()
        known, value = q.guess_expand(N, g, x["weak"], x["hard"], stream=sides[0])
        ch.keep("known", known), ch.keep("value", value)
        win, nok, amb = q.guess_pick(N, g, x["ok"], x["rows"], out_hard, stream=sides[0])
        ch.keep("winner", win), ch.keep("out_hard", out_hard)
    ch.check_all(src["true"]["ref"])


def test_recon_guess_settle_on_a_side_stream(q, torch, delay, sides):
    """recon_guess_settle(stream=side) against the restatement of tests/recon_guess_ref.py: 3 sources of 8 trials, keys of 1 000 bits.  The call
    brings its results to the host itself, on the stream"""
    g, kb, n = 3, 1000, 3
    T, Wk, Wn = 1 << g, (kb + 31) // 32 + 1, 64
    b, ref = {}, {}
    for which, seed, kinds in (("true", 1, ["xwaxxxxx", "xaxaxxxx", "wfxwxxxx"]), ("decoy", 2, ["wfxwxxxx", "xxxxxxxx", "xxxaxxxx"])):
        b[which] = recon_guess_ref.batch(np.random.default_rng(seed), g, [kb] * n, Wk, Wn, kinds)
        w = b[which]
        ref[which] = recon_guess_ref.settle(g, w["rows"], w["ok"], w["iters"], w["keys"], w["key_bits"], w["want"], w["first"])
    cmp_ = lambda r: {k: np.asarray(r[k]).reshape(n, -1) for k in ("status", "corrected", "iterations", "crc", "keys", "guess", "passed", "trial_crc")}
    differ_in_every_frame(cmp_(ref["true"]), cmp_(ref["decoy"]), "recon_guess_settle")
    ch = Chain(torch, delay, sides[0], "recon_guess_settle", host_waits=True)
    x = {k: ch.input(np.asarray(b["true"][k]), np.asarray(b["decoy"][k])) for k in ("rows", "ok", "iters", "keys", "want", "first")}
    key_bits = dev(torch, b["true"]["key_bits"])
    with ch:
        ch.stage()
        got = q.recon_guess_settle(g, x["rows"], x["ok"], x["iters"], x["keys"], key_bits, x["want"], x["first"], stream=sides[0])
    assert recon_guess_ref.same(got, ref["true"]) is None, recon_guess_ref.same(got, ref["true"])
    assert recon_guess_ref.same(got, ref["decoy"]) is not None


def test_recon_verify_tag_on_a_side_stream(q, torch, delay, sides):
    """recon_verify_tag(stream=side) against tests/recon_tag_ref.py: six blocks of 1 000 .. 1 005 bits under two shared hash keys; block b is a good one
    in the true inputs where it is a failed decode in the decoy, and the other way round"""
    bits = [1000, 1001, 1002, 1003, 1004, 1005]
    n = len(bits)
    B, want = {}, {}
    for which, phase in (("true", 0), ("decoy", 1)):
        w = B[which] = recon_tag_ref.batch(q, np.random.default_rng(1 + phase), bits, 2, True)
        for b in range(n):
            w["crc_want"][b] = q.crc32_words(w["alice"][b], bits[b])
            w["ok"][b] = int(b % 2 == phase)
        w["iters"] = (np.arange(n) + 1 + 10 * phase).astype(np.int32)
        want[which] = recon_tag_ref.expected(q, w)
    differ_in_every_frame(*({k: np.asarray(want[w][k]).reshape(n, -1) for k in ("status", "corrected", "iterations", "crc", "keys", "tags")} for w in ("true", "decoy")),
                          "recon_verify_tag")
    ch = Chain(torch, delay, sides[0], "recon_verify_tag", host_waits=True)
    t, d = B["true"], B["decoy"]
    x = {k: ch.input(np.asarray(t[k]), np.asarray(d[k])) for k in ("out", "keys", "crc_want", "ok", "iters", "hash_keys")}
    key_bits = dev(torch, np.asarray(t["key_bits"], np.int32))
    with ch:
        ch.stage()
        got = q.recon_verify_tag(x["out"], x["keys"], key_bits, x["crc_want"], x["ok"], x["iters"], x["hash_keys"], stream=sides[0])
    recon_tag_ref.check_verdict(got, want["true"])


# ---------------------------------------------------------------- the stream switch

def test_decoder_stream_switch(q, O, torch, delay, sides, peg):
    """load on A behind the delay, set_stream(B), run and fetch, wait for B only: the run is ordered after the loads, so the result is the true one"""
    A, B = sides
    case = decoder_case(q, O, peg, "flood_f32", False)
    dec = case.decoder(q)
    on_a = Chain(torch, delay, A, "decoder stream switch: loads on A")
    x = case.inputs(torch, on_a, q)
    case.load(dec, x)
    dec.run()
    with on_a:
        dec.set_stream(A)
        on_a.stage()
        case.load(dec, x)
        on_a.issued()
        on_b = Chain(torch, delay, B, "decoder stream switch: run and fetches on B", behind=on_a)
        with on_b:
            dec.set_stream(B)
            dec.run()
            case.fetch(dec, on_b)
        got = on_b.host                      # on the host before A is waited for
        what = [k for k, w in case.expect("decoy").items() if same_bits(got[k], w)]
        print("stream switch: outputs equal to the DECOY's reference:", what)
    on_b.check_all(case.expect("true"))


def test_qber_stream_switch(q, torch, delay, sides):
    """a first estimate into the estimator's own counts on A behind the delay, a second one on B into the same counts: the second comes after the first
    and after the inputs A brings, and both are exact"""
    A, B = sides
    c = qber_case(q, "peg504", False)
    est = q.QberEstimator(c.code, c.F, n_grid=N_GRID)
    on_a = Chain(torch, delay, A, "qber stream switch: first estimate on A")
    x = qber_tensors(torch, q, on_a, c)
    own = lambda t: q._L.qldpc_qber_estimate_dev(est._h, *[q._vp(x[k].data_ptr()) for k in ("bits", "cls", "nch", "synd", "erase", "known", "value")], c.F, None,
                                                 *[q._vp(t[k].data_ptr()) for k in ("index", "qber", "llr_mag")], None, None)
    outs = [{k: torch.zeros(c.F, dtype=torch.int32 if k == "index" else torch.float32, device="cuda") for k in ("index", "qber", "llr_mag")} for _ in range(2)]
    with on_a:
        est.set_stream(A)
        on_a.stage()
        assert own(outs[0]) == 0
        for k, t in outs[0].items():
            on_a.keep("first " + k, t)
        on_a.issued()
        on_b = Chain(torch, delay, B, "qber stream switch: second estimate on B", behind=on_a)
        with on_b:
            est.set_stream(B)
            assert own(outs[1]) == 0
            for k, t in outs[1].items():
                on_b.keep("second " + k, t)
        what = [k for k in ("index", "qber", "llr_mag") if same_bits(on_b.host["second " + k], c.ref["decoy"][k])]
        print("stream switch: outputs of the second estimate equal to the DECOY's reference:", what)
    on_b.check_all({"second " + k: c.ref["true"][k] for k in ("index", "qber", "llr_mag")})
    on_a.check_all({"first " + k: c.ref["true"][k] for k in ("index", "qber", "llr_mag")})


def test_polar_stream_switch(q, torch, delay, sides):
    """one context, two decodes under two torch.cuda.stream blocks: X1 on A behind the delay, X2 on B.  They share the context's scratch (n = 14), so
    the second is ordered after the first.  This states the contract; without the rule it can pass by luck, the calls need not overlap"""
    A, B = sides
    c = polar_case(14, "i8", "sc")
    dec = q.Polar(14, c.pos, "i8", 31, max_frames=65)
    on_a = Chain(torch, delay, A, "polar stream switch: X1 on A")
    on_b = Chain(torch, delay, B, "polar stream switch: X2 on B", behind=on_a)
    t, d = c.inp["true"], c.inp["decoy"]
    x1 = SimpleNamespace(llr=on_a.input(t.llr, d.llr), fz=on_a.input(PR.pack(t.fv), PR.pack(d.fv)))
    x2 = SimpleNamespace(llr=dev(torch, d.llr), fz=dev(torch, PR.pack(d.fv)))      # X2 is the decoy's frames, unchanged all along
    with on_a:
        on_a.stage()
        for k, v in dec.decode(x1.llr, x1.fz, leaf=True).items():
            on_a.keep("X1 " + k, v)
        on_a.issued()
        with on_b:
            for k, v in dec.decode(x2.llr, x2.fz, leaf=True).items():
                on_b.keep("X2 " + k, v)
    names = ("u", "info", "x", "leaf")
    on_a.check_all({"X1 " + k: c.ref["true"][k] for k in names})
    on_b.check_all({"X2 " + k: c.ref["decoy"][k] for k in names})


# ---------------------------------------------------------------- the detector detects

def test_control_decoder_left_on_the_null_stream(q, O, torch, delay, sides, peg):
    """the inputs are produced on the side stream behind the delay, the decoder stays on the null stream: it must return the DECOY's reference exactly.
    The side stream does not hold the null stream back, and the delay outlasts the calls"""
    case = decoder_case(q, O, peg, "flood_f32", False)
    dec = case.decoder(q)
    ch = Chain(torch, delay, sides[0], "control: " + case.what, control=True)
    x = case.inputs(torch, ch, q)
    case.load(dec, x)
    dec.run()
    with ch:
        ch.stage()
        ch.off_side()
        case.load(dec, x)
        dec.run()
        case.fetch(dec, ch)
    ch.check_all(case.expect("decoy"))


def test_control_polar_left_on_the_null_stream(q, torch, delay, sides):
    c = polar_case(8, "i8", "sc")
    dec = q.Polar(8, c.pos, "i8", 31, max_frames=65)
    ch = Chain(torch, delay, sides[0], "control: polar lanes", control=True)
    x = polar_tensors(ch, c)
    with ch:
        ch.stage()
        ch.off_side()
        for k, v in dec.decode(x.llr, x.fz, leaf=True).items():
            ch.keep(k, v)
    ch.check_all({k: c.ref["decoy"][k] for k in ("u", "info", "x", "leaf")})


def test_control_qber_left_on_the_null_stream(q, torch, delay, sides):
    c = qber_case(q, "peg504", False)
    est = q.QberEstimator(c.code, c.F, n_grid=N_GRID)
    ch = Chain(torch, delay, sides[0], "control: qber estimate", control=True)
    x = qber_tensors(torch, q, ch, c)
    with ch:
        ch.stage()
        ch.off_side()
        out = qber_estimate(est, x)
        for k in PER_FRAME + POOLED:
            ch.keep(k, out[k])
    ch.check_all({k: c.ref["decoy"][k] for k in PER_FRAME + POOLED})
