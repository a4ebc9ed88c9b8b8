"""GPU suite: blind reconciliation at the decoder -- the weakest-VN select over the posterior rows (qldpc_fetch_weakest_dev) against the lexsort
of tests/blind_ref.py, the known-bit loads (qldpc_load_known_dev) against the oracle on LLRs with +-23.03 written in, and the round loop built
from the two against the same loop over the oracle.  70 blocks of PEGReg504x1008 at QBER 9 % (a rate-0.5 code at f = 1.15: most first decodes
fail), syndrome form, NMS 0.75, 50 iterations, early exit."""
import os

import numpy as np
import pytest

import blind_ref

pytestmark = pytest.mark.gpu

N, M, F, QBER, N_ITE = 1008, 504, 70, 0.09, 50
DS = [0, 1, 16, 1008, 2000]


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def i32(words):
    return np.ascontiguousarray(words).astype(np.int64).astype(np.uint32).view(np.int32)


def dev_bits(q, torch, bits):
    return torch.from_numpy(i32(q.pack_bits(bits))).cuda()


class Case:
    """the 70 blocks, drawn block by block, and the oracle's first decode of them per schedule (computed once, never changed)"""

    def __init__(self, q, O, gold):
        p = os.path.join(gold, "PEGReg504x1008.alist")
        self.code, self.og = q.Code.from_alist(p), O.Graph.from_alist(p)
        self.ogl, self.order = blind_ref.layered_graph(O, self.code, self.og)
        a, b = [], []
        for s in range(F):
            rng = np.random.default_rng(s)
            a_ = rng.integers(0, 2, N).astype(np.int32)
            a.append(a_)
            b.append(a_ ^ (rng.random(N) < QBER))
        self.a, self.b = np.stack(a).astype(np.uint8), np.stack(b).astype(np.uint8)
        self.s = np.stack([self.og.syndrome(x)[1] for x in self.a]).astype(np.uint8)
        self.mag = np.float32(np.log(0.91 / 0.09))
        self.llr = np.where(self.b == 1, -self.mag, self.mag).astype(np.float32)
        self.O = O
        self._first = {}

    def oracle(self, sched, llr, rows=None, i8=False, n_ite=N_ITE, synd=True):
        s = self.s if rows is None else self.s[rows]
        if sched == "hlayered":
            return self.O.decode(self.ogl, llr, "NMS", 0.75, n_ite, "hlayered", synd, 1, n_threads=8, target=s[:, self.order], msg_i8=i8)
        return self.O.decode(self.og, llr, "NMS", 0.75, n_ite, "flooding", synd, 1, n_threads=8, target=s, msg_i8=i8)

    def first(self, sched):
        if sched not in self._first:
            self._first[sched] = self.oracle(sched, self.llr)
        return self._first[sched]


@pytest.fixture(scope="module")
def case(q, O, gold):
    return Case(q, O, gold)


def decoder(q, case, sched, dtype="f32", V=1, freeze=True, n_frames=F, n_ite=N_ITE, synd=True):
    return q.Decoder(case.code, N, n_ite, rule="NMS", rule_param=0.75, n_frames=n_frames, schedule=sched, frames_per_lane=V, engine="frames",
                     freeze_messages=freeze, msg_dtype=dtype, enable_syndrome=synd)


def run(q, torch, case, dec, llr, rows=None, known=None, value=None, erase=None, known_first=True):
    s = case.s if rows is None else case.s[rows]
    dec.load_llr(torch.from_numpy(np.ascontiguousarray(llr, np.float32)).cuda())
    dec.load_syndrome(dev_bits(q, torch, s))
    if known is not None and known_first:
        dec.load_known(dev_bits(q, torch, known), dev_bits(q, torch, value))
    if erase is not None:
        dec.load_erasures(dev_bits(q, torch, erase))
    if known is not None and not known_first:
        dec.load_known(dev_bits(q, torch, known), dev_bits(q, torch, value))
    dec.run()
    return status(q, dec)


def status(q, dec):
    hard = q.unpack_bits(dec.fetch_packed().cpu().numpy().view(np.uint32), N)
    it, ok = dec.fetch_status()
    return hard, it.cpu().numpy(), ok.cpu().numpy()


def weak(dec, d, cand=None, take=None):
    return dec.fetch_weakest(d, cand, take).cpu().numpy().view(np.uint32)


# ---------------------------------------------------------------- the select, exact

# (schedule, messages, frames per lane, messages frozen).  8-bit messages exist with 4 frames per lane and unfrozen messages only (0 = auto gives the
# same decoder): the 70 frames are then one group whose third and fourth 64 hold no frame.  Layered fp32 sweeps with freeze = False keep the
# compressed check state.
CONFIGS = [("flooding", "f32", 1, True), ("flooding", "f32", 2, True), ("hlayered", "f32", 1, False), ("hlayered", "f32", 2, True),
           ("flooding", "i8", 0, False), ("flooding", "i8", 4, False), ("hlayered", "i8", 0, False)]


@pytest.mark.parametrize("sched,dtype,V,freeze", CONFIGS)
def test_select_equals_the_lexsort_of_fetch_post(q, torch, case, sched, dtype, V, freeze):
    dec = decoder(q, case, sched, dtype, V, freeze)
    hard, it, ok = run(q, torch, case, dec, case.llr)
    post = dec.fetch_post().cpu().numpy()
    failed = ok == 0
    assert 0 < failed.sum() < F
    ref = case.first(sched) if dtype == "f32" else None
    if ref is not None:
        assert (ok == ref["synd_ok"]).all() and (it == ref["iters"]).all()
        exact = np.ones(F, bool) if freeze else failed              # a converged frame whose messages are not frozen goes on sweeping
        assert (post[exact].view(np.uint32) == ref["post"][exact].view(np.uint32)).all()
    for d in DS:
        got = weak(dec, d)
        assert (got == blind_ref.weakest_rows(post, d)).all(), d
        if ref is not None:
            assert (got[exact] == blind_ref.weakest_rows(ref["post"], d)[exact]).all(), d
    rng = np.random.default_rng(11)
    cand = (rng.random((F, N)) < 0.3).astype(np.uint8)
    cand[3] = 0                                                         # a frame without candidates
    take = failed.astype(np.int32)
    for d in DS:
        got = weak(dec, d, dev_bits(q, torch, cand), torch.from_numpy(take).cuda())
        assert (got == blind_ref.weakest_rows(post, d, cand, take)).all(), d
        assert (got[~failed] == 0).all()
    got = weak(dec, 16, None, torch.zeros(F, dtype=torch.int32, device="cuda"))
    assert (got == 0).all()                                             # nobody taken: every workgroup returns at once
    assert (dec.fetch_post().cpu().numpy().view(np.uint32) == post.view(np.uint32)).all()      # the select left the posteriors alone


@pytest.mark.parametrize("V", [1, 2])
def test_select_where_ties_decide(q, torch, case, V):
    """one flooding iteration, no syndrome test: a posterior takes few distinct magnitudes, so most of the order is the index order"""
    dec = decoder(q, case, "flooding", "f32", V, False, n_ite=1, synd=False)
    run(q, torch, case, dec, case.llr)
    post = dec.fetch_post().cpu().numpy()
    assert np.unique(np.abs(post)).size < 40
    ref = case.oracle("flooding", case.llr, n_ite=1, synd=False)
    assert (post.view(np.uint32) == ref["post"].view(np.uint32)).all()
    for d in (1, 16, 300, 777):
        assert (weak(dec, d) == blind_ref.weakest_rows(post, d)).all(), d


def test_select_counts_past_16_bits(q, torch):
    """N = 73 728 with every |posterior| in [2, 8): one histogram bin of the first digit holds all 73 728 keys, and few magnitudes exist"""
    K, Mp, Fr = 65536, 8192, 3
    code = q.Code.ira(K + Mp, K, 0.125, 11, 3, 7)
    dec = q.Decoder(code, K, 1, rule="NMS", rule_param=0.01, n_frames=Fr, enable_syndrome=False, engine="frames")
    rng = np.random.default_rng(2)
    llr = np.where(rng.random((Fr, K + Mp)) < 0.02, -3.5, 3.5).astype(np.float32)
    dec.load_llr(torch.from_numpy(llr).cuda())
    dec.run()
    post = dec.fetch_post().cpu().numpy()
    key = post.view(np.uint32) & 0x7fffffff
    assert all(np.bincount(key[f] >> 24).max() > 65535 for f in range(Fr)) and np.unique(key).size < 64
    for d in (40000, 70000):
        got = dec.fetch_weakest(d).cpu().numpy().view(np.uint32)
        assert (got == blind_ref.weakest_rows(post, d)).all(), d


# ---------------------------------------------------------------- known bits

def known_masks(case, seed):
    rng = np.random.default_rng(seed)
    known = (rng.random((F, N)) < 0.06).astype(np.uint8)
    known[5] = 0
    value = np.where(rng.random((F, 1)) < 0.7, case.a, rng.integers(0, 2, (F, N))).astype(np.uint8)      # mostly Alice's bits, some frames arbitrary
    return known, value


@pytest.mark.parametrize("sched,dtype,V,freeze", [("flooding", "f32", 1, True), ("flooding", "f32", 2, True), ("hlayered", "f32", 1, True),
                                                  ("hlayered", "f32", 1, False), ("flooding", "i8", 0, False)])
def test_load_known_equals_the_oracle_on_pinned_llrs(q, torch, case, sched, dtype, V, freeze):
    known, value = known_masks(case, 21)
    i8 = dtype == "i8"
    ref = case.oracle(sched, blind_ref.pinned(case.llr, known, value), i8=i8)
    dec = decoder(q, case, sched, dtype, V, freeze)
    hard, it, ok = run(q, torch, case, dec, case.llr, known=known, value=value)
    assert (hard == ref["hard"]).all() and (it == ref["iters"]).all() and (ok == ref["synd_ok"]).all()
    if not i8:
        assert (it != case.first(sched)["iters"]).any()             # the known bits change the decode
    post = dec.fetch_post().cpu().numpy()
    exact = np.ones(F, bool) if freeze else ok == 0
    assert (post[exact].view(np.uint32) == ref["post"][exact].view(np.uint32)).all()
    # known wins over erased, in either order of the two loads
    rng = np.random.default_rng(22)
    erase = (rng.random((F, N)) < 0.05).astype(np.uint8)
    erase[:, :64] |= known[:, :64]                                  # make sure the two overlap
    llr_e = np.where(erase != 0, np.float32(0), case.llr).astype(np.float32)
    ref_e = case.oracle(sched, blind_ref.pinned(llr_e, known, value), i8=i8)
    for known_first in (True, False):
        hard, it, ok = run(q, torch, case, dec, case.llr, known=known, value=value, erase=erase, known_first=known_first)
        assert (hard == ref_e["hard"]).all() and (it == ref_e["iters"]).all() and (ok == ref_e["synd_ok"]).all(), known_first
    # the next load clears it
    if not i8:
        hard, it, ok = run(q, torch, case, dec, case.llr)
        ref0 = case.first(sched)
        assert (hard == ref0["hard"]).all() and (it == ref0["iters"]).all() and (ok == ref0["synd_ok"]).all()
        hard, it, ok = run(q, torch, case, dec, case.llr, erase=erase)      # and erasures alone erase again
        ref1 = case.oracle(sched, llr_e)
        assert (hard == ref1["hard"]).all() and (it == ref1["iters"]).all()


@pytest.mark.parametrize("V", [1, 2])
def test_load_known_on_the_coded_form_of_load_bits(q, torch, case, V):
    """load_bits keeps a flooding frame set as received bits + a magnitude; with known bits it runs on the LLR array those stand for"""
    known, value = known_masks(case, 31)
    rng = np.random.default_rng(32)
    erase = (rng.random((F, N)) < 0.03).astype(np.uint8)
    mag = torch.full((F,), float(case.mag), device="cuda")
    out = []
    for form in ("bits", "llr"):
        dec = decoder(q, case, "flooding", "f32", V, True)
        if form == "bits":
            dec.load_bits(dev_bits(q, torch, case.b), mag)
        else:
            dec.load_llr(torch.from_numpy(case.llr).cuda())
        dec.load_erasures(dev_bits(q, torch, erase))
        dec.load_syndrome(dev_bits(q, torch, case.s))
        dec.load_known(dev_bits(q, torch, known), dev_bits(q, torch, value))
        dec.run()
        out.append(status(q, dec) + (dec.fetch_post().cpu().numpy(),))
        if form == "bits":                                           # a fresh load_bits is the coded form again, without known bits
            dec.load_bits(dev_bits(q, torch, case.b), mag)
            dec.load_syndrome(dev_bits(q, torch, case.s))
            dec.run()
            hard, it, ok = status(q, dec)
            ref0 = case.first("flooding")
            assert (hard == ref0["hard"]).all() and (it == ref0["iters"]).all() and (ok == ref0["synd_ok"]).all()
    for x, y in zip(out[0][:3], out[1][:3]):
        assert (x == y).all()
    assert (out[0][3].view(np.uint32) == out[1][3].view(np.uint32)).all()
    llr_e = np.where(erase != 0, np.float32(0), case.llr).astype(np.float32)
    ref = case.oracle("flooding", blind_ref.pinned(llr_e, known, value))
    assert (out[0][0] == ref["hard"]).all() and (out[0][1] == ref["iters"]).all() and (out[0][3].view(np.uint32) == ref["post"].view(np.uint32)).all()


def test_load_known_on_the_edge_engine(q, torch, case):
    known, value = known_masks(case, 41)
    rows = np.arange(4)
    ref = case.oracle("flooding", blind_ref.pinned(case.llr[rows], known[rows], value[rows]), rows=rows)
    dec = q.Decoder(case.code, N, N_ITE, rule="NMS", rule_param=0.75, n_frames=4, engine="edges")
    hard, it, ok = run(q, torch, case, dec, case.llr[rows], rows=rows, known=known[rows], value=value[rows])
    assert (hard == ref["hard"]).all() and (it == ref["iters"]).all() and (ok == ref["synd_ok"]).all()
    with pytest.raises(q.QldpcError) as e:
        dec.fetch_weakest(16)
    assert e.value.status == -7


# ---------------------------------------------------------------- the loop, exact

@pytest.mark.parametrize("sched", ["flooding", "hlayered"])
def test_blind_loop_equals_the_oracle_loop(q, torch, case, sched):
    D, MAX_ROUNDS = 16, 12
    asks, done_ref, hard_ref = blind_ref.loop(lambda llr_rows, live: case.oracle(sched, llr_rows, rows=live), case.llr, case.a, D, MAX_ROUNDS)
    assert (done_ref >= 0).all() and (hard_ref == case.a).all()        # the oracle alone ends on Alice's word within the cap
    done_dev = np.full(F, -1, np.int32)
    known_dev = np.zeros((F, N), np.uint8)
    dec = decoder(q, case, sched, "f32", 1, False)
    rounds = 0
    for r in range(MAX_ROUNDS):
        live = np.flatnonzero(done_dev < 0)
        if live.size == 0:
            break
        rounds = r + 1
        assert (live == np.flatnonzero((done_ref < 0) | (done_ref >= r))).all(), r
        hard, it, ok = run(q, torch, case, dec, case.llr[live], rows=live, known=known_dev[live], value=case.a[live])
        cand = (known_dev[live] == 0).astype(np.uint8)
        got = weak(dec, D, dev_bits(q, torch, cand), torch.from_numpy((ok == 0).astype(np.int32)).cuda())
        ask_dev = np.stack([blind_ref.unpack_row(w, N) for w in got])
        assert (ask_dev == asks[r][live]).all(), r                     # the ask rows of this round
        assert ((ok == 1) == (done_ref[live] == r)).all(), r           # and who succeeds in it
        assert (hard[ok == 1] == case.a[live][ok == 1]).all()
        assert (ask_dev.sum(1)[ok == 0] == D).all() and (ask_dev & known_dev[live]).sum() == 0
        done_dev[live[ok == 1]] = r
        known_dev[live] |= ask_dev
    assert (done_dev >= 0).all() and (done_dev == done_ref).all()      # every block ends on Alice's word within the cap
    assert (done_dev >= 1).any() and (done_dev >= 2).any()             # blocks that need rounds, and one that needs two or more
    print("blind loop %s: rounds %d, blocks by round of success %s, bits disclosed per block %.1f"
          % (sched, rounds, np.bincount(done_dev).tolist(), known_dev.sum() / F))


# ---------------------------------------------------------------- error paths

def test_fetch_weakest_error_paths(q, O, torch, case):
    dec = decoder(q, case, "flooding")
    dec.load_llr(torch.from_numpy(case.llr).cuda())
    with pytest.raises(q.QldpcError) as e:
        dec.fetch_weakest(16)                                         # loaded, not run
    assert e.value.status == -8
    dec.run()
    with pytest.raises(q.QldpcError) as e:
        dec.fetch_weakest(-1)
    assert e.value.status == -1
    with pytest.raises(q.QldpcError) as e:
        dec.load_known(dev_bits(q, torch, case.a[:5]), dev_bits(q, torch, case.a[:5]))      # not the frame count that was loaded
    assert e.value.status == -8
    # after a run that compacted its active frames the posteriors of the frames that left early are gone
    rng = np.random.default_rng(1)
    F2 = 400
    frames = np.where(rng.random((F2, N)) < rng.uniform(0.03, 0.075, (F2, 1)), -2.6, 2.6).astype(np.float32)
    dec2 = q.Decoder(case.code, 504, 30, info_bits_pos=np.arange(504, 1008, dtype=np.int32), rule="NMS", rule_param=0.75, n_frames=F2, compact="on")
    dec2.load_llr(torch.from_numpy(frames).cuda())
    dec2.run()
    assert dec2.last_run_stats()["compactions"] >= 1
    with pytest.raises(q.QldpcError) as e:
        dec2.fetch_weakest(16)
    assert e.value.status == -7


# ---------------------------------------------------------------- sessions

def session_blocks(q):
    """two lengths; per length one block whose plan fits its errors and one planned for a QBER so far below the true one that the bits disclosed
    stay below h(true QBER) per key bit (1 000 bits: 0.40 against 0.44; 5 000 bits: 0.35 against 0.40), so its first decode cannot succeed"""
    rng = np.random.default_rng(5)
    keys, bobs, kb, plan_q = [], [], [], []
    for key_bits, true_q, est_q in [(1000, 0.03, 0.03), (1000, 0.09, 0.025), (5000, 0.08, 0.02), (5000, 0.02, 0.02)]:
        a = rng.integers(0, 2, key_bits).astype(np.uint8)
        b = a ^ (rng.random(key_bits) < true_q)
        keys.append(q.pack_bits(a)); bobs.append(q.pack_bits(b)); kb.append(key_bits); plan_q.append(est_q)
    return keys, bobs, kb, plan_q


def test_session_blind_rounds(q):
    keys, bobs, kb, plan_q = session_blocks(q)
    n = len(keys)
    r = q.Recon(max_blocks=16)                                        # batches: the frames engine, horizontal layered
    msgs, pars = r.encode_blocks(keys, kb, plan_q)
    st0, fixed0, co0, it0 = r.decode_blocks(bobs, kb, plan_q, msgs, pars)
    assert list(st0) == [0, -9, -9, 0]                                # a block that succeeds at once and one that needs rounds share a call
    none = [(np.zeros(0, np.int32), np.zeros(0, np.uint8))] * n
    ask_bits = [k // 8 for k in kb]
    # no known position: the call is decode_blocks
    st, fixed, co, it, lk, asks = r.decode_blind(bobs, kb, plan_q, msgs, pars, none, 125)
    assert (st == st0).all() and (co == co0).all() and (it == it0).all() and all((x == y).all() for x, y in zip(fixed, fixed0))
    assert list(lk) == [r.leaked_bits(m) for m in msgs]
    assert [a.size for a in asks] == [0, 125, 125, 0]
    # the loop, per length with ask_bits = key_bits / 8: at most ceil(key_bits / ask_bits) = 8 requests can be made before every position is known
    for ab in sorted(set(ask_bits)):
        idx = [i for i in range(n) if ask_bits[i] == ab]
        known = {i: (np.zeros(0, np.int32), np.zeros(0, np.uint8)) for i in idx}
        open_ = list(idx)
        rounds = {i: 0 for i in idx}
        bound = -(-kb[idx[0]] // ab)
        for rnd in range(bound + 1):
            sub = open_
            st, fixed, co, it, lk, asks = r.decode_blind([bobs[i] for i in sub], [kb[i] for i in sub], [plan_q[i] for i in sub], [msgs[i] for i in sub],
                                                         [pars[i] for i in sub], [known[i] for i in sub], ab)
            nxt = []
            for t, i in enumerate(sub):
                assert lk[t] == r.leaked_bits(msgs[i]) + known[i][0].size
                if st[t] == 0:
                    assert (q.unpack_bits(fixed[t], kb[i]) == q.unpack_bits(keys[i], kb[i])).all()      # Alice's key, disclosed positions included
                    assert co[t] == int((q.unpack_bits(bobs[i], kb[i]) != q.unpack_bits(keys[i], kb[i])).sum())
                    assert asks[t].size == 0
                    continue
                assert st[t] == -9 and (fixed[t] == bobs[i]).all()    # untouched on failure
                a = asks[t]
                assert a.size == min(ab, kb[i] - known[i][0].size) and (np.diff(a) > 0).all() and a.min() >= 0 and a.max() < kb[i]
                assert np.intersect1d(a, known[i][0]).size == 0       # never a position that is already known
                known[i] = (np.concatenate([known[i][0], a]).astype(np.int32), np.concatenate([known[i][1], q.recon_disclose(keys[i], kb[i], a)]))
                rounds[i] += 1
                nxt.append(i)
            open_ = nxt
            if not open_:
                break
        assert not open_ and max(rounds.values()) <= bound
        print("session blind rounds, %d-bit blocks, %d bits a request: requests per block %s, bits disclosed %s"
              % (kb[idx[0]], ab, [rounds[i] for i in idx], [int(known[i][0].size) for i in idx]))
        assert max(rounds.values()) >= 1


def test_session_blind_argument_errors(q):
    keys, bobs, kb, plan_q = session_blocks(q)
    r = q.Recon(max_blocks=16)
    msgs, pars = r.encode_blocks(keys[:2], kb[:2], plan_q[:2])
    ok = (np.zeros(0, np.int32), np.zeros(0, np.uint8))
    for bad in ([3, 7, 3], [1000], [-1]):
        with pytest.raises(q.QldpcError) as e:
            r.decode_blind(bobs[:2], kb[:2], plan_q[:2], msgs, pars, [ok, (np.array(bad, np.int32), np.zeros(len(bad), np.uint8))], 16)
        assert e.value.status == -1
    with pytest.raises(q.QldpcError) as e:
        r.decode_blind(bobs[:2], kb[:2], plan_q[:2], msgs, pars, [ok, ok], -1)
    assert e.value.status == -1
    r8 = q.Recon(max_blocks=8, schedule="flooding")                  # the edge-parallel engine: refused before anything is decoded
    with pytest.raises(q.QldpcError) as e:
        r8.decode_blind(bobs[:2], kb[:2], plan_q[:2], msgs, pars, [ok, ok], 16)
    assert e.value.status == -7
