"""GPU suite: guessing rounds in reconciliation sessions (qldpc_recon_decode_guess).

1. the verdict kernels (qldpc_recon_guess_settle_dev) against their host mirror on the synthetic sources of tests/recon_guess_ref.py, exactly;
2. the session call against the hand composition of calls that are older than it -- a Decoder on the session's code and configuration, the block's first
   decode, fetch_weakest, guess_expand, the trials through load_known, fetch_status / fetch_packed, and the host mirror of the verdict -- block for block
   and field for field;
3. invariance under shuffling, splitting and max_blocks;  4. a call without a failure, and guess_bits = 0, is decode_blocks;  5. refusals.

The blocks of 2 - 4: 48 blocks of 1 000 and 48 of 2 000 bits, planned at QBER PLAN_Q, true QBERs spread evenly over 1.0 .. SPREAD times it, from SEED.
SEED and SPREAD were pinned on an MI355X with the composition alone (this module's `reference`, which is the reference and not the code under test): the
first seed of 0 .. 15 whose composition shows, for g = 3 and for g = 4, at least 4 blocks decoded at once, at least 2 rescued and at least 2 still failed.
What was tried is in SCAN below: the spread of 1.0 .. 1.5 the issue supposed has no failed block at all on these session codes, so the spread was
widened, not the condition."""
import numpy as np
import pytest

import recon_guess_ref as R

pytestmark = pytest.mark.gpu

PLAN_Q, SPREAD, SEED, PER_LENGTH = 0.03, 3.0, 0, 48
SCAN = """seeds 0 .. 15 each, (blocks decoded at once, rescued, still failed) of the 96 blocks, g = 3 / g = 4 (rate-0.5 codes, 479 of 1 024 and 1 130 of 2 048 parity bits punctured):
spread 1.5: (96, 0, 0) for every seed.  spread 2.0: at most one failed block per seed.
spread 2.5: seed 1 is the first to meet the condition, (89, 2, 5) / (89, 2, 5), but every failed block of every seed is a 2 000-bit block: one code without a source.
spread 3.0: seed 0 meets it, (77, 2, 17) / (77, 2, 17), with 2 failed blocks of 1 000 and 17 of 2 000 bits -- taken: both codes have sources, and the 17 of one
            code span nine trial launches at g = 3.  (seed 1: (78, 1, 17), seed 2: (77, 0, 19) / (77, 1, 18), seed 3: (77, 2, 17) / (77, 3, 16).)
spread 3.5: 24 - 33 still failed per seed, 0 - 6 rescued.  No rescue in any scan was a wrong key, none ambiguous."""
SESSION = dict(max_blocks=16, mother_step=0, key_quantum=1024, rule="NMS", rule_param=0.75)
N_ITE = 60                                                                         # qldpc_recon_cfg_default


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


# ---------------------------------------------------------------- 1. the verdict kernels

def settle_both(q, torch, g, b):
    host = q.recon_guess_settle_host(g, b["rows"], b["ok"], b["iters"], b["keys"], b["key_bits"], b["want"], b["first"])
    got = q.recon_guess_settle(g, dev(torch, b["rows"]), dev(torch, b["ok"]), dev(torch, b["iters"]), dev(torch, b["keys"]), dev(torch, b["key_bits"]),
                               dev(torch, b["want"]), dev(torch, b["first"]))
    return got, host


@pytest.mark.parametrize("n_src", [1, 3])
@pytest.mark.parametrize("g", [0, 1, 6, 7, 10])                                    # T = 1, 2, 64 (one wave), 128, 1024 (four ballot trips)
def test_settle_kernels_equal_the_host_mirror(q, torch, g, n_src):
    rng = np.random.default_rng(10 * g + n_src)
    T = 1 << g
    for kb in [1, 31, 32, 33, 1000]:
        Wk = (kb + 31) // 32 + 1
        kbs = [kb, max(1, kb - 1), kb][:n_src]
        for p_pass, p_wrong in [(0.0, 0.3), (1.0, 0.0), (0.3, 0.3), (2.0 / T, 8.0 / T)]:
            kinds = [R.random_kinds(rng, T, k, p_pass, p_wrong) for k in kbs]
            if n_src == 3:
                kinds[1] = "".join("w" if k in "ac" else k for k in kinds[1])       # a source without a winner beside two that may have one
            b = R.batch(rng, g, kbs, Wk, Wk + 3, kinds)
            got, host = settle_both(q, torch, g, b)
            assert R.same(got, host) is None, (g, n_src, kb, p_pass, R.same(got, host))
            if n_src == 3:                                                         # it keeps the key handed in, and nothing is written past a key's words
                nw = (kbs[1] + 31) // 32
                assert got["status"][1] == -9 and (got["keys"][1, :nw] == b["keys"][1, :nw]).all() and not got["keys"][1, nw:].any()
    if T >= 8:
        for name, (kinds, kb, verdict) in R.hand_built(T).items():
            Wk = (kb + 31) // 32 + 2
            b = R.batch(rng, g, [kb] * n_src, Wk, Wk + 5, [kinds] * n_src)
            got, host = settle_both(q, torch, g, b)
            assert R.same(got, host) is None, name
            assert all(tuple(int(got["guess"][f][s]) for f in ("winner", "n_ok", "n_pass", "ambiguous")) == verdict for s in range(n_src)), name


# ---------------------------------------------------------------- 2. the session call against the hand composition

def blocks(q, seed=SEED, spread=SPREAD, per_length=PER_LENGTH):
    """-> Alice's keys, Bob's keys, key_bits, planned QBERs, true error counts"""
    rng = np.random.default_rng(seed)
    alice, bob, kb, errors = [], [], [], []
    for key_bits in (1000, 2000):
        for true_q in PLAN_Q * np.linspace(1.0, spread, per_length):
            a = rng.integers(0, 2, key_bits).astype(np.uint8)
            b = a ^ (rng.random(key_bits) < true_q)
            alice.append(q.pack_bits(a)); bob.append(q.pack_bits(b)); kb.append(key_bits); errors.append(int((a != b).sum()))
    return alice, bob, kb, [PLAN_Q] * len(kb), errors


def frame_rows(q, msg, bob, parity):
    """the frame of a block as the session assembles it: Bob's key bits below key_bits, zeros up to K, the disclosed parity bits at their positions;
    the erase row = the punctured parity positions (even spacing: position j is punctured iff floor((j + 1) p / M) > floor(j p / M))"""
    K, M, p, kb = int(msg.code_k), int(msg.code_m), int(msg.n_punct), int(msg.key_bits)
    j = np.arange(M, dtype=np.int64)
    punct = ((j + 1) * p) // M > (j * p) // M
    bits, erase = np.zeros(K + M, np.uint8), np.zeros(K + M, np.uint8)
    bits[:kb] = q.unpack_bits(bob, kb)
    bits[K:][~punct] = q.unpack_bits(parity, M - p)
    erase[K:] = punct
    return q.pack_bits(bits), q.pack_bits(erase)


class Composition:
    """the decoder of one session code with the session's configuration, and the steps of the composition on it, at most 16 frames a run"""

    def __init__(self, q, torch, K, M):
        self.q, self.torch, self.K, self.N, self.Wn = q, torch, K, K + M, (K + M + 31) // 32
        self.code = q.Code.ira_peg(K + M, K, depth=2, seed=7)
        self.dec = q.Decoder(self.code, K, N_ITE, rule="NMS", rule_param=0.75, n_frames=16, schedule="hlayered", syndrome_depth=1, layer_chain="off")
        cls = np.ones(self.N, np.uint8)
        cls[:K] = 0
        self.cls = torch.from_numpy(cls).cuda()

    def run(self, bits, erase, mag, kb, known=None, value=None):
        q, torch = self.q, self.torch
        self.dec.load_bits(dev(torch, bits), torch.from_numpy(np.asarray(mag, np.float32)).cuda(), self.cls, n_channel=dev(torch, np.asarray(kb, np.int32)))
        self.dec.load_erasures(dev(torch, erase))
        if known is not None:
            self.dec.load_known(known, value)
        self.dec.run()
        it, ok = self.dec.fetch_status()
        return self.dec.fetch_packed().cpu().numpy().view(np.uint32), it.cpu().numpy(), ok.cpu().numpy()


def reference(q, torch, r, alice, bob, kb, plan_q, gs):
    """-> {g: (status, keys, corrected, iterations, guess rows [n, 6])} by the composition; the first decodes are shared by the values of g"""
    n = len(bob)
    msgs, pars = r.encode_blocks(alice, kb, plan_q)
    mag = float(q.bsc_llr(min(max(PLAN_Q, 0.001), 0.25)))
    out = {g: [np.full(n, -9, np.int32), [k.copy() for k in bob], np.zeros(n, np.int32), np.zeros(n, np.int32), np.tile(np.array([0, -1, 0, 0, 0, 0], np.int32), (n, 1))]
           for g in gs}
    for code in sorted({(int(m.code_k), int(m.code_m)) for m in msgs}):
        comp = Composition(q, torch, *code)
        idx = [i for i in range(n) if (int(msgs[i].code_k), int(msgs[i].code_m)) == code]
        rows = {i: frame_rows(q, msgs[i], bob[i], pars[i]) for i in idx}
        for at in range(0, len(idx), 16):
            sub = idx[at:at + 16]
            hard, it, ok = comp.run(np.stack([rows[i][0] for i in sub]), np.stack([rows[i][1] for i in sub]), [mag] * len(sub), [kb[i] for i in sub])
            good = np.array([bool(ok[t]) and q.crc32_words(hard[t], kb[i]) == int(msgs[i].crc32) for t, i in enumerate(sub)])
            cand = np.stack([np.concatenate([R.mask_words(kb[i]), np.zeros(comp.Wn - (kb[i] + 31) // 32, np.uint32)]) for i in sub])
            weak = {g: comp.dec.fetch_weakest(g, dev(torch, cand), dev(torch, (~good).astype(np.int32))).clone() for g in gs} if not good.all() else {}
            for t, i in enumerate(sub):
                nw = (kb[i] + 31) // 32
                for g in gs:
                    st, keys, co, its, gr = out[g]
                    its[i] = it[t]
                    if good[t]:
                        st[i] = 0
                        keys[i] = hard[t, :nw] & R.mask_words(kb[i])
                        co[i] = int((q.unpack_bits(keys[i], kb[i]) != q.unpack_bits(bob[i], kb[i])).sum())
            first = {i: (hard[t].copy(), int(it[t])) for t, i in enumerate(sub) if not good[t]}
            for t, i in enumerate(sub):
                if good[t]:
                    continue
                for g in gs:
                    T = 1 << g
                    known, value = q.guess_expand(comp.N, g, weak[g][t:t + 1].contiguous(), dev(torch, first[i][0][None]))
                    parts = [comp.run(np.tile(rows[i][0], (min(16, T), 1)), np.tile(rows[i][1], (min(16, T), 1)), [mag] * min(16, T), [kb[i]] * min(16, T),
                                      known[a:a + 16].contiguous(), value[a:a + 16].contiguous()) for a in range(0, T, 16)]
                    Wk = code[0] // 32
                    key_row = np.zeros((1, Wk), np.uint32)
                    key_row[0, :bob[i].size] = bob[i]
                    v = q.recon_guess_settle_host(g, np.concatenate([p[0] for p in parts]), np.concatenate([p[2] for p in parts]), np.concatenate([p[1] for p in parts]),
                                                  key_row, [kb[i]], [int(msgs[i].crc32)], [first[i][1]])
                    st, keys, co, its, gr = out[g]
                    st[i], co[i], its[i] = v["status"][0], v["corrected"][0], v["iterations"][0]
                    gr[i] = [int(v["guess"][f][0]) for f in R.FIELDS]
                    if st[i] == 0:
                        keys[i] = v["keys"][0, :bob[i].size].copy()
    return msgs, pars, out


def counts(ref):
    st, _, _, _, gr = ref
    return int((gr[:, 0] == 0).sum()), int(((gr[:, 0] == 1) & (st == 0)).sum()), int(((gr[:, 0] == 1) & (st != 0)).sum())


@pytest.fixture(scope="module")
def world(q, torch):
    alice, bob, kb, plan_q, errors = blocks(q)
    r = q.Recon(**SESSION)
    msgs, pars, ref = reference(q, torch, r, alice, bob, kb, plan_q, (3, 4))
    return dict(r=r, alice=alice, bob=bob, kb=kb, plan_q=plan_q, errors=errors, msgs=msgs, pars=pars, ref=ref)


def equal(got, want, where=""):
    st, keys, co, it, gr = got
    wst, wkeys, wco, wit, wgr = want
    assert (st == wst).all(), (where, "status", np.flatnonzero(st != wst))
    assert (co == wco).all() and (it == wit).all(), (where, "corrected / iterations", np.flatnonzero((co != wco) | (it != wit)))
    for f, col in zip(R.FIELDS, np.asarray(wgr).T):
        assert (gr[f] == col).all(), (where, f, np.flatnonzero(gr[f] != col))
    assert all((a == b).all() for a, b in zip(keys, wkeys)), (where, "keys")


def as_rows(guess):
    return np.stack([guess[f] for f in R.FIELDS], axis=1)


@pytest.mark.parametrize("g", [3, 4])                                              # S = 2 sources a trial launch (several launches a group), and S = 1
def test_session_call_equals_the_hand_composition(q, world, g):
    w = world
    ref = w["ref"][g]
    at_once, rescued, failed = counts(ref)
    print("composition, g = %d: %d blocks decoded at once, %d rescued, %d still failed" % (g, at_once, rescued, failed))
    assert at_once >= 4 and rescued >= 2 and failed >= 2                           # on the composition alone, first
    got = w["r"].decode_guess(w["bob"], w["kb"], w["plan_q"], w["msgs"], w["pars"], g)
    equal(got, ref, "g = %d" % g)
    st, keys, co, it, gr = got
    for i in range(len(st)):
        if st[i] == 0:
            assert (keys[i] == w["alice"][i]).all() and co[i] == w["errors"][i], i  # rescued or not: Alice's key, the true error count
        else:
            assert st[i] == -9 and (keys[i] == w["bob"][i]).all() and co[i] == 0 and gr["tried"][i] == 1 and gr["winner"][i] == -1
        assert gr["n_pass"][i] <= gr["n_ok"][i] <= (1 << g) and (gr["winner"][i] >= 0) == (gr["n_pass"][i] > 0 and gr["tried"][i] == 1)
    assert [w["r"].leaked_bits(m) for m in w["msgs"]] == [int(m.code_m) - int(m.n_punct) + 32 for m in w["msgs"]]      # nothing is disclosed


# ---------------------------------------------------------------- 3. invariance

def test_results_do_not_depend_on_the_company_a_block_keeps(q, world):
    w, g = world, 3
    n = len(w["bob"])
    ref = w["ref"][g]
    pick = lambda idx, ref=ref: (ref[0][idx], [ref[1][i] for i in idx], ref[2][idx], ref[3][idx], ref[4][idx])
    call = lambda r, idx: r.decode_guess([w["bob"][i] for i in idx], [w["kb"][i] for i in idx], [w["plan_q"][i] for i in idx], [w["msgs"][i] for i in idx],
                                         [w["pars"][i] for i in idx], g)
    perm = np.random.default_rng(1).permutation(n)
    equal(call(w["r"], perm), pick(perm), "shuffled")
    cut = n // 3 + 1                                                               # two calls, neither a whole number of launches
    equal(call(w["r"], np.arange(cut)), pick(np.arange(cut)), "first call of two")
    equal(call(w["r"], np.arange(cut, n)), pick(np.arange(cut, n)), "second call of two")
    r64 = q.Recon(**dict(SESSION, max_blocks=64))
    equal(call(r64, np.arange(n)), pick(np.arange(n)), "max_blocks = 64")


# ---------------------------------------------------------------- 4. nothing failed, or guess_bits = 0: decode_blocks

def launches(r):
    """loads and fetches of the session's decoders: a trial launch would add to both, the weakest-VN select is a fetch (the sweeps are left out: how many
    of them the host queues before it sees the early exit is a matter of timing; expand and settle are no decoder kernels and cannot show here)"""
    return {k["name"]: k["launches"] for k in r.profile_read() if k["name"] in ("load", "fetch", "status")}


def test_without_a_failure_or_with_no_guess_bits_the_call_is_decode_blocks(q, world):
    w = world
    r = q.Recon(**SESSION)
    clean = np.flatnonzero(w["ref"][3][4][:, 0] == 0)
    every = np.arange(len(w["bob"]))
    for idx, g in [(clean, 3), (clean, 4), (every, 0)]:
        args = ([w["bob"][i] for i in idx], [w["kb"][i] for i in idx], [w["plan_q"][i] for i in idx], [w["msgs"][i] for i in idx], [w["pars"][i] for i in idx])
        r.profile(True)
        st0, keys0, co0, it0 = r.decode_blocks(*args)
        plain = launches(r)
        r.profile(True)
        st, keys, co, it, gr = r.decode_guess(*args, g)
        assert launches(r) == plain and plain["load"] and plain["fetch"], (g, plain, launches(r))      # no select and no trial launch
        r.profile(False)
        assert (st == st0).all() and (co == co0).all() and (it == it0).all() and all((a == b).all() for a, b in zip(keys, keys0))
        assert (as_rows(gr) == [0, -1, 0, 0, 0, 0]).all()
        assert (st0 == 0).all() if g else (st0 != 0).any()


# ---------------------------------------------------------------- 5. refusals

def test_refusals(q, world):
    w = world
    r = w["r"]
    few = lambda idx: ([w["bob"][i] for i in idx], [w["kb"][i] for i in idx], [w["plan_q"][i] for i in idx], [w["msgs"][i] for i in idx], [w["pars"][i] for i in idx])
    idx = list(range(40, 48))                                                      # the noisy end of the 1 000-bit blocks
    for g, status in [(-1, -6), (11, -6), (5, -6)]:                                # 2^5 = 32 trials on max_blocks = 16
        with pytest.raises(q.QldpcError) as e:
            r.decode_guess(*few(idx), g)
        assert e.value.status == status, g
    assert "max_blocks" in str(e.value)                                            # the message names the remedy
    r8 = q.Recon(**dict(SESSION, max_blocks=8, schedule="flooding"))               # the edge-parallel engine
    with pytest.raises(q.QldpcError) as e:
        r8.decode_guess(*few(idx), 2)
    assert e.value.status == -7
    assert q._L.qldpc_recon_decode_guess(r._h, 1, None, None, None, None, None, 3, None, None, None, None) == -1
    # a block with a bad header is refused alone, its neighbours are decoded and guessed
    bob, kb, plan_q, msgs, pars = few(idx)
    bad = q.ReconMsg.from_buffer_copy(msgs[3])
    bad.code_m += 32
    msgs = list(msgs)
    msgs[3] = bad
    st, keys, co, it, gr = r.decode_guess(bob, kb, plan_q, msgs, pars, 3)
    ref = w["ref"][3]
    assert st[3] == -6 and (keys[3] == bob[3]).all() and tuple(as_rows(gr)[3]) == (0, -1, 0, 0, 0, 0) and co[3] == 0 and it[3] == 0
    rest = [t for t in range(len(idx)) if t != 3]
    assert [int(st[t]) for t in rest] == [int(ref[0][idx[t]]) for t in rest] and (as_rows(gr)[rest] == ref[4][[idx[t] for t in rest]]).all()
    assert gr["tried"][rest].any()
