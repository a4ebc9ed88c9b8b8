"""GPU suite: keyed universal-hash tags inside Bob's verify step (qldpc_recon_decode_blocks_tagged, _decode_guess_tagged, qldpc_recon_tag_blocks).

1. the verdict kernel (qldpc_recon_verify_tag_dev) against its host mirror on the synthetic batches of tests/recon_tag_ref.py, exactly;
2. Recon.tag_blocks against the polyhash context and polyhash_host;
3. the session call against decode_blocks, polyhash_host of the returned keys and Alice's tags from a second session (the two-party check);
4. invariance under shuffling, splitting, the engine and the number of keys;  5. decode_guess_tagged against decode_guess;  6. refusals.

The blocks of 3 - 5 are those of tests/test_recon_guess_gpu.py, whose generator is restated here: 48 blocks of 1 000 and 48 of 2 000 bits planned at QBER
0.03, true QBERs spread evenly over 1 .. 3 times it, seed 0.  That file records, pinned on an MI355X, that 77 of them decode at once, 2 are rescued at
g = 3 and at g = 4 and 17 stay failed, and that no rescue was a wrong key: both branches occur."""
import ctypes as C

import numpy as np
import pytest

import polyhash_ref as PR
import recon_tag_ref as T

pytestmark = pytest.mark.gpu

PLAN_Q, SPREAD, SEED, PER_LENGTH = 0.03, 3.0, 0, 48
SESSION = dict(max_blocks=16, mother_step=0, key_quantum=1024, rule="NMS", rule_param=0.75)
LENGTHS = [1, 33, 1000, 255 * 32 + 5, 256 * 32, 257 * 32 - 1, 65536, 1 << 18]


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


# ---------------------------------------------------------------- 1. the verdict kernel

def verify_both(q, torch, B):
    host = q.recon_verify_tag_host(B["out"], B["keys"], B["key_bits"], B["crc_want"], B["ok"], B["iters"], B["hash_keys"])
    got = q.recon_verify_tag(dev(torch, B["out"]), dev(torch, B["keys"]), dev(torch, B["key_bits"]), dev(torch, B["crc_want"]), dev(torch, B["ok"]),
                             dev(torch, B["iters"]), dev(torch, B["hash_keys"]))
    return got, host


@pytest.mark.parametrize("n", [1, 3, 17])
@pytest.mark.parametrize("r", [1, 2, 4])
def test_verify_kernel_equals_the_host_mirror(q, torch, n, r):
    rng = np.random.default_rng(100 * n + r)
    if n == 1:
        cases = [([b], ()) for b in LENGTHS] + [([1000], (0,))]
    elif n == 3:
        cases = [([b, max(1, b - 1), b], ()) for b in LENGTHS] + [([1 << 18, 33, 1000], (0,)), ([1000, 65, 257 * 32 - 1], (0,))]      # a failed block beside two others
    else:
        cases = [([LENGTHS[i % len(LENGTHS)] for i in range(n)], (3, 6, 15)), ([int(b) for b in rng.integers(1, 9000, n)], (0,))]      # mixed lengths in one launch
    for bits, collide in cases:
        for shared in (True, False):
            B = T.batch(q, rng, bits, r, shared, collide)
            got, host = verify_both(q, torch, B)
            T.check_verdict(got, host)
            for b in collide:                                                      # the CRC passes the wrong key, and the tag is not Alice's
                assert got["status"][b] == T.OK and (got["keys"][b, :len(T.masked(B["alice"][b], bits[b]))] != T.masked(B["alice"][b], bits[b])).any()
                hk = B["hash_keys"] if shared else B["hash_keys"][b]
                assert got["tags"][b].tolist() != PR.tags(B["alice"][b], bits[b], hk).tolist()
            bad = host["status"] != T.OK
            assert not got["tags"][bad].any() and got["tags"][~bad].any(axis=1).all()
            for b in np.flatnonzero(bad):                                          # a bad block keeps the key handed in, nothing is written past a key's words
                nw = (bits[b] + 31) // 32
                assert (got["keys"][b, :nw] == B["keys"][b, :nw]).all() and not got["keys"][b, nw:].any()
    if n == 3:
        small = T.batch(q, rng, [33, 1000, 64], r, True)
        T.check_verdict(verify_both(q, torch, small)[0], T.expected(q, small))      # ... and against the Python integers, once
        for hk in T.hash_keys(rng):                                                # the special hash keys: 0, 1, p (-> 0), p - 1, all ones
            B = T.batch(q, rng, [1, 1000, 257 * 32 - 1], r, True)
            B["hash_keys"] = np.tile(hk, r)
            got, host = verify_both(q, torch, B)
            T.check_verdict(got, host)
            assert got["tags"][0].tolist() == PR.tags(B["out"][0], 1, B["hash_keys"]).tolist()


# ---------------------------------------------------------------- 2. tag_blocks against the polyhash context

@pytest.mark.parametrize("r", [1, 3])
def test_tag_blocks_equals_the_polyhash_context(q, r):
    rng = np.random.default_rng(7 + r)
    bits = [1, 31, 32, 33, 1000, 255 * 32 + 5, 256 * 32, 257 * 32 - 1, 52429, 65536, 1 << 18] + [int(b) for b in rng.integers(1, 1 << 18, 29)]
    keys = [T.words(rng, (b + 31) // 32 + int(rng.integers(0, 3))) for b in bits]      # some rows carry words past the block
    s = q.Recon(**SESSION)                                                          # max_blocks = 16: three launches
    ph = q.PolyHash(max_blocks=64, max_key_bits=1 << 18, n_keys=r)
    shared = T.words(rng, 2 * r)
    per_block = T.words(rng, len(bits) * 2 * r).reshape(len(bits), 2 * r)
    for hk in (shared, per_block):
        tags = s.tag_blocks(keys, bits, hk)
        assert tags.shape == (len(bits), 2 * r) and tags.dtype == np.uint32
        want = ph.blocks(keys, bits, hk if hk.ndim == 1 else list(hk))
        assert (tags == np.stack(want)).all()
        for i in (0, 3, 7, 10, 20):
            row = hk if hk.ndim == 1 else hk[i]
            assert tags[i].tolist() == np.concatenate([q.polyhash_host(keys[i], bits[i], row[2 * k:2 * k + 2]) for k in range(r)]).tolist()
    assert (s.tag_blocks(keys[:1], bits[:1], shared) == s.tag_blocks(keys, bits, shared)[:1]).all()


# ---------------------------------------------------------------- 3. the session call

def blocks(q, seed=SEED, spread=SPREAD, per_length=PER_LENGTH):
    """-> Alice's keys, Bob's keys, key_bits, planned QBERs (the generator of tests/test_recon_guess_gpu.py)"""
    rng = np.random.default_rng(seed)
    alice, bob, kb = [], [], []
    for key_bits in (1000, 2000):
        for true_q in PLAN_Q * np.linspace(1.0, spread, per_length):
            a = rng.integers(0, 2, key_bits).astype(np.uint8)
            b = a ^ (rng.random(key_bits) < true_q)
            alice.append(q.pack_bits(a)); bob.append(q.pack_bits(b)); kb.append(key_bits)
    return alice, bob, kb, [PLAN_Q] * len(kb)


def host_tags(q, key, bits, hk):
    return np.concatenate([q.polyhash_host(key, bits, hk[2 * k:2 * k + 2]) for k in range(len(hk) // 2)])


@pytest.fixture(scope="module")
def world(q):
    alice, bob, kb, plan_q = blocks(q)
    r, ra = q.Recon(**SESSION), q.Recon(**SESSION)
    msgs, pars = ra.encode_blocks(alice, kb, plan_q)
    hk = T.words(np.random.default_rng(61), 4)                                      # two keys, shared by the blocks
    plain = r.decode_blocks(bob, kb, plan_q, msgs, pars)
    tagged = r.decode_blocks_tagged(bob, kb, plan_q, msgs, pars, hk)
    return dict(r=r, ra=ra, alice=alice, bob=bob, kb=kb, plan_q=plan_q, msgs=msgs, pars=pars, hk=hk, plain=plain, tagged=tagged,
                alice_tags=ra.tag_blocks(alice, kb, hk))


def same_decode(a, b):
    return (a[0] == b[0]).all() and all((x == y).all() for x, y in zip(a[1], b[1])) and (a[2] == b[2]).all() and (a[3] == b[3]).all()


def test_tagged_call_is_decode_blocks_with_the_tags_of_both_parties(q, world):
    w = world
    st, keys, co, it, tags = w["tagged"]
    assert same_decode(w["tagged"], w["plain"])                                    # block for block
    assert tags.shape == (len(st), 4) and tags.dtype == np.uint32
    ok = np.flatnonzero(st == 0)
    failed = np.flatnonzero(st != 0)
    assert len(ok) >= 4 and len(failed) >= 2 and set(st.tolist()) == {0, -9}
    for i in ok:
        assert tags[i].tolist() == host_tags(q, keys[i], w["kb"][i], w["hk"]).tolist() == w["alice_tags"][i].tolist()
    for i in failed:
        assert not tags[i].any() and (keys[i] == w["bob"][i]).all()


# ---------------------------------------------------------------- 4. invariance

def pick(w, idx):
    return ([w["bob"][i] for i in idx], [w["kb"][i] for i in idx], [w["plan_q"][i] for i in idx], [w["msgs"][i] for i in idx], [w["pars"][i] for i in idx])


def test_invariance(q, world):
    w = world
    r, n = w["r"], len(w["bob"])
    st0, keys0, co0, it0, tags0 = w["tagged"]
    perm = np.random.default_rng(5).permutation(n)
    per_block = T.words(np.random.default_rng(6), n * 4).reshape(n, 4)
    st, keys, co, it, tags = r.decode_blocks_tagged(*pick(w, perm), w["hk"])        # shuffled
    assert (st == st0[perm]).all() and (tags == tags0[perm]).all() and (co == co0[perm]).all() and all((keys[t] == keys0[i]).all() for t, i in enumerate(perm))
    st, keys, co, it, tags = r.decode_blocks_tagged(*pick(w, perm), per_block[perm])      # a key row per block
    assert (st == st0[perm]).all()
    for t, i in enumerate(perm):
        assert tags[t].tolist() == (host_tags(q, keys0[i], w["kb"][i], per_block[i]).tolist() if st0[i] == 0 else [0, 0, 0, 0])
    halves = [np.arange(0, 37), np.arange(37, n)]                                   # split into two calls
    got = [r.decode_blocks_tagged(*pick(w, h), w["hk"]) for h in halves]
    assert (np.concatenate([g[0] for g in got]) == st0).all() and (np.concatenate([g[4] for g in got]) == tags0).all()
    one = r.decode_blocks_tagged(*pick(w, np.arange(n)), w["hk"][:2])              # r = 1 against r = 2: key 0 of r = 2 gives r = 1's tag
    assert one[4].shape == (n, 2) and (one[4] == tags0[:, :2]).all() and (one[0] == st0).all()
    # max_blocks = 4 on the flooding schedule: the edge-parallel engine, whose decodes are its own; the tags follow the keys it returns
    sub = np.arange(0, n, 4)
    r4 = q.Recon(**dict(SESSION, max_blocks=4, schedule="flooding"))
    plain = r4.decode_blocks(*pick(w, sub))
    edge = r4.decode_blocks_tagged(*pick(w, sub), w["hk"])
    assert same_decode(edge, plain) and (edge[0] == 0).sum() >= 4
    for t, i in enumerate(sub):
        assert edge[4][t].tolist() == (host_tags(q, edge[1][t], w["kb"][i], w["hk"]).tolist() if edge[0][t] == 0 else [0, 0, 0, 0])
        if edge[0][t] == 0 and st0[i] == 0:
            assert (edge[4][t] == tags0[i]).all()                                  # both engines returned Alice's key


# ---------------------------------------------------------------- 5. guessing rounds

def test_decode_guess_tagged(q, world):
    w = world
    r, n = w["r"], len(w["bob"])
    every = pick(w, np.arange(n))
    st0, keys0, co0, it0, tags0 = w["tagged"]
    plain = r.decode_guess(*every, 3)
    st, keys, co, it, gr, tags = r.decode_guess_tagged(*every, 3, w["hk"])
    assert same_decode((st, keys, co, it), plain[:4]) and (gr == plain[4]).all()    # every field of decode_guess
    at_once, rescued, failed = np.flatnonzero(gr["tried"] == 0), np.flatnonzero((gr["tried"] == 1) & (st == 0)), np.flatnonzero(st != 0)
    assert len(rescued) >= 1 and len(failed) >= 2 and len(at_once) >= 4
    assert (st[at_once] == 0).all() and (tags[at_once] == tags0[at_once]).all()
    for i in rescued:                                                              # the tag of the winner's key, which is Alice's
        assert st0[i] != 0 and not tags0[i].any()
        assert tags[i].tolist() == host_tags(q, keys[i], w["kb"][i], w["hk"]).tolist() == w["alice_tags"][i].tolist()
    for i in failed:
        assert not tags[i].any() and (keys[i] == w["bob"][i]).all()
    per_block = T.words(np.random.default_rng(8), n * 2).reshape(n, 2)              # a key row per block, one key
    st1, keys1, _, _, gr1, tags1 = r.decode_guess_tagged(*every, 3, per_block)
    assert (st1 == st).all() and (gr1 == gr).all()
    for i in range(n):
        assert tags1[i].tolist() == (host_tags(q, keys1[i], w["kb"][i], per_block[i]).tolist() if st1[i] == 0 else [0, 0])
    zero = r.decode_guess_tagged(*every, 0, w["hk"])                               # g = 0 is decode_blocks_tagged
    assert same_decode(zero[:4], w["tagged"][:4]) and (zero[5] == tags0).all() and not zero[4]["tried"].any()


# ---------------------------------------------------------------- 6. refusals

def test_refusals(q, world):
    w = world
    r = w["r"]
    idx = list(range(40, 48))
    few = pick(w, idx)
    for hk in (np.zeros(0, np.uint32), np.zeros(10, np.uint32)):                   # n_keys of 0 and 5
        for call in (lambda: r.decode_blocks_tagged(*few, hk), lambda: r.decode_guess_tagged(*few, 3, hk), lambda: r.tag_blocks(few[0], few[1], hk)):
            with pytest.raises(q.QldpcError) as e:
                call()
            assert e.value.status == -1 and "n_keys" in str(e.value)
    # NULL rows: refused before anything is written, and the error names the block
    (kws, pars), kp, kb, qb, arr, pp = q._block_args(*few, True)
    n = len(kws)
    up, ip, fp = C.POINTER(C.c_uint32), C.POINTER(C.c_int), C.POINTER(C.c_float)
    hk, tags = np.ones(2, np.uint32), np.full((n, 2), 7, np.uint32)
    st, co, it = (np.full(n, 77, np.int32) for _ in range(3))
    out = (st.ctypes.data_as(ip), co.ctypes.data_as(ip), it.ctypes.data_as(ip))
    rows = lambda a, hole: (up * n)(*[None if i == hole else a[i if a.ndim == 2 else slice(None)].ctypes.data_as(up) for i in range(n)])
    guess = np.zeros(n, q.RECON_GUESS_DTYPE)
    head = (r._h, n, kp, kb.ctypes.data_as(ip), qb.ctypes.data_as(fp), arr, pp)
    for hp, tp, word in ((rows(hk, 5), rows(tags, -1), "hash-key"), (rows(hk, -1), rows(tags, 2), "tag")):
        for call in (lambda: q._L.qldpc_recon_decode_blocks_tagged(*head, 1, hp, tp, *out),
                     lambda: q._L.qldpc_recon_decode_guess_tagged(*head, 3, C.c_void_p(guess.ctypes.data), 1, hp, tp, *out),
                     lambda: q._L.qldpc_recon_tag_blocks(r._h, n, kp, kb.ctypes.data_as(ip), 1, hp, tp)):
            assert call() == -1
            msg = q._L.qldpc_last_error().decode()
            assert word in msg and ("block 5" if word == "hash-key" else "block 2") in msg
    assert (tags == 7).all() and (st == 77).all()
    assert q._L.qldpc_recon_decode_blocks_tagged(r._h, n, kp, kb.ctypes.data_as(ip), qb.ctypes.data_as(fp), arr, pp, 1, None, None, *out) == -1
    assert q._L.qldpc_recon_verify_tag_dev(1, 1, 1, 1, *([None] * 7), 0, None, None, None, None) == -1
    with pytest.raises(q.QldpcError) as e:                                         # a block past 2^18 bits
        r.tag_blocks([np.zeros(8193, np.uint32)], [(1 << 18) + 1], hk)
    assert e.value.status == -6
    # the refusals of decode_guess
    for g, status in [(-1, -6), (11, -6), (5, -6)]:                                # 2^5 = 32 trials on max_blocks = 16
        with pytest.raises(q.QldpcError) as e:
            r.decode_guess_tagged(*few, g, hk)
        assert e.value.status == status, g
    r8 = q.Recon(**dict(SESSION, max_blocks=8, schedule="flooding"))               # the edge-parallel engine
    with pytest.raises(q.QldpcError) as e:
        r8.decode_guess_tagged(*few, 2, hk)
    assert e.value.status == -7
    # a block with a bad header is refused alone: zeros for it, its neighbours are decoded and tagged
    bob, kbs, plan_q, msgs, parities = few
    bad = q.ReconMsg.from_buffer_copy(msgs[3])
    bad.code_m += 32
    msgs = list(msgs)
    msgs[3] = bad
    st, keys, co, it, tg = r.decode_blocks_tagged(bob, kbs, plan_q, msgs, parities, hk)
    assert st[3] == -6 and not tg[3].any() and (keys[3] == bob[3]).all()
    rest = [t for t in range(len(idx)) if t != 3]
    assert [int(st[t]) for t in rest] == [int(w["tagged"][0][idx[t]]) for t in rest]
    assert all(tg[t].tolist() == (host_tags(q, keys[t], kbs[t], hk).tolist() if st[t] == 0 else [0, 0]) for t in rest)
