"""GPU suite of SC-Flip trials in the polar reconciliation sessions: the select kernel against its mirror, the flip session (PolarRecon with
max_flips: decode_flip) against its mirror bit for bit in keys, status, corrected, flip_pos, decodes and n_tried, with several chunks of which the
last is partial, on a ladder at mixed counts, where two trials of a block pass a short CRC, with fewer flips than the session holds, resumed after
a plain decode, on a delayed side stream, its refusals, and the existing calls on a flip session against a ladder session."""
import numpy as np
import pytest

import polar_recon_ref as RR
import polar_ref as R
from stream_order import Chain, Delay, differ_in_every_frame
from test_polar_flip_host import FLIP_KEYS, mirror, select_inputs, session_case

pytestmark = pytest.mark.gpu

OK, EINVAL, ESIZE, EUNSUPPORTED, ESTATE, EDECODE = 0, -1, -6, -7, -8, -9
F = 130                            # two full waves and a partial one


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def dev(torch, a):
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def same(got, want, keys, what):
    """device tensors (or host arrays) against the mirror's arrays, bit for bit, and n_tried where both have it"""
    for k in keys:
        x, y = got[k], np.ascontiguousarray(want[k])
        x = np.ascontiguousarray(x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x, y.dtype))
        assert x.shape == y.shape and x.dtype.itemsize == y.dtype.itemsize and np.array_equal(x.view(np.uint8), y.view(np.uint8)), what + ": " + k
    if "n_tried" in got and "n_tried" in want:
        assert int(got["n_tried"]) == int(want["n_tried"]), what + ": n_tried"


def status(q, fn, *args, **kw):
    with pytest.raises(q.QldpcError) as e:
        fn(*args, **kw)
    assert str(e.value)
    return e.value.status


# ---- the select ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("messages", ["i8", "f32"])
@pytest.mark.parametrize("n", [1, 2, 5, 6, 8, 10, 12])
def test_select_device_is_the_mirror(q, torch, n, messages):
    """130 frames: random leaves, all-equal leaves, zeros and denormals, fewer candidates than flips, none, a ladder that removes candidates"""
    rng = np.random.default_rng([n, messages == "i8", 71])
    for name, leaf, frozen, rank, extra in select_inputs(rng, n, messages, F):
        mask = R.pack(frozen[None, :].astype(np.uint8))[0]
        for T in (1, 2, 8, 32):
            got = q.polar_flip_select(n, leaf, mask, T, rank, extra, messages)
            assert np.array_equal(got, q.polar_flip_select_host(n, leaf, mask, T, rank, extra, messages)), "%s n=%d T=%d %s" % (name, n, T, messages)


# ---- the session -----------------------------------------------------------------------------------------------------------------------------

_CASES = {}


def case(n, seed=0, qber=None, B=F, **kw):
    """130 blocks of a 5G code through a BSC whose rate leaves blocks of every kind at most sizes, key lengths mixed"""
    key = (n, seed, qber, B, tuple(sorted(kw.items())))
    if key not in _CASES:
        _CASES[key] = session_case(n, seed, (0.08 if n < 8 else 0.07) if qber is None else qber, B=B, kind=kw.pop("kind", "5g"), **kw)
    return _CASES[key]


def session(q, c, messages, max_flips, max_blocks=0, frames=F):
    dec = q.Polar(c["n"], c["pos"], messages, 31, max_frames=frames)
    return dec, q.PolarRecon(dec, *c["crc"], max_blocks=max_blocks, extra_pos=c["xp"] if len(c["xp"]) else None, max_flips=max_flips)


def device_flip(torch, sess, c, T, keys=None, **kw):
    d_keys = dev(torch, c["kbob"] if keys is None else keys)
    return sess.decode_flip(d_keys, dev(torch, c["syn"]), dev(torch, c["xcrc"]), n_flips=T, extra_bits=dev(torch, c["xb"]), extra=dev(torch, c["extra"]),
                            key_bits=dev(torch, c["kb"]), **kw)


@pytest.mark.parametrize("messages", ["i8", "f32"])
@pytest.mark.parametrize("T", [1, 8, 32])
@pytest.mark.parametrize("n", [1, 4, 5, 6, 7, 10])
def test_flip_session_is_its_mirror(q, torch, n, T, messages):
    """130 blocks, max_blocks = 130: chunks of 130, 16 and 4 blocks.  The call twice on one session: nothing of the first is left in the second"""
    c = case(n)
    dec, sess = session(q, c, messages, T)
    assert sess.max_flips == T
    size = sess.device_bytes()
    want = mirror(q, c, T, messages)
    what = "n=%d T=%d %s" % (n, T, messages)
    print("%s: tried %d, rescued %d" % (what, want["n_tried"], int((want["flip_pos"] >= 0).sum())))
    for k in range(2):
        same(device_flip(torch, sess, c, T), want, FLIP_KEYS, what + " call %d" % k)
    assert sess.device_bytes() == size


def test_several_chunks_and_a_partial_last_one(q, torch):
    """max_blocks = 16 and 8 flips: chunks of two blocks.  More than two blocks are open and their number is odd (asserted from the mirror; the
    seed is the first that gives it)"""
    for seed in range(50):
        c = case(6, seed=seed, qber=0.1, B=16)
        want = mirror(q, c, 8, "i8")
        if want["n_tried"] > 2 and want["n_tried"] % 2 == 1 and (want["flip_pos"] >= 0).any():
            break
    assert want["n_tried"] > 2 and want["n_tried"] % 2 == 1
    for messages in ("i8", "f32"):
        dec, sess = session(q, c, messages, 8, max_blocks=16)
        same(device_flip(torch, sess, c, 8), mirror(q, c, 8, messages), FLIP_KEYS, "chunks of 2, %s" % messages)


@pytest.mark.parametrize("messages", ["i8", "f32"])
def test_flips_on_a_ladder_at_mixed_counts(q, torch, messages):
    c = case(7, E=20)
    assert len(set(c["extra"].tolist())) > 3 and c["extra"].any()
    dec, sess = session(q, c, messages, 8)
    want = mirror(q, c, 8, messages)
    assert want["n_tried"] > 0
    same(device_flip(torch, sess, c, 8), want, FLIP_KEYS, "ladder %s" % messages)


def test_the_lowest_of_two_accepted_trials_wins(q, torch):
    """the case of the CPU suite (a 4-bit CRC, 32 flips, blocks with several accepted trials): a chunk is one block"""
    c = case(6, qber=0.12, B=36, crc=(4, 0x3), kind="random")
    dec, sess = session(q, c, "i8", 32, frames=36)
    same(device_flip(torch, sess, c, 32), mirror(q, c, 32, "i8"), FLIP_KEYS, "two accepted trials")


def test_fewer_flips_than_the_session_holds_and_resume_after_a_plain_decode(q, torch):
    c = case(7)
    dec, sess = session(q, c, "f32", 32)
    for T in (1, 4, 16):
        same(device_flip(torch, sess, c, T), mirror(q, c, T, "f32"), FLIP_KEYS, "n_flips=%d of 32" % T)
    # Bob's plain decode, then the flips on what it left
    d_keys, d_syn, d_crc, d_kb = dev(torch, c["kbob"]), dev(torch, c["syn"]), dev(torch, c["xcrc"]), dev(torch, c["kb"])
    plain = sess.decode(d_keys, d_syn, d_crc, d_kb)
    st = plain["status"].clone()
    got = sess.decode_flip(d_keys, d_syn, d_crc, n_flips=8, key_bits=d_kb, resume=True, status=st)
    assert got["status"] is st and got["keys"] is d_keys
    host_plain = q.polar_recon_decode_host(c["n"], c["pos"], c["kbob"], c["syn"], c["xcrc"], c["kb"], "f32", crc_len=c["crc"][0], crc_poly=c["crc"][1])
    want = mirror(q, c, 8, "f32", keys=host_plain["keys"], resume=True, status=host_plain["status"])
    same(got, want, FLIP_KEYS, "resume")
    whole = mirror(q, c, 8, "f32")
    same(got, whole, ("keys", "status", "flip_pos"), "resume against one call")
    assert want["n_tried"] > 0 and (want["flip_pos"] >= 0).any()


# ---- stream order ------------------------------------------------------------------------------------------------------------------------------

def stream_case(q):
    """n = 8, float messages, a CRC-32, 65 blocks of N bits, 8 flips.  In the true inputs the even blocks are Bob's without an error (OK at once:
    corrected 0, flip_pos -1, one decode) and the odd ones are blocks that a flip rescues (picked with the mirror from a pool through a BSC of
    5 %: corrected > 0, flip_pos >= 0, 10 decodes); in the decoy the other way round, around other keys: every block of corrected, flip_pos,
    decodes and keys differs.  The status is OK everywhere"""
    n, N, B, T = 8, 256, 65, 8
    rng = np.random.default_rng(811)
    pos = RR.code(rng, n, "5g")
    code = dict(messages="f32", crc_len=32, crc_poly=RR.CRC32[1])
    x = rng.integers(0, 2, (1500, N), dtype=np.uint8)
    y = x ^ (rng.random(x.shape) < 0.05).astype(np.uint8)
    syn, crc = q.polar_recon_encode_host(n, pos, R.pack(x), None, *RR.CRC32)
    pool = np.flatnonzero(q.polar_recon_decode_flip_host(n, pos, R.pack(y), syn, crc, n_flips=T, **code)["flip_pos"] >= 0)
    assert len(pool) >= B
    c = dict(n=n, pos=pos, T=T, inp={}, ref={})
    for which, phase in (("true", 0), ("decoy", 1)):
        clean = np.arange(B) % 2 == phase
        take, pool = pool[:int((~clean).sum())], pool[int((~clean).sum()):]
        xa = rng.integers(0, 2, (B, N), dtype=np.uint8)
        xb = xa.copy()
        xa[~clean], xb[~clean] = x[take], y[take]
        ka, kbob = R.pack(xa), R.pack(xb)
        syn, crc = q.polar_recon_encode_host(n, pos, ka, None, *RR.CRC32)
        out = q.polar_recon_decode_flip_host(n, pos, kbob, syn, crc, n_flips=T, **code)
        assert (out["status"] == OK).all() and np.array_equal(out["flip_pos"] < 0, clean) and np.array_equal(out["decodes"] == 1, clean), which
        c["inp"][which] = (ka, kbob)
        c["ref"][which] = dict(syndrome=syn, crc=crc, status=out["status"], corrected=out["corrected"], flip_pos=out["flip_pos"], decodes=out["decodes"], keys=out["keys"])
    differ_in_every_frame({k: v for k, v in c["ref"]["true"].items() if k != "status"}, {k: v for k, v in c["ref"]["decoy"].items() if k != "status"}, "polar flip")
    return c


def test_flip_session_on_a_side_stream(q, torch):
    """encode -> decode_flip on a delayed non-blocking side stream while the inputs still hold the decoy.  decode_flip waits for its stream once,
    so the host does not run ahead of the delay; what is shown is that every kernel, memset and read-back of the call is on the stream of the
    call, in order, and that the call waits for that stream and no other"""
    c = stream_case(q)
    delay, side = Delay(torch), torch.cuda.Stream()
    dec = q.Polar(c["n"], c["pos"], "f32", max_frames=65)
    sess = q.PolarRecon(dec, *RR.CRC32, max_flips=c["T"])
    ch = Chain(torch, delay, side, "polar flip", host_waits=True)
    (ta, tb), (da, db) = c["inp"]["true"], c["inp"]["decoy"]
    alice, bob = ch.input(ta, da), ch.input(tb, db)
    with torch.cuda.stream(side):                                 # driven on the decoy, on the side stream, whose allocations the chain then finds cached
        syn, crc = sess.encode(alice)
        warm = [t.clone() for t in (syn, crc, bob)]
        warm += [v.clone() for v in sess.decode_flip(bob.clone(), syn, crc, n_flips=c["T"]).values() if hasattr(v, "clone")]
    del warm, syn, crc
    with ch:
        ch.stage()
        syn, crc = sess.encode(alice)
        ch.keep("syndrome", syn)
        ch.keep("crc", crc)
        out = sess.decode_flip(bob, syn, crc, n_flips=c["T"])
        for k in ("status", "corrected", "flip_pos", "decodes"):
            ch.keep(k, out[k])
        ch.keep("keys", bob, in_place=True)
    assert out["n_tried"] == 32
    ch.check_all(c["ref"]["true"])


# ---- refusals, and the existing calls on a flip session ----------------------------------------------------------------------------------------------

def test_flip_refusals(q, torch):
    c = case(6)
    pos = c["pos"]
    make = lambda dec, **kw: q.PolarRecon(dec, *c["crc"], **kw)
    sc = q.Polar(6, pos, "i8", 31, max_frames=F)
    for kw in (dict(form="wide"), dict(rule="ssc")):
        assert status(q, make, q.Polar(6, pos, "i8", 31, max_frames=F, **kw), max_flips=8) == EUNSUPPORTED
    assert status(q, make, q.PolarList(6, pos, "i8", 31, 4, 11, 0x621, max_frames=F), max_flips=8) == EUNSUPPORTED
    for bad in (3, 12, 64, -1):
        assert status(q, make, sc, max_flips=bad) == EINVAL, bad
    assert status(q, make, sc, max_flips=16, max_blocks=8) == ESIZE and status(q, make, sc, max_flips=8, max_blocks=F + 1) == ESIZE
    assert status(q, make, sc, max_flips=8, extra_pos=[int(pos[0]), int(pos[0])]) == EINVAL
    plain, ladder, sess = make(sc), make(sc, extra_pos=pos[:4]), make(sc, max_flips=8, max_blocks=8)
    assert plain.max_flips == 0 and ladder.max_flips == 0 and sess.max_flips == 8 and sess.extra_words == 0 and sess.max_blocks == 8
    keys, kb, syn, crc = (dev(torch, c[k][:8]) for k in ("kbob", "kb", "syn", "xcrc"))
    before = keys.clone()
    for other in (plain, ladder):
        assert status(q, other.decode_flip, keys, syn, crc, key_bits=kb) == ESTATE
    assert "create_flip" in str(pytest.raises(q.QldpcError, plain.decode_flip, keys, syn, crc).value)
    for bad in (0, 3, 6, -8):
        assert status(q, sess.decode_flip, keys, syn, crc, n_flips=bad, key_bits=kb) == EINVAL, bad
    assert status(q, sess.decode_flip, keys, syn, crc, n_flips=16, key_bits=kb) == ESIZE
    assert status(q, sess.decode_flip, keys, syn, crc, resume=2, status=kb.clone()) == EINVAL
    assert status(q, sess.decode_flip, keys, syn, crc, resume=True) == EINVAL
    L, vp = q._L, lambda t: t.data_ptr()
    st, fp = torch.zeros(8, dtype=torch.int32, device="cuda"), torch.zeros(8, dtype=torch.int32, device="cuda")
    raw = lambda *p: L.qldpc_polar_recon_decode_flip(sess._h, 8, p[0], None, p[1], p[2], None, None, 8, 0, p[3], None, p[4], None, None)
    full = [vp(t) for t in (keys, syn, crc, st, fp)]
    for k in range(5):
        assert raw(*[None if j == k else a for j, a in enumerate(full)]) == EINVAL, k
    big = dev(torch, c["kbob"][:9])
    assert status(q, sess.decode_flip, big, dev(torch, c["syn"][:9]), dev(torch, c["xcrc"][:9])) == ESIZE
    torch.cuda.synchronize()
    assert torch.equal(keys, before) and not st.any() and not fp.any()      # a refused call has touched nothing
    empty = sess.decode_flip(keys[:0], syn[:0], crc[:0])
    assert empty["status"].numel() == 0 and empty["n_tried"] == 0
    # the select on its own
    leaf, mask = np.zeros((2, 64), np.int8), np.zeros(2, np.uint32)
    for bad in (0, 5, 48):
        assert status(q, q.polar_flip_select, 6, leaf, mask, bad) == EINVAL
    assert status(q, q.polar_flip_select, 6, leaf, mask, 64) == ESIZE
    assert status(q, q.polar_flip_select, 0, leaf[:, :1], mask[:1], 1) == ESIZE
    assert L.qldpc_polar_flip_select_dev(None, 6, 0, 2, None, None, None, None, 1, None) == EINVAL
    assert q.polar_flip_select(6, leaf[:0], mask, 4).shape == (0, 4)


@pytest.mark.parametrize("messages", ["i8", "f32"])
def test_existing_calls_on_a_flip_session_are_the_ladder_sessions(q, torch, messages):
    """after decode_flip has run: encode (with the extra row), decode and decode_rounds on a flip session against a ladder session of the same
    code, ladder and CRC"""
    c = case(7, E=20)
    dec, sess = session(q, c, messages, 8)
    ladder = q.PolarRecon(dec, *c["crc"], extra_pos=c["xp"])
    device_flip(torch, sess, c, 8)
    d_ka, d_kb = dev(torch, c["ka"]), dev(torch, c["kb"])
    a, b = sess.encode(d_ka, d_kb, want_extra=True), ladder.encode(d_ka, d_kb, want_extra=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and np.array_equal(a[2].cpu().numpy().view(np.uint32), c["xb"])
    outs = []
    for s in (sess, ladder):
        k1, k2, ex = dev(torch, c["kbob"]), dev(torch, c["kbob"]), dev(torch, c["extra"])
        plain = s.decode(k1, a[0], a[1], d_kb)
        rounds = s.decode_rounds(k2, a[0], a[1], a[2], ex, step=5, max_rounds=3, key_bits=d_kb)
        outs.append((k1, plain["status"], plain["corrected"], k2, ex, rounds["status"], rounds["corrected"], rounds["decodes"], rounds["open_per_round"]))
    for x, y in zip(*outs):
        assert torch.equal(x, y) if hasattr(x, "cpu") else x == y
    assert (outs[0][5] == OK).any() and sum(outs[0][8][1:]) > 0
