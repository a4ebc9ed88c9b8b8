"""GPU suite of incremental freezing in the polar subsystem: Polar.decode_rows against its host mirror bit for bit in all four outputs, against
Polar.decode with all-zero rows, and its refusals; the ladder session (PolarRecon with extra_pos: encode with want_extra, decode_rounds) against its
mirrors bit for bit, rounds in one call against single-round resume calls, a session reused for a smaller call, the two extreme calls, one
encode -> decode_rounds chain on a delayed side stream, and the refusals on the device."""
import numpy as np
import pytest

import polar_ladder_ref as LD
import polar_recon_ref as RR
import polar_ref as R
from stream_order import Chain, Delay, differ_in_every_frame
from test_polar_ladder_host import ROUND_KEYS, inputs, start_counts

pytestmark = pytest.mark.gpu

OK, EINVAL, ESIZE, EUNSUPPORTED, ESTATE, EDECODE = 0, -1, -6, -7, -8, -9
SIZES = (1, 2, 3, 4, 5, 6, 7, 10, 12)
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


def host(t):
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 and a.ndim == 2 else a


def same(got, want, keys, what):
    """device tensors (or host arrays) against the mirror's arrays, bit for bit"""
    for k in keys:
        x, y = got[k], np.ascontiguousarray(want[k])
        x = np.ascontiguousarray(x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x, y.dtype))
        assert x.shape == y.shape and x.dtype.itemsize == y.dtype.itemsize and np.array_equal(x.view(np.uint8), y.view(np.uint8)), what + ": " + k


def status(q, fn, *args, **kw):
    with pytest.raises(q.QldpcError) as e:
        fn(*args, **kw)
    assert str(e.value)
    return e.value.status


# ---- the rows decode -----------------------------------------------------------------------------------------------------------------------------

def rows_case(n, messages, frames=F):
    rng = np.random.default_rng([n, messages == "i8", 41])
    N, maxq = 1 << n, (1, 31, 126)[n % 3]
    pos = RR.code(rng, n, "random")
    llr = inputs(rng, messages, frames, N, maxq)
    fz = R.pack(rng.integers(0, 2, (frames, N), dtype=np.uint8))
    bits = (rng.random((frames, N)) < rng.random((frames, 1))).astype(np.uint8)      # every frame a density, and so a rate, of its own
    bits[0], bits[-1] = 0, 1
    return pos, maxq, llr, fz, R.pack(bits)


@pytest.mark.parametrize("messages", ["i8", "f32"])
@pytest.mark.parametrize("n", SIZES)
def test_rows_device_is_the_mirror(q, torch, n, messages):
    """130 frames, every frame a frozen set of its own, with and without frozen values: all four outputs together, then each alone on 65 frames"""
    pos, maxq, llr, fz, rows = rows_case(n, messages)
    dec = q.Polar(n, pos, messages, maxq, max_frames=F)
    d_llr, d_fz, d_rows = dev(torch, llr), dev(torch, fz), dev(torch, rows)
    for values, d_values in ((fz, d_fz), (None, None)):
        want = q.polar_decode_rows_host(n, pos, llr, rows, values, messages, maxq, leaf=True)
        same(dec.decode_rows(d_llr, d_rows, d_values, leaf=True), want, ("u", "info", "x", "leaf"), "n=%d %s" % (n, messages))
    for name in ("u", "info", "x", "leaf"):
        out = dec.decode_rows(d_llr[:65], d_rows[:65], None, leaf=name == "leaf", want=() if name == "leaf" else (name,))
        assert set(out) == {name}
        same(out, {name: want[name][:65]}, (name,), "n=%d %s alone" % (n, messages))


@pytest.mark.parametrize("messages", ["i8", "f32"])
def test_rows_device_above_a_tile(q, torch, messages):
    """n = 16, 3 frames: the levels above a tile of the scratch, a wave of three lanes"""
    n = 16
    pos, maxq, llr, fz, rows = rows_case(n, messages, 3)
    out = q.Polar(n, pos, messages, maxq, max_frames=3).decode_rows(dev(torch, llr), dev(torch, rows), dev(torch, fz), leaf=True)
    same(out, q.polar_decode_rows_host(n, pos, llr, rows, fz, messages, maxq, leaf=True), ("u", "info", "x", "leaf"), "n=16 %s" % messages)


@pytest.mark.parametrize("messages", ["i8", "f32"])
@pytest.mark.parametrize("n", [3, 5, 6, 10])
def test_zero_rows_are_the_plain_decode(q, torch, n, messages):
    pos, maxq, llr, fz, rows = rows_case(n, messages)
    dec = q.Polar(n, pos, messages, maxq, max_frames=F)
    d_llr, d_fz = dev(torch, llr), dev(torch, fz)
    plain = {k: v.cpu().numpy() for k, v in dec.decode(d_llr, d_fz, leaf=True).items()}
    same(dec.decode_rows(d_llr, torch.zeros_like(d_fz), d_fz, leaf=True), plain, ("u", "info", "x", "leaf"), "n=%d %s" % (n, messages))


def test_rows_refusals(q, torch):
    n, pos = 6, [5, 9, 40]
    llr, rows = torch.zeros((4, 64), dtype=torch.int8, device="cuda"), torch.zeros((4, 2), dtype=torch.int32, device="cuda")
    for kw in (dict(form="wide"), dict(rule="ssc")):
        dec = q.Polar(n, pos, "i8", 31, max_frames=4, **kw)
        with pytest.raises(q.QldpcError) as e:
            dec.decode_rows(llr, rows)
        assert e.value.status == EUNSUPPORTED and ("QLDPC_POLAR_LANES" if "form" in kw else "QLDPC_POLAR_SC") in str(e.value)
        assert dec.decode(llr)["u"].shape == (4, 2)                # the context still serves its own call
    assert "plan" in str(pytest.raises(q.QldpcError, q.Polar(n, pos, "i8", 31, max_frames=4, rule="ssc").decode_rows, llr, rows).value)
    dec = q.Polar(n, pos, "i8", 31, max_frames=3)
    assert status(q, dec.decode_rows, llr, rows) == ESIZE
    assert status(q, dec.decode_rows, llr[:3], None) == EINVAL
    assert dec.decode_rows(llr[:0], rows[:0])["u"].shape == (0, 2)
    assert q.Polar(4, [3], "i8", 31, max_frames=4, form="wide").decode_rows(llr[:, :16].contiguous(), rows[:, :1].contiguous())["u"].shape == (4, 1)


# ---- the ladder session ----------------------------------------------------------------------------------------------------------------------------

_CASES = {}


def case(q, n, E_kind):
    """the code, a ladder of 0, 33 or K entries (at most K), 130 blocks with the key lengths N, N - 1, N - 37 and 1 in turn against clean, 2 % and
    25 % blocks, one length invalid, and Alice's three rows from the mirror"""
    if (n, E_kind) not in _CASES:
        rng = np.random.default_rng([n, ["zero", "mid", "all"].index(E_kind), 42])
        pos = RR.code(rng, n, "5g")
        K = len(pos)
        E = min(K, dict(zero=0, mid=33, all=K)[E_kind])
        xp = LD.ladder(rng, pos, E)
        crc_len, crc_poly = RR.crcs(K)[-1]
        ka, kbob, kb = RR.blocks(rng, n, F)
        kb[7] = 0
        syn, crc, xb = q.polar_recon_encode_ladder_host(n, pos, xp, ka, kb, crc_len, crc_poly)
        _CASES[(n, E_kind)] = dict(pos=pos, xp=xp, E=E, ka=ka, kbob=kbob, kb=kb, crc=(crc_len, crc_poly), syn=syn, xcrc=crc, xb=xb, extra=start_counts(rng, F, E))
    return _CASES[(n, E_kind)]


def session(q, c, n, messages, max_blocks=0):
    dec = q.Polar(n, c["pos"], messages, 31, max_frames=F)
    return dec, q.PolarRecon(dec, *c["crc"], max_blocks=max_blocks, extra_pos=c["xp"])


def mirror_rounds(q, c, n, messages, keys, extra, sl=slice(None), **kw):
    return q.polar_recon_decode_rounds_host(n, c["pos"], c["xp"], keys, c["syn"][sl], c["xcrc"][sl], c["xb"][sl], extra, key_bits=c["kb"][sl], messages=messages,
                                            crc_len=c["crc"][0], crc_poly=c["crc"][1], **kw)


def device_rounds(torch, sess, c, keys, extra, sl=slice(None), **kw):
    """-> the call's dict plus keys and extra, which it rewrote in place"""
    d_keys, d_extra = dev(torch, keys), dev(torch, extra)
    out = sess.decode_rounds(d_keys, dev(torch, c["syn"][sl]), dev(torch, c["xcrc"][sl]), dev(torch, c["xb"][sl]), d_extra, key_bits=dev(torch, c["kb"][sl]), **kw)
    out.update(keys=host(d_keys), extra=d_extra)
    return out


@pytest.mark.parametrize("messages", ["i8", "f32"])
@pytest.mark.parametrize("E_kind", ["zero", "mid", "all"])
@pytest.mark.parametrize("n", SIZES)
def test_ladder_session_is_its_mirrors(q, torch, n, E_kind, messages):
    """Alice's three rows; three rounds in one call from mixed start counts (one invalid) over mixed key lengths (one invalid); the same as three
    single-round calls with resume, the extra raised on the device between them; then a smaller call on the same session"""
    c = case(q, n, E_kind)
    E, step = c["E"], 7
    dec, sess = session(q, c, n, messages)
    assert sess.extra_words == (E + 31) // 32 and sess.leaked_bits == (1 << n) - len(c["pos"]) + c["crc"][0]
    size = sess.device_bytes()
    syn, crc, xb = sess.encode(dev(torch, c["ka"]), dev(torch, c["kb"]), want_extra=True)
    same(dict(syn=syn, crc=crc, xb=xb), dict(syn=c["syn"].view(np.int32), crc=c["xcrc"], xb=c["xb"].view(np.int32)), ("syn", "crc", "xb"), "alice n=%d E=%d" % (n, E))
    plain = sess.encode(dev(torch, c["ka"]), dev(torch, c["kb"]))
    assert torch.equal(plain[0], syn) and torch.equal(plain[1], crc)
    what = "n=%d E=%d %s" % (n, E, messages)
    whole = device_rounds(torch, sess, c, c["kbob"], c["extra"], step=step, max_rounds=3)
    same(whole, mirror_rounds(q, c, n, messages, c["kbob"], c["extra"], step=step, max_rounds=3), ROUND_KEYS, what)
    # three single-round calls
    got = device_rounds(torch, sess, c, c["kbob"], c["extra"], step=step, max_rounds=1)
    want = mirror_rounds(q, c, n, messages, c["kbob"], c["extra"], step=step, max_rounds=1)
    same(got, want, ROUND_KEYS, what + " call 1")
    for k in (2, 3):
        st, ex = got["status"], got["extra"]
        raised = torch.where((st == EDECODE) & (ex < E), torch.clamp(ex + step, max=E), ex).to(torch.int32)
        w_raised = np.where((want["status"] == EDECODE) & (want["extra"] < E), np.minimum(E, want["extra"] + step), want["extra"]).astype(np.int32)
        d_keys = dev(torch, got["keys"])
        out = sess.decode_rounds(d_keys, dev(torch, c["syn"]), dev(torch, c["xcrc"]), dev(torch, c["xb"]), raised, step=step, max_rounds=1, key_bits=dev(torch, c["kb"]),
                                 resume=True, status=st)
        assert out["status"] is st
        out.update(keys=host(d_keys), extra=raised)
        got = out
        want = mirror_rounds(q, c, n, messages, want["keys"], w_raised, step=step, max_rounds=1, resume=True, status=want["status"])
        same(got, want, ROUND_KEYS, what + " call %d" % k)
    same(got, dict(keys=whole["keys"], status=whole["status"].cpu().numpy(), extra=whole["extra"].cpu().numpy()), ("keys", "status", "extra"), what + " three calls against one")
    # a smaller call after the larger ones, on other blocks
    sl = slice(60, 100)
    small = device_rounds(torch, sess, c, c["kbob"][sl], c["extra"][sl], sl, step=step, max_rounds=3)
    same(small, mirror_rounds(q, c, n, messages, c["kbob"][sl], c["extra"][sl], sl, step=step, max_rounds=3), ROUND_KEYS, what + " smaller call")
    assert sess.device_bytes() == size
    if E == 0:                                                      # every new call as its plain counterpart
        d_keys = dev(torch, c["kbob"])
        plain = sess.decode(d_keys, dev(torch, c["syn"]), dev(torch, c["xcrc"]), dev(torch, c["kb"]))
        zero = device_rounds(torch, sess, c, c["kbob"], np.zeros(F, np.int32), step=1, max_rounds=3)
        same(zero, dict(status=plain["status"].cpu().numpy(), corrected=plain["corrected"].cpu().numpy(), keys=host(d_keys)), ("status", "corrected", "keys"), what)
        assert zero["open_per_round"] == [F - 1, 0, 0]


@pytest.mark.parametrize("n", [7, 10])
def test_the_two_extreme_calls(q, torch, n):
    """130 blocks of N bits.  Bob holds Alice's keys: round 0 leaves nothing open.  Bob holds noise: every block stays open to the last round"""
    c = case(q, n, "mid")
    dec, sess = session(q, c, n, "f32")
    rng = np.random.default_rng([n, 43])
    ka = rng.integers(0, 1 << 32, c["ka"].shape, dtype=np.uint64).astype(np.uint32)
    syn, crc, xb = q.polar_recon_encode_ladder_host(n, c["pos"], c["xp"], ka, None, *c["crc"])
    d_syn, d_crc, d_xb = dev(torch, syn), dev(torch, crc), dev(torch, xb)
    for which, keys, rounds in (("clean", ka, [F, 0, 0, 0]), ("noise", rng.integers(0, 1 << 32, ka.shape, dtype=np.uint64).astype(np.uint32), [F] * 4)):
        d_keys, d_extra = dev(torch, keys), torch.zeros(F, dtype=torch.int32, device="cuda")
        got = sess.decode_rounds(d_keys, d_syn, d_crc, d_xb, d_extra, step=5, max_rounds=4)
        got.update(keys=host(d_keys), extra=d_extra)
        want = q.polar_recon_decode_rounds_host(n, c["pos"], c["xp"], keys, syn, crc, xb, np.zeros(F, np.int32), 5, 4, messages="f32", crc_len=c["crc"][0], crc_poly=c["crc"][1])
        same(got, want, ROUND_KEYS, which)
        assert got["open_per_round"] == rounds, which
        assert (d_extra.cpu().numpy() == (0 if which == "clean" else 15)).all() and (got["decodes"].cpu().numpy() == (1 if which == "clean" else 4)).all()


# ---- stream order ------------------------------------------------------------------------------------------------------------------------------

def stream_case(q):
    """n = 8, float messages, 32 CRC bits, a ladder of 16, 65 blocks of N bits, step 16, 2 rounds.  In the true inputs the even blocks hold one flip
    (OK in round 0: extra 0, one decode) and the odd ones 25 % flips (failed twice: extra 16, two decodes), in the decoy the other way round, around
    different keys: every block of every output differs"""
    n, N, B = 8, 256, 65
    rng = np.random.default_rng(809)
    pos = RR.code(rng, n, "5g")
    c = dict(n=n, pos=pos, xp=pos[:16].copy(), inp={}, ref={})
    for which, phase in (("true", 0), ("decoy", 1)):
        x = rng.integers(0, 2, (B, N), dtype=np.uint8)
        e = (rng.random((B, N)) < 0.25).astype(np.uint8)
        light = np.arange(B) % 2 == phase
        e[light] = 0
        e[light, rng.integers(0, N, int(light.sum()))] = 1
        ka, kbob = R.pack(x), R.pack(x ^ e)
        syn, crc, xb = q.polar_recon_encode_ladder_host(n, pos, c["xp"], ka, None, *RR.CRC32)
        out = q.polar_recon_decode_rounds_host(n, pos, c["xp"], kbob, syn, crc, xb, np.zeros(B, np.int32), 16, 2, messages="f32", crc_len=32, crc_poly=RR.CRC32[1])
        assert np.array_equal(out["status"] == OK, light) and np.array_equal(out["decodes"] == 1, light), which
        c["inp"][which] = (ka, kbob)
        c["ref"][which] = dict(syndrome=syn, crc=crc, extra_bits=xb, status=out["status"], corrected=out["corrected"], keys=out["keys"], extra=out["extra"],
                               decodes=out["decodes"])
    differ_in_every_frame(c["ref"]["true"], c["ref"]["decoy"], "polar ladder")
    return c


def test_ladder_session_on_a_side_stream(q, torch):
    """encode (with the extra row) -> decode_rounds on a delayed non-blocking side stream while the inputs still hold the decoy.  decode_rounds
    waits for its stream once a round, so the host does not run ahead of the delay; what is shown is that every kernel, memset and read-back of
    the rounds is on the stream of the call, in order, and that the call waits for that stream and no other"""
    c = stream_case(q)
    delay, side = Delay(torch), torch.cuda.Stream()
    dec = q.Polar(c["n"], c["pos"], "f32", max_frames=65)
    sess = q.PolarRecon(dec, *RR.CRC32, extra_pos=c["xp"])
    ch = Chain(torch, delay, side, "polar ladder", host_waits=True)
    (ta, tb), (da, db) = c["inp"]["true"], c["inp"]["decoy"]
    alice, bob = ch.input(ta, da), ch.input(tb, db)
    with torch.cuda.stream(side):                                 # driven on the decoy, on the side stream, whose allocations the chain then finds cached
        syn, crc, xb = sess.encode(alice, want_extra=True)
        extra = torch.zeros(65, dtype=torch.int32, device="cuda")
        warm = [t.clone() for t in (syn, crc, xb, bob, extra)]
        warm += [v.clone() for v in sess.decode_rounds(bob.clone(), syn, crc, xb, extra, step=16, max_rounds=2).values() if hasattr(v, "clone")]
    del warm, syn, crc, xb, extra
    with ch:
        ch.stage()
        syn, crc, xb = sess.encode(alice, want_extra=True)
        ch.keep("syndrome", syn)
        ch.keep("crc", crc)
        ch.keep("extra_bits", xb)
        extra = torch.zeros(65, dtype=torch.int32, device="cuda")
        out = sess.decode_rounds(bob, syn, crc, xb, extra, step=16, max_rounds=2)
        ch.keep("status", out["status"])
        ch.keep("corrected", out["corrected"])
        ch.keep("decodes", out["decodes"])
        ch.keep("extra", extra)
        ch.keep("keys", bob, in_place=True)
    assert out["open_per_round"] == [65, 32]
    ch.check_all(c["ref"]["true"])


# ---- refusals on the device ----------------------------------------------------------------------------------------------------------------------

def test_ladder_refusals(q, torch):
    n = 6
    c = case(q, n, "mid")
    pos, xp = c["pos"], c["xp"]
    frozen = np.setdiff1d(np.arange(64), pos)
    make = lambda dec, extra_pos, **kw: q.PolarRecon(dec, *c["crc"], extra_pos=extra_pos, **kw)
    sc = q.Polar(n, pos, "i8", 31, max_frames=F)
    for kw in (dict(form="wide"), dict(rule="ssc")):
        assert status(q, make, q.Polar(n, pos, "i8", 31, max_frames=F, **kw), xp) == EUNSUPPORTED
    assert "plan" in str(pytest.raises(q.QldpcError, make, q.Polar(n, pos, "i8", 31, max_frames=F, rule="ssc"), xp).value)
    assert status(q, make, q.PolarList(n, pos, "i8", 31, 4, 11, 0x621, max_frames=F), xp) == EUNSUPPORTED
    assert status(q, make, sc, np.concatenate([pos, pos[:1]])) == ESIZE
    assert status(q, make, sc, [pos[0], pos[1], pos[0]]) == EINVAL
    assert status(q, make, sc, [int(frozen[0])]) == EINVAL and status(q, make, sc, [64]) == EINVAL
    assert status(q, make, sc, xp, max_blocks=F + 1) == ESIZE and status(q, q.PolarRecon, sc, 0, 0, extra_pos=xp) == ESIZE
    plain, sess = q.PolarRecon(sc, *c["crc"]), make(sc, xp, max_blocks=8)
    assert plain.extra_words == 0 and sess.extra_words == 2 and sess.max_blocks == 8
    keys, kb = dev(torch, c["kbob"][:8]), dev(torch, c["kb"][:8])
    syn, crc, xb, extra = (dev(torch, c[k][:8]) for k in ("syn", "xcrc", "xb", "extra"))
    assert status(q, plain.encode, keys, kb, want_extra=True) == ESTATE
    assert status(q, plain.decode_rounds, keys, syn, crc, None, extra) == ESTATE and "create_ladder" in str(pytest.raises(q.QldpcError, plain.decode_rounds, keys, syn, crc, None, extra).value)
    before = (keys.clone(), extra.clone())
    assert status(q, sess.decode_rounds, keys, syn, crc, xb, extra, step=0) == EINVAL
    assert status(q, sess.decode_rounds, keys, syn, crc, xb, extra, max_rounds=0) == EINVAL
    assert status(q, sess.decode_rounds, keys, syn, crc, xb, extra, resume=2, status=extra.clone()) == EINVAL
    assert status(q, sess.decode_rounds, keys, syn, crc, xb, extra, resume=True) == EINVAL
    L, vp = q._L, lambda t: t.data_ptr()
    raw = lambda *p: L.qldpc_polar_recon_decode_rounds(sess._h, 8, p[0], None, p[1], p[2], p[3], p[4], 1, 1, 0, p[5], None, None, None)
    st = torch.zeros(8, dtype=torch.int32, device="cuda")
    full = [vp(t) for t in (keys, syn, crc, xb, extra, st)]
    for k in range(6):
        assert raw(*[None if j == k else a for j, a in enumerate(full)]) == EINVAL, k
    assert L.qldpc_polar_recon_encode_ladder_dev(sess._h, 8, full[0], None, full[1], full[2], None) == EINVAL
    big = dev(torch, c["kbob"][:9])
    assert status(q, sess.decode_rounds, big, dev(torch, c["syn"][:9]), dev(torch, c["xcrc"][:9]), dev(torch, c["xb"][:9]), dev(torch, c["extra"][:9])) == ESIZE
    assert status(q, sess.encode, big, None, want_extra=True) == ESIZE
    torch.cuda.synchronize()
    assert torch.equal(keys, before[0]) and torch.equal(extra, before[1])      # a refused call has touched nothing
    empty = sess.decode_rounds(keys[:0], syn[:0], crc[:0], xb[:0], extra[:0], max_rounds=2)
    assert empty["status"].numel() == 0 and empty["open_per_round"] == [0, 0]
    assert [t.shape[0] for t in sess.encode(keys[:0], want_extra=True)] == [0, 0, 0]
