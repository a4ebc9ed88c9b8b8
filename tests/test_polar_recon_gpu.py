"""GPU suite of the polar reconciliation sessions: PolarRecon around every kind of context against the host mirrors bit for bit (syndrome, crc,
status, corrected, pick and the keys), the prior and verdict kernels on their own against their mirrors and on the constructed branch rows of the
CPU suite, a session reused with fewer and other blocks, device_bytes over calls, and one encode -> decode chain on a delayed side stream."""
import numpy as np
import pytest

import polar_recon_ref as RR
import polar_ref as R
from stream_order import Chain, Delay, differ_in_every_frame
from test_polar_recon_host import VERDICT_CASES, check_verdict, decoders, mirror_decode

pytestmark = pytest.mark.gpu

OK, EINVAL, ESIZE, EDECODE = 0, -1, -6, -9
B_MAX = 130
CRC_OF = {1: (1, 1), 2: (1, 1), 3: (1, 1), 4: (1, 1), 5: (1, 1), 6: (11, 0x621), 7: RR.CRC32, 10: (11, 0x621), 12: RR.CRC32}
SESSIONS = [(n, d) for n in (5, 6, 7, 10, 12) for d in decoders(n)] + [(n, d) for n in (1, 2, 3, 4) for d in ("sc", 4)]


@pytest.fixture(scope="module")
def torch():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return torch


def dev(torch, a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def host(t):
    a = t.cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.int32 and a.ndim == 2 else a


_CASES = {}


def case(q, n):
    """the code, the blocks and Alice's message of a size, shared by every session test of the size: 130 blocks, the key lengths N, N - 1, N - 37
    and 1 in turn against clean, 2 % and 25 % blocks"""
    if n not in _CASES:
        rng = np.random.default_rng([n, 77])
        pos = RR.code(rng, n, "5g")
        ka, kbob, kb = RR.blocks(rng, n, B_MAX)
        crc_len, crc_poly = CRC_OF[n]
        syn, crc = q.polar_recon_encode_host(n, pos, ka, kb, crc_len, crc_poly)
        _CASES[n] = dict(pos=pos, ka=ka, kbob=kbob, kb=kb, crc_len=crc_len, crc_poly=crc_poly, syn=syn, crc=crc, mirror={})
    return _CASES[n]


def mirror_of(q, n, messages, decoder):
    c = case(q, n)
    key = (messages, decoder)
    if key not in c["mirror"]:
        c["mirror"][key] = mirror_decode(q, n, c["pos"], c["kbob"], c["syn"], c["crc"], c["kb"], messages, 31, decoder, c["crc_len"], c["crc_poly"])
    return c["mirror"][key]


def context(q, n, pos, messages, decoder, crc_len, crc_poly):
    if isinstance(decoder, int):
        return q.PolarList(n, pos, messages, 31, decoder, crc_len, crc_poly, max_frames=B_MAX), {}
    form, rule = dict(sc=("lanes", "sc"), ssc=("lanes", "ssc"), wide=("wide", "sc"))[decoder]
    return q.Polar(n, pos, messages, 31, max_frames=B_MAX, form=form, rule=rule), dict(crc_len=crc_len, crc_poly=crc_poly)


@pytest.mark.parametrize("messages", ["i8", "f32"])
@pytest.mark.parametrize("n,decoder", SESSIONS)
def test_session_is_the_mirror(q, torch, n, decoder, messages):
    """encode, then decode of 130 blocks, of the last 70 and of the last one on the same session: every output is the mirror's, a shorter call on
    other blocks leaves no trace of the longer one, and device_bytes does not move"""
    c = case(q, n)
    want = mirror_of(q, n, messages, decoder)
    ok = want["status"] == OK
    # on the mirror's output: neither branch goes untested (below n = 5 a list of 4 paths always holds one that matches a CRC bit)
    assert ok.any() and ((want["status"] == EDECODE).any() or n < 5), "the case must hold an accepted and a refused block"
    dec, crc_args = context(q, n, c["pos"], messages, decoder, c["crc_len"], c["crc_poly"])
    sess = q.PolarRecon(dec, max_blocks=B_MAX, **crc_args)
    assert sess.syndrome_words == c["syn"].shape[1] and sess.leaked_bits == (1 << n) - len(c["pos"]) + c["crc_len"]
    size = sess.device_bytes()
    esz = 1 if messages == "i8" else 4
    assert size >= B_MAX * (esz << n) and dec.device_bytes() > 0
    is_list = isinstance(decoder, int)
    for lo in (0, 60, 129):
        sl = slice(lo, B_MAX)
        syn, crc = sess.encode(dev(torch, c["ka"][sl]), dev(torch, c["kb"][sl]))
        assert np.array_equal(host(syn).reshape(B_MAX - lo, -1), c["syn"][sl]) and np.array_equal(host(crc).view(np.uint32), c["crc"][sl]), (n, decoder, lo)
        keys = dev(torch, c["kbob"][sl])
        out = sess.decode(keys, syn, crc, dev(torch, c["kb"][sl]), want_pick=is_list)
        for k in ("status", "corrected") + (("pick",) if is_list else ()):
            assert np.array_equal(host(out[k]), want[k][sl]), (n, decoder, messages, lo, k)
        assert np.array_equal(host(keys), want["keys"][sl]), (n, decoder, messages, lo)
        assert sess.device_bytes() == size
    # no key_bits row: every block is N bits
    syn, crc = sess.encode(dev(torch, c["ka"][:9]))
    syn_h, crc_h = q.polar_recon_encode_host(n, c["pos"], c["ka"][:9], None, c["crc_len"], c["crc_poly"])
    assert np.array_equal(host(syn).reshape(9, -1), syn_h) and np.array_equal(host(crc).view(np.uint32), crc_h)
    keys = dev(torch, c["kbob"][:9])
    out = sess.decode(keys, syn, crc, want_pick=is_list)
    ref = mirror_decode(q, n, c["pos"], c["kbob"][:9], syn_h, crc_h, None, messages, 31, decoder, c["crc_len"], c["crc_poly"])
    assert all(np.array_equal(host(out[k]), ref[k]) for k in out) and np.array_equal(host(keys), ref["keys"])


@pytest.mark.parametrize("messages", ["i8", "f32"])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 10, 12])
def test_prior_kernel_is_its_mirror(q, torch, n, messages):
    """the LLR rows (by their bits) and the frozen rows; with a block whose key_bits is out of range, and with levels of the caller's"""
    c = case(q, n)
    kb = c["kb"].copy()
    kb[3], kb[4] = 0, (1 << n) + 1
    for levels in ((None, None), ((2, 9) if messages == "i8" else (0.5, 1e30))):
        llr, frozen = q.polar_recon_prior(n, c["pos"], c["kbob"], c["syn"], kb, messages, 31, *levels)
        llr_h, frozen_h = q.polar_recon_prior_host(n, c["pos"], c["kbob"], c["syn"], kb, messages, 31, *levels)
        assert llr.dtype == llr_h.dtype and np.array_equal(llr.view(np.uint8), llr_h.view(np.uint8)) and np.array_equal(frozen, frozen_h), (n, messages, levels)
    full = np.arange(1 << n, dtype=np.int32)                      # K = N: no syndrome at all
    llr, frozen = q.polar_recon_prior(n, full, c["kbob"], np.zeros((B_MAX, 0), np.uint32), kb, messages, 31)
    llr_h, frozen_h = q.polar_recon_prior_host(n, full, c["kbob"], np.zeros((B_MAX, 0), np.uint32), kb, messages, 31)
    assert np.array_equal(llr.view(np.uint8), llr_h.view(np.uint8)) and not frozen.any() and not frozen_h.any()


def test_prior_kernel_past_2_31_positions(q, torch):
    """2^21 + 3 blocks of N = 1 024 in int8: the LLR rows pass 2^31 bytes, and the last rows, rows on both sides of that mark and the first are the
    mirror's.  Every block is the same few key rows in turn, so the host holds 64 of them"""
    n, N, W, B = 10, 1024, 32, (1 << 21) + 3
    c = case(q, n)
    keys = dev(torch, c["kbob"][:64]).repeat((B + 63) // 64, 1)[:B].contiguous()
    syn = dev(torch, c["syn"][:64]).repeat((B + 63) // 64, 1)[:B].contiguous()
    kb = dev(torch, c["kb"][:64]).repeat((B + 63) // 64)[:B].contiguous()
    mask, prefix, _ = q.polar_recon_tables(n, c["pos"])
    d_mask, d_prefix = dev(torch, mask), dev(torch, prefix)
    llr = torch.zeros((B, N), dtype=torch.int8, device="cuda")
    frozen = torch.zeros((B, W), dtype=torch.int32, device="cuda")
    p = lambda t: q._vp(t.data_ptr())
    q._chk(q._L.qldpc_polar_recon_prior_dev(q._stream_arg(None, 0), n, N - len(c["pos"]), p(d_mask), p(d_prefix), 0, 31, 1.0, 31.0, B, p(keys), p(kb), p(syn), p(llr),
                                            p(frozen)), "prior")
    llr_h, frozen_h = q.polar_recon_prior_host(n, c["pos"], c["kbob"][:64], c["syn"][:64], c["kb"][:64], "i8", 31)
    rows = np.array([0, 1, (1 << 21) - 2, (1 << 21) - 1, 1 << 21, B - 2, B - 1])
    idx = torch.from_numpy(rows).cuda()
    assert np.array_equal(llr[idx].cpu().numpy(), llr_h[rows % 64]) and np.array_equal(host(frozen[idx]), frozen_h[rows % 64])
    assert bool((llr.view(B, N)[:: 4099] != 0).all())             # no row in between was left out


@pytest.mark.parametrize("n,K,key_bits", VERDICT_CASES)
def test_verdict_kernel_on_the_branch_rows(q, torch, n, K, key_bits):
    for crc_len, crc_poly in RR.crcs(K):
        check_verdict(q.polar_recon_verdict, q, n, K, key_bits, crc_len, crc_poly)


def test_verdict_kernel_over_several_workgroups(q, torch):
    """700 blocks of the decoded rows of a real batch, so that lanes of one wave leave at different places"""
    n, messages = 7, "f32"
    c = case(q, n)
    reps = 6
    kbob, kb, crc = np.tile(c["kbob"], (reps, 1))[:700], np.tile(c["kb"], reps)[:700], np.tile(c["crc"], reps)[:700]
    llr, frozen = q.polar_recon_prior_host(n, c["pos"], kbob, np.tile(c["syn"], (reps, 1))[:700], kb, messages)
    d = q.polar_decode_host(n, c["pos"], llr, frozen, messages)
    got = q.polar_recon_verdict(n, len(c["pos"]), d["info"], d["x"], kbob, crc, None, kb, c["crc_len"], c["crc_poly"])
    ref = q.polar_recon_verdict_host(n, len(c["pos"]), d["info"], d["x"], kbob, crc, None, kb, c["crc_len"], c["crc_poly"])
    assert all(np.array_equal(got[k], ref[k]) for k in ref) and {OK, EDECODE} <= set(ref["status"].tolist())


def test_session_refusals_on_the_device(q, torch):
    n = 6
    c = case(q, n)
    sc = q.Polar(n, c["pos"], "i8", 31, max_frames=8)
    status = lambda fn, *a, **kw: pytest.raises(q.QldpcError, fn, *a, **kw).value.status
    assert status(q.PolarRecon, sc) == ESIZE                                                     # an SC context needs a CRC
    assert status(q.PolarRecon, sc, 11, 0x621, max_blocks=9) == ESIZE
    assert status(q.PolarRecon, sc, 11, 0x621, max_blocks=-1) == EINVAL
    assert status(q.PolarRecon, sc, 11, 0x621, prior=2, pin=1) == EINVAL
    assert status(q.PolarRecon, sc, 11, 0x621, pin=32) == EINVAL
    assert status(q.PolarRecon, sc, 11, 0x821) == ESIZE
    assert status(q.PolarRecon, q.PolarList(n, c["pos"], "i8", 31, 4, 0, 0, max_frames=8)) == EINVAL           # a list context without a CRC
    lst = q.PolarList(n, c["pos"], "i8", 31, 4, 11, 0x621, max_frames=8)
    assert status(q.PolarRecon, lst, 11, 0x621) == EINVAL                                        # the CRC is the context's
    sess = q.PolarRecon(sc, 11, 0x621, max_blocks=4)
    assert sess.max_blocks == 4 and q.PolarRecon(lst).crc_len == 11
    keys = dev(torch, c["ka"][:5])
    assert status(sess.encode, keys) == ESIZE
    syn, crc = sess.encode(keys[:4])
    assert status(sess.decode, keys, dev(torch, c["syn"][:5]), dev(torch, c["crc"][:5])) == ESIZE
    assert status(sess.decode, keys[:4], syn, crc, want_pick=True) == EINVAL                    # pick is the list decoder's
    empty = sess.decode(keys[:0], syn[:0], crc[:0])
    assert empty["status"].numel() == 0


# ---- stream order ------------------------------------------------------------------------------------------------------------------------------

def stream_case(q):
    """n = 8, float messages, SC with 32 CRC bits, 65 blocks of N bits.  In the true inputs the even blocks hold one flip (accepted) and the odd ones
    25 % flips (refused), in the decoy the other way round, around different keys: every block of every output differs"""
    n, N, F = 8, 256, 65
    rng = np.random.default_rng(808)
    pos = RR.code(rng, n, "5g")
    c = dict(n=n, pos=pos, inp={}, ref={})
    for which, phase in (("true", 0), ("decoy", 1)):
        x = rng.integers(0, 2, (F, N), dtype=np.uint8)
        e = (rng.random((F, N)) < 0.25).astype(np.uint8)
        light = np.arange(F) % 2 == phase
        e[light] = 0
        e[light, rng.integers(0, N, int(light.sum()))] = 1
        ka, kbob = R.pack(x), R.pack(x ^ e)
        syn, crc = q.polar_recon_encode_host(n, pos, ka, None, *RR.CRC32)
        out = q.polar_recon_decode_host(n, pos, kbob, syn, crc, None, "f32", crc_len=RR.CRC32[0], crc_poly=RR.CRC32[1])
        assert np.array_equal(out["status"] == OK, light), which
        c["inp"][which] = (ka, kbob)
        c["ref"][which] = dict(syndrome=syn, crc=crc, status=out["status"], corrected=out["corrected"], keys=out["keys"])
    differ_in_every_frame(c["ref"]["true"], c["ref"]["decoy"], "polar recon")
    return c


def test_session_on_a_side_stream(q, torch):
    """encode -> decode on a delayed non-blocking side stream while the inputs still hold the decoy: the session's kernels and the context's run on
    the stream of the call, in order"""
    c = stream_case(q)
    delay, side = Delay(torch), torch.cuda.Stream()
    dec = q.Polar(c["n"], c["pos"], "f32", max_frames=65)
    sess = q.PolarRecon(dec, *RR.CRC32)
    ch = Chain(torch, delay, side, "polar recon")
    (ta, tb), (da, db) = c["inp"]["true"], c["inp"]["decoy"]
    alice, bob = ch.input(ta, da), ch.input(tb, db)
    with torch.cuda.stream(side):                                 # the session and its context have been driven on the decoy, on the side stream,
        syn, crc = sess.encode(alice)                             # whose allocations the chain then finds cached
        warm = [t.clone() for t in (syn, crc, bob)] + [v.clone() for v in sess.decode(bob.clone(), syn, crc).values()]
    del warm, syn, crc
    with ch:
        ch.stage()
        syn, crc = sess.encode(alice)
        ch.keep("syndrome", syn)
        ch.keep("crc", crc)
        out = sess.decode(bob, syn, crc)
        ch.keep("status", out["status"])
        ch.keep("corrected", out["corrected"])
        ch.keep("keys", bob, in_place=True)
    ch.check_all(c["ref"]["true"])
