"""CPU suite of the polar reconciliation sessions: the host mirrors (qldpc_polar_recon_*_host) against the numpy restatement of
tests/polar_recon_ref.py bit for bit, the verdict mirror on constructed rows through each of its branches, every refusal of every new call, the
operating points of the existing polar suites through the session mirror, and the sanitizer program.  No GPU, no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import polar_list_ref as LR
import polar_recon_ref as RR
import polar_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 2, 3, 4, 5, 6, 7, 8, 10, 12)
OK, EINVAL, ESIZE, EUNSUPPORTED, EDECODE = 0, -1, -6, -7, -9


def decoders(n):
    """the decoders of a size: SC, SSC, the wide form from n = 6 on, list 1 and list 4"""
    return ["sc", "ssc"] + (["wide"] if n >= 6 else []) + [1, 4]


def mirror_decode(q, n, pos, keys, syn, crc, kb, messages, maxq, decoder, crc_len, crc_poly, **kw):
    if isinstance(decoder, int):
        return q.polar_recon_decode_host(n, pos, keys, syn, crc, kb, messages, maxq, list_size=decoder, crc_len=crc_len, crc_poly=crc_poly, want_pick=True, **kw)
    form, rule = dict(sc=("lanes", "sc"), ssc=("lanes", "ssc"), wide=("wide", "sc"))[decoder]
    return q.polar_recon_decode_host(n, pos, keys, syn, crc, kb, messages, maxq, form=form, rule=rule, crc_len=crc_len, crc_poly=crc_poly, **kw)


def same_floats(a, b):
    return a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---- the mirrors against the restatement -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("messages", ["i8", "f32"])
@pytest.mark.parametrize("n", SIZES)
def test_mirrors_are_the_restatement(q, n, messages):
    """every kind of code, every CRC that fits it, key lengths N, N - 1, N - 37 and 1 mixed in a batch with clean, 2 % and 25 % blocks, junk in the
    pad of both keys: encode, prior and, around every decoder of the size, decode"""
    rng = np.random.default_rng([n, messages == "i8", 11])
    maxq = (3, 31, 126)[n % 3]
    seen = set()
    for kind in RR.CODES:
        pos = RR.code(rng, n, kind)
        for crc_len, crc_poly in RR.crcs(len(pos)):
            what = "n=%d %s %s K=%d crc_len=%d" % (n, messages, kind, len(pos), crc_len)
            ka, kbob, kb = RR.blocks(rng, n, 12)
            for key_bits in (kb, None):
                syn, crc = q.polar_recon_encode_host(n, pos, ka, key_bits, crc_len, crc_poly)
                syn_r, crc_r = RR.alice(q, n, pos, ka, key_bits, crc_len, crc_poly)
                assert syn.shape == syn_r.shape and np.array_equal(syn, syn_r) and np.array_equal(crc, crc_r), what
                llr, frozen = q.polar_recon_prior_host(n, pos, kbob, syn, key_bits, messages, maxq)
                llr_r, frozen_r = RR.prior(n, pos, kbob, syn, key_bits, messages, *RR.default_levels(messages, maxq))
                assert same_floats(llr, llr_r) and np.array_equal(frozen, frozen_r), what
            syn_k, crc_k = q.polar_recon_encode_host(n, pos, ka, kb, crc_len, crc_poly)
            for decoder in decoders(n):
                got = mirror_decode(q, n, pos, kbob, syn_k, crc_k, kb, messages, maxq, decoder, crc_len, crc_poly)
                ref = RR.bob(q, n, pos, kbob, syn_k, crc_k, kb, messages, maxq, decoder, crc_len, crc_poly)
                for k in ("status", "corrected", "keys") + (("pick",) if isinstance(decoder, int) else ()):
                    assert np.array_equal(got[k], ref[k]), "%s %s: %s" % (what, decoder, k)
                seen |= set(got["status"].tolist())
                ok = got["status"] == OK
                assert (got["corrected"][~ok] == -1).all() and np.array_equal(got["keys"][~ok], kbob[~ok]), what
    assert OK in seen and (EDECODE in seen or n <= 2)


def test_other_levels_and_a_block_out_of_range(q):
    """prior and pin of the caller's, and key_bits outside 1 .. N: the LLR row is all +pin, status ESIZE, the key untouched; Alice sends the
    message of the all-zero key"""
    rng = np.random.default_rng(5)
    n, N = 7, 128
    pos = RR.code(rng, n, "5g")
    ka, kbob, kb = RR.blocks(rng, n, 8)
    kb[2], kb[5], kb[6] = 0, N + 1, -3
    syn, crc = q.polar_recon_encode_host(n, pos, ka, kb, 11, 0x621)
    syn_r, crc_r = RR.alice(q, n, pos, ka, kb, 11, 0x621)
    assert np.array_equal(syn, syn_r) and np.array_equal(crc, crc_r) and not syn[[2, 5, 6]].any() and not crc[[2, 5, 6]].any()
    for messages, p, pin in (("i8", 2, 9), ("f32", 0.5, 1e30), ("f32", 3.0, 3.0), ("i8", 31, 31)):
        llr, frozen = q.polar_recon_prior_host(n, pos, kbob, syn, kb, messages, 31, p, pin)
        llr_r, frozen_r = RR.prior(n, pos, kbob, syn, kb, messages, p, pin)
        assert same_floats(llr, llr_r) and np.array_equal(frozen, frozen_r)
        assert (llr[[2, 5, 6]] == pin).all()
        got = q.polar_recon_decode_host(n, pos, kbob, syn, crc, kb, messages, 31, crc_len=11, crc_poly=0x621, prior=p, pin=pin)
        ref = RR.bob(q, n, pos, kbob, syn, crc, kb, messages, 31, "sc", 11, 0x621, p, pin)
        assert all(np.array_equal(got[k], ref[k]) for k in ("status", "corrected", "keys"))
        assert (got["status"][[2, 5, 6]] == ESIZE).all() and (got["corrected"][[2, 5, 6]] == -1).all() and np.array_equal(got["keys"][[2, 5, 6]], kbob[[2, 5, 6]])


# ---- the verdict on constructed rows -----------------------------------------------------------------------------------------------------------

VERDICT_CASES = [(7, 50, 100), (7, 50, 128), (7, 50, 64), (7, 50, 1), (4, 7, 16), (4, 7, 9), (10, 512, 1000), (5, 20, 31)]


def check_verdict(fn, q, n, K, key_bits, crc_len, crc_poly):
    """fn: polar_recon_verdict_host or the device's polar_recon_verdict.  The expected results are stated by verdict_rows, not computed by anything"""
    rows, want_sc, want_list, flips = RR.verdict_rows(q, np.random.default_rng([n, K, key_bits]), n, K, key_bits, crc_len, crc_poly)
    for pick, want in ((None, want_sc), (rows["pick"], want_list)):
        got = fn(n, K, rows["info"], rows["x"], rows["keys"], rows["crc"], pick, rows["key_bits"], crc_len, crc_poly)
        what = "n=%d K=%d key_bits=%d pick=%s" % (n, K, key_bits, pick is not None)
        assert np.array_equal(got["status"], want), what
        ok = want == OK
        assert np.array_equal(got["corrected"], np.where(ok, flips, -1)), what
        assert np.array_equal(got["keys"][ok], rows["x"][ok]) and np.array_equal(got["keys"][~ok], rows["keys"][~ok]), what
        ref = RR.verdict(q, n, K, rows["info"], rows["x"], rows["keys"], rows["key_bits"], rows["crc"], pick, crc_len, crc_poly)
        assert all(np.array_equal(got[k], ref[k]) for k in ("status", "corrected", "keys")), what
    assert {OK, EDECODE, ESIZE} <= set(want_sc.tolist()) and {OK, EDECODE, ESIZE} <= set(want_list.tolist())


@pytest.mark.parametrize("n,K,key_bits", VERDICT_CASES)
def test_verdict_branches(q, n, K, key_bits):
    for crc_len, crc_poly in RR.crcs(K):
        check_verdict(q.polar_recon_verdict_host, q, n, K, key_bits, crc_len, crc_poly)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------

def _status(q, fn, *args, **kw):
    with pytest.raises(q.QldpcError) as e:
        fn(*args, **kw)
    assert str(e.value)
    return e.value.status


def test_argument_checks_of_the_mirrors(q):
    z = lambda B, n: np.zeros((B, max(1, (1 << n) // 32)), np.uint32)
    enc, dec, pri, ver = q.polar_recon_encode_host, q.polar_recon_decode_host, q.polar_recon_prior_host, q.polar_recon_verdict_host
    c = np.zeros(1, np.uint32)
    # the code
    assert _status(q, enc, 0, [], np.zeros((1, 1), np.uint32), None, 1, 1) == ESIZE
    assert _status(q, enc, 21, [], np.zeros((1, 1), np.uint32), None, 1, 1) == ESIZE
    assert _status(q, enc, 3, [1, 8], z(1, 3), None, 1, 1) == ESIZE
    assert _status(q, enc, 3, [1, 1], z(1, 3), None, 1, 1) == EINVAL
    assert _status(q, q.polar_recon_tables, 0, []) == ESIZE
    assert _status(q, q.polar_recon_tables, 3, [9]) == ESIZE
    # the CRC: 1 .. min(32, K), the polynomial within crc_len bits
    for crc_len, crc_poly in ((0, 0), (-1, 0), (33, 0), (3, 1), (2, 4)):
        assert _status(q, enc, 3, [1, 2], z(1, 3), None, crc_len, crc_poly) == ESIZE
        assert _status(q, dec, 3, [1, 2], z(1, 3), z(1, 3), c, crc_len=crc_len, crc_poly=crc_poly) == ESIZE
        assert _status(q, ver, 3, 2, z(1, 3), z(1, 3), z(1, 3), c, crc_len=crc_len, crc_poly=crc_poly) == ESIZE
    assert _status(q, enc, 3, [], z(1, 3), None, 1, 1) == ESIZE                                   # K = 0 has room for no CRC
    # the levels
    for messages, p, pin in (("i8", 0, 5), ("i8", 6, 5), ("i8", 1, 32), ("i8", 1.5, 5), ("i8", 1, 4.5), ("i8", float("nan"), 5), ("f32", 0.0, 1.0), ("f32", -1.0, 1.0),
                             ("f32", 2.0, 1.0), ("f32", 1.0, 2e30), ("f32", 1.0, float("inf")), ("f32", float("nan"), 1.0), ("f32", 1e-60, 1.0)):
        assert _status(q, pri, 3, [1, 2], z(1, 3), z(1, 3), None, messages, 31, p, pin) == EINVAL
        assert _status(q, dec, 3, [1, 2], z(1, 3), z(1, 3), c, None, messages, 31, crc_len=1, crc_poly=1, prior=p, pin=pin) == EINVAL
    assert _status(q, pri, 3, [1], z(1, 3), z(1, 3), None, "i8", 127) == ESIZE
    assert _status(q, pri, 3, [1], z(1, 3), z(1, 3), None, "f16") == EINVAL
    # the decoder of the decode mirror
    assert _status(q, dec, 3, [1, 2], z(1, 3), z(1, 3), c, list_size=3, crc_len=1, crc_poly=1) == ESIZE
    assert _status(q, dec, 17, [1, 2], z(1, 17), z(1, 17), c, list_size=4, crc_len=1, crc_poly=1) == ESIZE      # the list decoder goes to 2^16
    assert _status(q, dec, 3, [1, 2], z(1, 3), z(1, 3), c, form=2, crc_len=1, crc_poly=1) == EINVAL
    assert _status(q, dec, 3, [1, 2], z(1, 3), z(1, 3), c, rule=2, crc_len=1, crc_poly=1) == EINVAL
    assert _status(q, dec, 3, [1, 2], z(1, 3), z(1, 3), c, form="wide", list_size=4, crc_len=1, crc_poly=1) == EINVAL
    assert _status(q, dec, 6, [1, 2], z(1, 6), z(1, 6), c, form="wide", rule="ssc", crc_len=1, crc_poly=1) == EUNSUPPORTED
    assert _status(q, dec, 3, [1, 2], z(1, 3), z(1, 3), c, crc_len=1, crc_poly=1, want_pick=True) == EINVAL     # pick is the list decoder's
    assert _status(q, ver, 0, 0, np.zeros((1, 0), np.uint32), np.zeros((1, 1), np.uint32), np.zeros((1, 1), np.uint32), c, crc_len=1, crc_poly=1) == ESIZE
    assert _status(q, ver, 3, 9, z(1, 3), z(1, 3), z(1, 3), c, crc_len=1, crc_poly=1) == ESIZE
    # shapes, refused by the binding
    assert _status(q, enc, 6, [1, 2], z(1, 5), None, 1, 1) == ESIZE
    assert _status(q, enc, 3, [1, 2], z(2, 3), [8], 1, 1) == ESIZE
    assert _status(q, dec, 6, [1, 2], z(1, 6), z(1, 5), c, crc_len=1, crc_poly=1) == ESIZE
    assert _status(q, dec, 3, [1, 2], z(2, 3), z(2, 3), c, crc_len=1, crc_poly=1) == ESIZE
    # counts and pointers, at the C ABI
    L = q._L
    ip = np.array([1, 2], np.int32).ctypes.data_as(q._ip)
    w = np.zeros(4, np.uint32).ctypes.data_as(q._up)
    i4 = np.zeros(4, np.int32).ctypes.data_as(q._ip)
    assert L.qldpc_polar_recon_encode_host(3, 2, ip, 1, 1, -1, w, None, w, w) == EINVAL
    assert L.qldpc_polar_recon_encode_host(3, 2, ip, 1, 1, 0, None, None, None, None) == OK
    assert L.qldpc_polar_recon_encode_host(3, 2, ip, 1, 1, 1, None, None, w, w) == EINVAL
    assert L.qldpc_polar_recon_encode_host(3, 2, ip, 1, 1, 1, w, None, None, w) == EINVAL
    assert L.qldpc_polar_recon_encode_host(3, 2, ip, 1, 1, 1, w, None, w, None) == EINVAL
    assert L.qldpc_polar_recon_prior_host(3, 2, ip, 0, 31, 1.0, 31.0, -1, w, None, w, w, w) == EINVAL
    assert L.qldpc_polar_recon_prior_host(3, 2, ip, 0, 31, 1.0, 31.0, 0, None, None, None, None, None) == OK
    for hole in range(4):
        a = [w, w, w, w]
        a[hole] = None
        assert L.qldpc_polar_recon_prior_host(3, 2, ip, 0, 31, 1.0, 31.0, 1, a[0], None, a[1], a[2], a[3]) == EINVAL
    assert L.qldpc_polar_recon_verdict_host(3, 2, 1, 1, -1, w, w, None, w, None, w, i4, i4) == EINVAL
    assert L.qldpc_polar_recon_verdict_host(3, 2, 1, 1, 0, None, None, None, None, None, None, None, None) == OK
    for hole in range(5):
        a = [w, w, w, w, i4]
        a[hole] = None
        assert L.qldpc_polar_recon_verdict_host(3, 2, 1, 1, 1, a[0], a[1], None, a[2], None, a[3], a[4], None) == EINVAL
    assert L.qldpc_polar_recon_verdict_host(3, 2, 0, 0, 1, None, w, i4, w, None, None, i4, None) == OK             # with pick neither info nor crc is needed
    assert L.qldpc_polar_recon_decode_host(3, 2, ip, 0, 31, 0, 0, 0, 1, 1, 1.0, 31.0, -1, w, None, w, w, i4, None, None) == EINVAL
    assert L.qldpc_polar_recon_decode_host(3, 2, ip, 0, 31, 0, 0, 0, 1, 1, 1.0, 31.0, 0, None, None, None, None, None, None, None) == OK
    for hole in range(4):
        a = [w, w, w, i4]
        a[hole] = None
        assert L.qldpc_polar_recon_decode_host(3, 2, ip, 0, 31, 0, 0, 0, 1, 1, 1.0, 31.0, 1, a[0], None, a[1], a[2], a[3], None, None) == EINVAL
    full = np.arange(8, dtype=np.int32).ctypes.data_as(q._ip)
    assert L.qldpc_polar_recon_encode_host(3, 8, full, 1, 1, 1, w, None, None, w) == OK                          # K = N: there is no syndrome
    assert L.qldpc_polar_recon_prior_host(3, 8, full, 0, 31, 1.0, 31.0, 1, w, None, None, np.zeros(8, np.int8).ctypes.data_as(q._vp), w) == OK


def test_argument_checks_of_the_device_calls_without_a_device(q):
    """every check of the session calls and of the two building blocks comes before the first HIP call, so it is the same on a machine without a
    GPU; a session needs a context, which needs a device, so here its calls meet no session"""
    L = q._L
    h = q._vp()
    one = q._vp(64)      # a pointer that is never followed: every call below is refused, or has nothing to do, before it would be
    assert L.qldpc_polar_recon_create(None, None, 11, 0x621, 1.0, 31.0, 0, C.byref(h)) == EINVAL and not h.value
    assert L.qldpc_polar_recon_create(None, None, 11, 0x621, 1.0, 31.0, 0, None) == EINVAL
    assert L.qldpc_polar_recon_encode_dev(None, 1, one, None, one, one) == EINVAL
    assert L.qldpc_polar_recon_decode_dev(None, 1, one, None, one, one, one, None, None) == EINVAL
    assert L.qldpc_polar_recon_device_bytes(None) == 0
    assert L.qldpc_polar_recon_syndrome_words(None) == EINVAL and L.qldpc_polar_recon_leaked_bits(None) == EINVAL
    L.qldpc_polar_recon_free(None)
    pri, ver = L.qldpc_polar_recon_prior_dev, L.qldpc_polar_recon_verdict_dev
    assert pri(None, 0, 0, one, one, 0, 31, 1.0, 31.0, 1, one, None, one, one, one) == ESIZE
    assert pri(None, 3, 2, one, one, 2, 31, 1.0, 31.0, 1, one, None, one, one, one) == EINVAL
    assert pri(None, 3, 2, one, one, 0, 127, 1.0, 31.0, 1, one, None, one, one, one) == ESIZE
    assert pri(None, 3, 2, one, one, 0, 31, 0.0, 31.0, 1, one, None, one, one, one) == EINVAL
    assert pri(None, 3, 2, one, one, 1, 31, 1.0, 1e31, 1, one, None, one, one, one) == EINVAL
    assert pri(None, 3, 9, one, one, 0, 31, 1.0, 31.0, 1, one, None, one, one, one) == ESIZE
    assert pri(None, 3, -1, one, one, 0, 31, 1.0, 31.0, 1, one, None, one, one, one) == ESIZE
    assert pri(None, 3, 2, one, one, 0, 31, 1.0, 31.0, -1, one, None, one, one, one) == EINVAL
    assert pri(None, 3, 2, None, None, 0, 31, 1.0, 31.0, 0, None, None, None, None, None) == OK
    for hole in range(6):
        a = [one] * 6
        a[hole] = None
        assert pri(None, 3, 2, a[0], a[1], 0, 31, 1.0, 31.0, 1, a[2], None, a[3], a[4], a[5]) == EINVAL
    assert ver(None, 0, 0, 1, 1, 1, one, one, None, one, None, one, one, None) == ESIZE
    assert ver(None, 3, 9, 1, 1, 1, one, one, None, one, None, one, one, None) == ESIZE
    assert ver(None, 3, 2, 0, 0, 1, one, one, None, one, None, one, one, None) == ESIZE
    assert ver(None, 3, 2, 3, 1, 1, one, one, None, one, None, one, one, None) == ESIZE
    assert ver(None, 3, 2, 1, 2, 1, one, one, None, one, None, one, one, None) == ESIZE
    assert ver(None, 3, 2, 1, 1, -1, one, one, None, one, None, one, one, None) == EINVAL
    assert ver(None, 3, 2, 1, 1, 0, None, None, None, None, None, None, None, None) == OK
    for hole in range(5):
        a = [one] * 5
        a[hole] = None
        assert ver(None, 3, 2, 1, 1, 1, a[0], a[1], None, a[2], None, a[3], a[4], None) == EINVAL
    for hole in range(3):
        a = [one] * 3
        a[hole] = None
        assert ver(None, 3, 2, 0, 0, 1, None, a[0], one, a[1], None, None, a[2], None) == EINVAL


# ---- the operating points of the existing suites, through the session mirror -------------------------------------------------------------------

def test_operating_point_of_the_sc_suite(q):
    """R.recon_frames(1): N = 1 024, K = 512 in the 5G order, QBER 2 %, 2 000 blocks, Bob's key the hard decisions of his LLRs; floats, the default
    prior, 32 CRC bits.  The bar is the one tests/test_polar_host.py sets for this point (1 995 of 2 000); with 32 CRC bits a wrong accept has an
    expectation below 1e-6 here, so none is the condition"""
    pos, x, _, llr = R.recon_frames(1)
    alice, bob = R.pack(x), R.pack((llr < 0).astype(np.uint8))
    syn, crc = q.polar_recon_encode_host(10, pos, alice, None, *RR.CRC32)
    assert syn.shape == (2000, 16)
    out = q.polar_recon_decode_host(10, pos, bob, syn, crc, None, "f32", crc_len=RR.CRC32[0], crc_poly=RR.CRC32[1])
    ok = out["status"] == OK
    same = (out["keys"] == alice).all(axis=1)
    flips = (R.unpack(alice, 1024) ^ R.unpack(bob, 1024)).sum(axis=1)
    print("QBER 0.02, 2 000 keys, SC float, prior 1: %d OK, %d of them wrong, leak %d bits a block" % (ok.sum(), (ok & ~same).sum(), 512 + 32))
    assert ok.sum() >= 1995
    assert not (ok & ~same).any()
    assert np.array_equal(out["corrected"][ok], flips[ok]) and (out["corrected"][~ok] == -1).all() and np.array_equal(out["keys"][~ok], bob[~ok])


def test_operating_point_of_the_list_suite(q):
    """LR.recon_frames() (QBER 6 %, where SC starts to fail) with list 4 and CRC 11 beside SC with the same CRC.  Wrong accepts are expected at
    about 2^-11 x the failed frames = 0.05, so at most 2; every one is counted and printed"""
    pos, x, _, llr = LR.recon_frames()
    alice, bob = R.pack(x), R.pack((llr < 0).astype(np.uint8))
    syn, crc = q.polar_recon_encode_host(10, pos, alice, None, *LR.CRC11)
    res = {}
    for name, L in (("SC", 0), ("list 4", 4)):
        out = q.polar_recon_decode_host(10, pos, bob, syn, crc, None, "f32", list_size=L, crc_len=LR.CRC11[0], crc_poly=LR.CRC11[1], want_pick=bool(L))
        ok = out["status"] == OK
        wrong = ok & (out["keys"] != alice).any(axis=1)
        res[name] = (int(ok.sum()), int(wrong.sum()))
        print("QBER 0.06, 2 000 keys, %s + CRC 11: %d OK, %d wrong keys accepted %s" % (name, res[name][0], res[name][1], np.flatnonzero(wrong).tolist()))
        if L:
            assert np.array_equal(ok, out["pick"] >= 0)      # the pad is the whole of nothing here: the pick alone decides
    assert res["list 4"][0] > res["SC"][0]
    assert res["SC"][1] <= 2 and res["list 4"][1] <= 2


# ---- the sanitizer program ---------------------------------------------------------------------------------------------------------------------

def test_host_code_under_asan_ubsan(tmp_path):
    """the four mirrors and the tables at every size up to 2^9 around every host decoder, every row malloc'ed at its exact size, and every refusal,
    as a stand-alone program (nothing loaded into Python is sanitised)"""
    exe = str(tmp_path / "polar_recon_sanitize")
    csrc = os.path.join(ROOT, "qcrypto-ldpc_amd", "csrc")
    srcs = ["qldpc_polar_recon_host.c", "qldpc_polar_host.c", "qldpc_polar_ssc_host.c", "qldpc_polar_wide_host.c", "qldpc_polar_list_host.c"]
    subprocess.check_call(["gcc", "-std=gnu11", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                           "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-o", exe, os.path.join(ROOT, "tests", "c", "polar_recon_sanitize.c")] +
                          [os.path.join(csrc, s) for s in srcs] + ["-lm"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "sanitizer pass ok" in r.stdout, r.stdout + r.stderr
