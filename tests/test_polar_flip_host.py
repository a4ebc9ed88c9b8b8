"""CPU suite of SC-Flip trials in the polar reconciliation sessions: the select mirror (qldpc_polar_flip_select_host) and the session mirror
(qldpc_polar_recon_decode_flip_host) against the numpy restatement of tests/polar_flip_ref.py bit for bit, resume after a plain decode, the case in
which two trials of a block pass a short CRC, monotonicity, the operating point of the issue with a CRC-32 as the verdict, every refusal of both
mirrors, and the sanitizer program.  No GPU, no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import polar_flip_ref as FL
import polar_ladder_ref as LD
import polar_recon_ref as RR
import polar_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EINVAL, ESIZE, ESTATE, EDECODE = 0, -1, -6, -8, -9
FLIP_KEYS = ("keys", "status", "corrected", "flip_pos", "decodes")


def same(a, b, keys, what):
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8)), what + ": " + k
    if "n_tried" in a and "n_tried" in b:
        assert int(a["n_tried"]) == int(b["n_tried"]), what + ": n_tried"


# ---- the select ------------------------------------------------------------------------------------------------------------------------------

def select_inputs(rng, n, messages, F):
    """-> a list of (name, leaf [F, N], frozen bool [N], rank or None, extra or None): random leaves; all-equal leaves (the position decides
    alone); zeros of both signs and denormals (floats) or -1 / 0 / 1 (int8); fewer candidates than flips; none; a ladder whose counts remove
    candidates"""
    N = 1 << n
    dt = np.int8 if messages == "i8" else np.float32
    pos, frozen = R.random_code(rng, N, max(1, N // 2))
    rand = R.i8_inputs(rng, F, N, 126).clip(-127, 126) if messages == "i8" else R.f32_inputs(rng, F, N)
    if messages == "i8":
        equal = np.full((F, N), 5, np.int8) * np.where(rng.random((F, N)) < 0.5, -1, 1).astype(np.int8)
        tiny = rng.integers(-1, 2, (F, N)).astype(np.int8)
    else:
        equal = (np.where(rng.random((F, N)) < 0.5, -1.0, 1.0) * 2.5).astype(np.float32)
        sign = np.where(rng.random((F, N)) < 0.5, -1.0, 1.0)
        tiny = (sign * rng.integers(0, 3, (F, N)) * 1.401298464324817e-45).astype(np.float32)      # -0.0, +0.0 and the two smallest denormals
    few = np.ones(N, bool)
    few[rng.permutation(N)[:min(N, 3)]] = False
    E = max(1, int((~frozen).sum()) // 2)
    rank = LD.rank_table(N, LD.ladder(rng, pos, E))
    rank32 = np.where(rank > 0x7fffffff, 0x7fffffff, rank).astype(np.int32)
    extra = rng.integers(0, E + 1, F).astype(np.int32)
    extra[0], extra[-1] = 0, E
    return [("random", rand.astype(dt), frozen, None, None), ("equal", equal, frozen, None, None), ("tiny", tiny, frozen, None, None), ("few", rand.astype(dt), few, None, None),
            ("none", rand.astype(dt), np.ones(N, bool), None, None), ("ladder", equal, frozen, rank32, extra), ("ladder, no counts", tiny, frozen, rank32, None)]


@pytest.mark.parametrize("messages", ["i8", "f32"])
@pytest.mark.parametrize("n", [1, 2, 5, 6, 8, 10])
def test_select_mirror_is_the_restatement(q, n, messages):
    rng = np.random.default_rng([n, messages == "i8", 61])
    for name, leaf, frozen, rank, extra in select_inputs(rng, n, messages, 7):
        for T in (1, 2, 8, 32):
            got = q.polar_flip_select_host(n, leaf, R.pack(frozen[None, :].astype(np.uint8))[0], T, rank, extra, messages)
            want = FL.select(leaf, frozen, T, rank, extra)
            assert got.dtype == np.int32 and np.array_equal(got, want), "%s n=%d T=%d %s" % (name, n, T, messages)
            if name == "none":
                assert (got == -1).all()
            if name == "few":
                assert ((got >= 0).sum(axis=1) == min(T, 3, 1 << n)).all()
            if name == "equal" and rank is None:                    # the position alone decides: the first T information positions
                assert np.array_equal(got[0][got[0] >= 0], np.flatnonzero(~frozen)[:T])


# ---- the session mirror ----------------------------------------------------------------------------------------------------------------------------

def session_case(n, seed, qber, B=36, crc=None, E=0, kind="random"):
    """a code (random unless another kind is asked for), B blocks through a BSC with the key lengths N, N - 1 and N - 5 in turn (junk past the
    length on both sides), a CRC (the longest of the suites that fits K unless one is given), a ladder of E entries with mixed counts, and
    Alice's rows from the restatement"""
    rng = np.random.default_rng([n, seed, 51])
    N = 1 << n
    pos = RR.code(rng, n, kind)
    crc_len, crc_poly = crc or RR.crcs(len(pos))[-1]
    lengths = [N, N - 1, max(1, N - 5)]
    kb = np.array([lengths[b % 3] for b in range(B)], np.int32)
    x = rng.integers(0, 2, (B, N), dtype=np.uint8)
    e = (rng.random((B, N)) < qber).astype(np.uint8)
    junk = np.arange(N)[None, :] >= kb[:, None]
    ka = R.pack(np.where(junk, rng.integers(0, 2, (B, N), dtype=np.uint8), x))
    kbob = R.pack(np.where(junk, rng.integers(0, 2, (B, N), dtype=np.uint8), x ^ e))
    xp = LD.ladder(rng, pos, E)
    syn, cr, xb = LD.alice(n, pos, xp, ka, kb, crc_len, crc_poly)
    extra = rng.integers(0, E + 1, B).astype(np.int32) if E else None
    return dict(n=n, pos=pos, xp=xp, crc=(crc_len, crc_poly), ka=ka, kbob=kbob, kb=kb, syn=syn, xcrc=cr, xb=xb if E else None, extra=extra)


def mirror(q, c, T, messages, keys=None, **kw):
    return q.polar_recon_decode_flip_host(c["n"], c["pos"], c["kbob"] if keys is None else keys, c["syn"], c["xcrc"], n_flips=T, extra_pos=c["xp"], extra_bits=c["xb"],
                                          extra=c["extra"], key_bits=c["kb"], messages=messages, crc_len=c["crc"][0], crc_poly=c["crc"][1], **kw)


def restated(c, T, messages, keys=None, **kw):
    return FL.flip(c["n"], c["pos"], c["kbob"] if keys is None else keys, c["syn"], c["xcrc"], T, extra_pos=c["xp"], extra_bits=c["xb"], extra=c["extra"], key_bits=c["kb"],
                   messages=messages, crc_len=c["crc"][0], crc_poly=c["crc"][1], **kw)


def three_kinds(out):
    """a block that is OK at once, a rescued block and a block that still fails"""
    at_once = (out["status"] == OK) & (out["decodes"] == 1)
    return at_once.any() and (out["flip_pos"] >= 0).any() and (out["status"] == EDECODE).any()


# (n, n_flips, seed, qber, ladder entries): seeds and rates chosen on the CPU so that every case holds the three kinds of block
SESSION_CASES = [(2, 1, 3, 0.1, 0), (5, 8, 3, 0.02, 0), (5, 1, 3, 0.02, 0), (6, 8, 1, 0.02, 0), (6, 1, 1, 0.02, 0), (8, 8, 4, 0.006, 0), (8, 1, 4, 0.006, 0),
                 (5, 8, 1, 0.02, 3), (6, 1, 1, 0.02, 3)]


@pytest.mark.parametrize("messages", ["i8", "f32"])
@pytest.mark.parametrize("n,T,seed,qber,E", SESSION_CASES)
def test_session_mirror_is_the_restatement(q, n, T, seed, qber, E, messages):
    """every output, short keys among the blocks; then a plain decode followed by a resumed flip call against the call that does both"""
    c = session_case(n, seed, qber, E=E)
    what = "n=%d T=%d E=%d %s" % (n, T, E, messages)
    want = restated(c, T, messages)
    assert three_kinds(want), what
    got = mirror(q, c, T, messages)
    same(got, want, FLIP_KEYS, what)
    open_ = want["decodes"] > 1
    assert want["n_tried"] == int(open_.sum()) and (want["decodes"][open_] == 2 + T).all() and (want["flip_pos"][~open_] == -1).all()
    rescued = want["flip_pos"] >= 0
    assert (want["status"][rescued] == OK).all() and (want["corrected"][rescued] >= 0).all()
    # monotone: a block that is OK without flips keeps every output
    if E == 0:
        plain = q.polar_recon_decode_host(n, c["pos"], c["kbob"], c["syn"], c["xcrc"], c["kb"], messages, crc_len=c["crc"][0], crc_poly=c["crc"][1])
        ok = plain["status"] == OK
        assert ok.any() and np.array_equal(got["keys"][ok], plain["keys"][ok]) and np.array_equal(got["corrected"][ok], plain["corrected"][ok])
        assert (got["status"][ok] == OK).all() and (got["flip_pos"][ok] == -1).all() and (got["decodes"][ok] == 1).all()
        # resume after the plain decode: the same keys, status, corrected and flip_pos; the decodes without the first pass
        res = mirror(q, c, T, messages, keys=plain["keys"], resume=True, status=plain["status"])
        same(res, restated(c, T, messages, keys=plain["keys"], resume=True, status=plain["status"]), FLIP_KEYS, what + " resume")
        same(res, got, ("keys", "status", "flip_pos"), what + " resume against one call")
        assert np.array_equal(np.where(res["decodes"] > 0, res["corrected"], plain["corrected"]), got["corrected"])
        assert np.array_equal(res["decodes"], np.where(open_, 1 + T, 0))


def test_the_lowest_of_two_accepted_trials_wins(q):
    """a 4-bit CRC and 32 flips: blocks with two and more accepted trials exist (asserted from the restatement), and the lowest takes the key"""
    c = session_case(6, 0, 0.12, crc=(4, 0x3))
    want = restated(c, 32, "i8")
    two = [b for b, a in want["accepted"].items() if len(a) >= 2]
    assert two and three_kinds(want)
    same(mirror(q, c, 32, "i8"), want, FLIP_KEYS, "two accepted trials")
    for T in (8, 16):
        same(mirror(q, c, T, "f32"), restated(c, T, "f32"), FLIP_KEYS, "two accepted trials, T=%d" % T)


def test_resume_leaves_the_other_blocks_alone(q):
    c = session_case(6, 1, 0.02)
    B = c["ka"].shape[0]
    status = np.array([EDECODE, OK, ESIZE, 77] * (B // 4), np.int32)
    kb = c["kb"].copy()
    kb[4] = 0                                                      # an EDECODE block with no valid length: refused
    c = dict(c, kb=kb)
    got = mirror(q, c, 4, "f32", resume=True, status=status)
    same(got, restated(c, 4, "f32", resume=True, status=status), FLIP_KEYS, "resume")
    kept = status != EDECODE
    assert np.array_equal(got["status"][kept], status[kept]) and np.array_equal(got["keys"][kept], c["kbob"][kept]) and not got["decodes"][kept].any()
    assert got["status"][4] == ESIZE and got["decodes"][4] == 0 and got["n_tried"] == int((~kept).sum()) - 1


# ---- the operating point ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("messages", ["f32", "i8"])
def test_operating_point_with_a_crc32_verdict(q, messages):
    """N = 1 024, K = 512 in the 5G order, 2 000 keys through a BSC of 6 %, seed 20263, prior 1: SC fails 156 blocks; 97 / 120 / 131 of them are
    rescued by 1 / 8 / 16 flips (the issue's truth-judged counts, confirmed through the mirror; with a CRC-32 they hold but for a 2^-32 event),
    and no rescued key differs from Alice's"""
    n, pos, _, ka, kbob = LD.operating_point()
    syn, crc = q.polar_recon_encode_host(n, pos, ka, None, *RR.CRC32)
    for T, rescued in ((1, 97), (8, 120), (16, 131)):
        out = q.polar_recon_decode_flip_host(n, pos, kbob, syn, crc, n_flips=T, messages=messages, crc_len=32, crc_poly=RR.CRC32[1])
        print("T=%d: first pass failed %d, rescued %d" % (T, out["n_tried"], int((out["flip_pos"] >= 0).sum())))
        assert out["n_tried"] == 156 and int((out["flip_pos"] >= 0).sum()) == rescued
        ok = out["status"] == OK
        assert int(ok.sum()) == 2000 - 156 + rescued and np.array_equal(out["keys"][ok], ka[ok]) and set(out["status"].tolist()) == {OK, EDECODE}


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------

def status_of(q, fn, *args, **kw):
    with pytest.raises(q.QldpcError) as e:
        fn(*args, **kw)
    assert str(e.value)
    return e.value.status


def test_refusals_of_the_select_mirror(q):
    leaf, mask = np.zeros((2, 8), np.int8), np.zeros(1, np.uint32)
    sel = lambda *a, **kw: q.polar_flip_select_host(*a, **kw)
    for T in (0, -1, 3, 12, 48):
        assert status_of(q, sel, 3, leaf, mask, T) == EINVAL, T
    assert status_of(q, sel, 3, leaf, mask, 64) == ESIZE          # a power of two above the 32 flips there can be
    assert status_of(q, sel, 0, np.zeros((2, 1), np.int8), mask, 1) == ESIZE and status_of(q, sel, 21, np.zeros((2, 1), np.int8), mask, 1) == ESIZE
    assert status_of(q, sel, 3, leaf, mask, 1, messages="f16") == EINVAL
    assert status_of(q, sel, 3, leaf[:, :4], mask, 1) == ESIZE and status_of(q, sel, 3, leaf, np.zeros(2, np.uint32), 1) == ESIZE
    L, ip, up = q._L, C.POINTER(C.c_int), C.POINTER(C.c_uint32)
    pos = np.zeros((2, 2), np.int32)
    full = (leaf.ctypes.data_as(C.c_void_p), mask.ctypes.data_as(up), pos.ctypes.data_as(ip))
    assert L.qldpc_polar_flip_select_host(3, 0, 2, full[0], full[1], None, None, 2, full[2]) == OK
    for k in range(3):
        a = [None if j == k else v for j, v in enumerate(full)]
        assert L.qldpc_polar_flip_select_host(3, 0, 2, a[0], a[1], None, None, 2, a[2]) == EINVAL, k
    assert L.qldpc_polar_flip_select_host(3, 0, -1, full[0], full[1], None, None, 2, full[2]) == EINVAL
    assert L.qldpc_polar_flip_select_host(3, 0, 0, None, None, None, None, 2, None) == OK


def test_refusals_of_the_session_mirror(q):
    n, pos = 4, np.array([3, 5, 9, 12, 15], np.int32)
    keys, syn, crc = np.zeros((2, 1), np.uint32), np.zeros((2, 1), np.uint32), np.zeros(2, np.uint32)
    xb, extra = np.zeros((2, 1), np.uint32), np.zeros(2, np.int32)
    dec = lambda xp=(3, 9), **kw: q.polar_recon_decode_flip_host(n, pos, keys, syn, crc, kw.pop("n_flips", 2), extra_pos=xp, extra_bits=xb if len(xp) else None,
                                                                 extra=kw.pop("extra", extra), crc_len=kw.pop("crc_len", 3), crc_poly=3, **kw)
    for T in (0, -2, 3, 24, 48):
        assert status_of(q, dec, n_flips=T) == EINVAL, T
    assert status_of(q, dec, n_flips=64) == ESIZE
    assert status_of(q, dec, resume=2, status=extra) == EINVAL and status_of(q, dec, resume=True) == EINVAL
    assert status_of(q, dec, (3, 5, 9, 12, 15, 1)) == ESIZE and status_of(q, dec, (3, 3)) == EINVAL and status_of(q, dec, (4,)) == EINVAL
    assert status_of(q, dec, crc_len=0) == ESIZE and status_of(q, dec, messages="f16") == EINVAL and status_of(q, dec, maxq=127) == ESIZE
    assert status_of(q, dec, prior=0.0) == EINVAL and status_of(q, dec, pin=32.0) == EINVAL
    assert dec(())["status"].tolist() == dec()["status"].tolist() and dec(n_flips=32)["flip_pos"].shape == (2,)
    bad = dec(extra=np.array([0, 3], np.int32))                     # a count above the ladder: the block's refusal, not the call's
    assert bad["status"][1] == ESIZE and bad["decodes"][1] == 0 and bad["flip_pos"][1] == -1
    L, ip, up = q._L, C.POINTER(C.c_int), C.POINTER(C.c_uint32)
    P = lambda a, t: a.ctypes.data_as(t)
    xp, st, fp = np.array([3, 9], np.int32), np.zeros(2, np.int32), np.zeros(2, np.int32)

    def raw(B, keys_, crc_, xb_, status_, flip_, syn_=syn, extra_=None):
        return L.qldpc_polar_recon_decode_flip_host(n, 5, P(pos, ip), 0, 31, 3, 3, 1.0, 31.0, 2, P(xp, ip), B, keys_, None, P(syn_, up) if syn_ is not None else None,
                                                    crc_, xb_, extra_, 2, 0, status_, None, flip_, None, None)
    full = (P(keys, up), P(crc, up), P(xb, up), P(st, ip), P(fp, ip))
    assert raw(2, *full) == OK and raw(2, *full, extra_=P(extra, ip)) == OK      # extra is optional: every count 0
    for k in range(5):
        assert raw(2, *[None if j == k else a for j, a in enumerate(full)]) == EINVAL, k
    assert raw(2, *full, syn_=None) == EINVAL
    assert raw(-1, *full) == EINVAL and raw(0, None, None, None, None, None) == OK


# ---- the sanitizer program ---------------------------------------------------------------------------------------------------------------------------

def test_host_code_under_asan_ubsan(tmp_path):
    """both mirrors at every size up to 2^9 with every array malloc'ed at its stated size, and their refusals, as a stand-alone program (nothing
    loaded into Python is sanitised)"""
    exe = str(tmp_path / "polar_flip_sanitize")
    csrc = os.path.join(ROOT, "qcrypto-ldpc_amd", "csrc")
    units = ["qldpc_polar_host.c", "qldpc_polar_ssc_host.c", "qldpc_polar_wide_host.c", "qldpc_polar_list_host.c", "qldpc_polar_recon_host.c", "qldpc_polar_ladder_host.c",
             "qldpc_polar_flip_host.c"]
    subprocess.check_call(["gcc", "-std=gnu11", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                           "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-o", exe, os.path.join(ROOT, "tests", "c", "polar_flip_sanitize.c")] +
                          [os.path.join(csrc, u) for u in units] + ["-lm"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "sanitizer pass ok" in r.stdout, r.stdout + r.stderr
