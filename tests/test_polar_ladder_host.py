"""CPU suite of incremental freezing in the polar subsystem: the rows form of the SC mirror (qldpc_polar_decode_rows_host) and the ladder mirrors
(qldpc_polar_recon_encode_ladder_host, _decode_rounds_host, _ladder_extra_host) against the numpy restatement of tests/polar_ladder_ref.py bit for
bit, the equalities of the rule, the operating point of the issue through the mirrors with a CRC-32 as the verdict, every refusal of every new
call, and the sanitizer program.  No GPU, no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import polar_ladder_ref as LD
import polar_recon_ref as RR
import polar_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 2, 3, 4, 5, 6, 7, 8, 9, 12)
OK, EINVAL, ESIZE, ESTATE, EDECODE = 0, -1, -6, -8, -9


def inputs(rng, messages, F, N, maxq):
    return R.i8_inputs(rng, F, N, maxq) if messages == "i8" else R.f32_inputs(rng, F, N)


def mask_of(pos, N):
    mask = np.ones(N, bool)
    mask[np.asarray(pos, np.int64)] = False
    return mask


def codes(rng, n):
    """random, clustered and 5G codes (the polarization-weight order above N = 1 024), K = 0 and K = N; two of them at n = 12, where the restatement
    takes a while"""
    N = 1 << n
    kinds = ("random", "5g") if n > 9 else ("random", "clustered", "5g")
    out = [RR.code(rng, n, kind) for kind in kinds]
    return out + ([] if n > 9 else [np.zeros(0, np.int32), np.arange(N, dtype=np.int32)])


# ---- the rows decode -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("messages", ["i8", "f32"])
@pytest.mark.parametrize("n", SIZES)
def test_rows_mirror_is_the_restatement(q, n, messages):
    """u, info, x and leaf with rows random per frame (every frame a frozen set of its own), all zero and all ones, with and without frozen values"""
    rng = np.random.default_rng([n, messages == "i8", 31])
    N, F, maxq = 1 << n, (2 if n > 9 else 5), (1, 31, 126)[n % 3]
    for pos in codes(rng, n):
        mask = mask_of(pos, N)
        llr = inputs(rng, messages, F, N, maxq)
        fv = rng.integers(0, 2, (F, N), dtype=np.uint8)
        for kind, rows in (("random", (rng.random((F, N)) < rng.random((F, 1))).astype(np.uint8)), ("zero", np.zeros((F, N), np.uint8)), ("ones", np.ones((F, N), np.uint8))):
            values = fv if kind != "zero" else None
            out = q.polar_decode_rows_host(n, pos, llr, R.pack(rows), None if values is None else R.pack(values), messages, maxq, leaf=True)
            R.check_outputs(out, LD.decode_rows(llr, mask, rows, values, messages, maxq), pos, N, mask, "n=%d K=%d %s rows %s" % (n, len(pos), kind, messages))


def same(a, b, keys, what):
    for k in keys:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8)), what + ": " + k


@pytest.mark.parametrize("messages", ["i8", "f32"])
@pytest.mark.parametrize("n", SIZES)
def test_zero_rows_are_the_plain_mirror_and_one_row_is_a_smaller_code(q, n, messages):
    """all-zero rows: qldpc_polar_decode_host on all four outputs.  One row S for all frames: u, x and leaf of the code whose information set is the
    context's minus S.  int8 inputs of -1, 0 and 1 only: ties at every level"""
    rng = np.random.default_rng([n, messages == "i8", 32])
    N, F = 1 << n, 9
    for pos in codes(rng, n):
        llr = rng.integers(-1, 2, (F, N)).astype(np.int8) if messages == "i8" else inputs(rng, messages, F, N, 31)
        fz = R.pack(rng.integers(0, 2, (F, N), dtype=np.uint8))
        plain = q.polar_decode_host(n, pos, llr, fz, messages, 31, leaf=True)
        same(q.polar_decode_rows_host(n, pos, llr, np.zeros_like(fz), fz, messages, 31, leaf=True), plain, ("u", "info", "x", "leaf"), "zero rows n=%d" % n)
        S = rng.random(N) < 0.3
        rows = np.repeat(R.pack(S[None, :].astype(np.uint8)), F, axis=0)
        smaller = np.array([p for p in pos if not S[p]], np.int32)
        same(q.polar_decode_rows_host(n, pos, llr, rows, fz, messages, 31, leaf=True), q.polar_decode_host(n, smaller, llr, fz, messages, 31, leaf=True), ("u", "x", "leaf"),
             "one row n=%d" % n)


# ---- the ladder mirrors against the restatement ----------------------------------------------------------------------------------------------------

def ladder_case(rng, n, E_kind, B=12):
    """a code, a ladder of E entries (0, 1, 33 or K, at most K), a CRC, B blocks with mixed key lengths of which one is invalid"""
    pos = RR.code(rng, n, ("random", "clustered", "5g", "full")[int(rng.integers(0, 4))])
    K = len(pos)
    E = min(K, dict(zero=0, one=1, mid=33, all=K)[E_kind])
    xp = LD.ladder(rng, pos, E)
    crc_len, crc_poly = RR.crcs(K)[-1]
    ka, kbob, kb = RR.blocks(rng, n, B)
    kb[5] = (1 << n) + 1
    return pos, xp, E, crc_len, crc_poly, ka, kbob, kb


def start_counts(rng, B, E):
    """0, E, counts between, and one that is no count"""
    ex = rng.integers(0, E + 1, B).astype(np.int32)
    ex[0], ex[1], ex[2] = 0, E, (-1 if B % 2 else E + 1)
    return ex


ROUND_KEYS = ("status", "corrected", "keys", "extra", "decodes", "open_per_round")


@pytest.mark.parametrize("E_kind", ["zero", "one", "mid", "all"])
@pytest.mark.parametrize("n", [2, 5, 6, 8])
def test_ladder_mirrors_are_the_restatement(q, n, E_kind):
    """Alice's three rows, then Bob's rounds with every step and round count, from all-zero and from mixed start counts (one of them invalid),
    key lengths mixed (one of them invalid): status, corrected, keys, extra, decodes and open_per_round"""
    rng = np.random.default_rng([n, ["zero", "one", "mid", "all"].index(E_kind), 33])
    pos, xp, E, crc_len, crc_poly, ka, kbob, kb = ladder_case(rng, n, E_kind)
    B = ka.shape[0]
    for key_bits in (kb, None):
        got, want = q.polar_recon_encode_ladder_host(n, pos, xp, ka, key_bits, crc_len, crc_poly), LD.alice(n, pos, xp, ka, key_bits, crc_len, crc_poly)
        assert all(g.shape == w.shape and np.array_equal(g, w) for g, w in zip(got, want)), "alice n=%d E=%d" % (n, E)
        plain = q.polar_recon_encode_host(n, pos, ka, key_bits, crc_len, crc_poly)
        assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1])
    syn, crc, xb = q.polar_recon_encode_ladder_host(n, pos, xp, ka, kb, crc_len, crc_poly)
    k = 0
    for step in (1, 16, E + 5):
        for max_rounds in (1, 3):
            messages, maxq = ("i8", 31) if k % 2 else ("f32", 31)
            extra = np.zeros(B, np.int32) if k % 3 == 0 else start_counts(rng, B, E)
            k += 1
            args = dict(step=step, max_rounds=max_rounds, key_bits=kb, messages=messages, maxq=maxq, crc_len=crc_len, crc_poly=crc_poly)
            got = q.polar_recon_decode_rounds_host(n, pos, xp, kbob, syn, crc, xb, extra, **args)
            want = LD.rounds(n, pos, xp, kbob, syn, crc, xb, extra, **args)
            same(got, want, ROUND_KEYS, "n=%d E=%d step=%d rounds=%d %s" % (n, E, step, max_rounds, messages))
            assert got["status"][5] == ESIZE and got["decodes"][5] == 0 and np.array_equal(got["keys"][5], kbob[5])


def test_resume_reads_the_status_and_leaves_the_rest_alone(q):
    """resume = 1 against the restatement: only the EDECODE blocks are open; an OK block, an ESIZE block and a block of any other status keep their
    status, key and extra, whatever they are"""
    rng = np.random.default_rng(34)
    n = 6
    pos, xp, E, crc_len, crc_poly, ka, kbob, kb = ladder_case(rng, n, "mid")
    syn, crc, xb = q.polar_recon_encode_ladder_host(n, pos, xp, ka, kb, crc_len, crc_poly)
    B = ka.shape[0]
    status = np.array([EDECODE, OK, ESIZE, 77] * (B // 4), np.int32)
    extra = start_counts(rng, B, E)
    extra[3] = -40                                                 # not a candidate: not looked at
    args = dict(step=7, max_rounds=2, key_bits=kb, resume=True, status=status, messages="i8", crc_len=crc_len, crc_poly=crc_poly)
    got = q.polar_recon_decode_rounds_host(n, pos, xp, kbob, syn, crc, xb, extra, **args)
    same(got, LD.rounds(n, pos, xp, kbob, syn, crc, xb, extra, **args), ROUND_KEYS, "resume")
    kept = status != EDECODE
    assert np.array_equal(got["status"][kept], status[kept]) and np.array_equal(got["extra"][kept], extra[kept]) and np.array_equal(got["keys"][kept], kbob[kept])
    assert not got["decodes"][kept].any() and got["decodes"][~kept].sum() == got["open_per_round"].sum() > 0


# ---- equalities of the rule ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("messages", ["i8", "f32"])
@pytest.mark.parametrize("n", [1, 4, 5, 7, 10])
def test_one_round_from_zero_is_the_plain_session(q, n, messages):
    rng = np.random.default_rng([n, 35])
    pos, xp, E, crc_len, crc_poly, ka, kbob, kb = ladder_case(rng, n, "mid", 24)
    syn, crc, xb = q.polar_recon_encode_ladder_host(n, pos, xp, ka, kb, crc_len, crc_poly)
    got = q.polar_recon_decode_rounds_host(n, pos, xp, kbob, syn, crc, xb, np.zeros(24, np.int32), 16, 1, kb, messages=messages, crc_len=crc_len, crc_poly=crc_poly)
    same(got, q.polar_recon_decode_host(n, pos, kbob, syn, crc, kb, messages, crc_len=crc_len, crc_poly=crc_poly), ("keys", "status", "corrected"), "n=%d" % n)
    assert not got["extra"].any() and np.array_equal(got["decodes"], (got["status"] != ESIZE).astype(np.int32))


def noisy_blocks(rng, n, B, rate=0.08):
    N = 1 << n
    x = rng.integers(0, 2, (B, N), dtype=np.uint8)
    return R.pack(x), R.pack(x ^ (rng.random((B, N)) < rate).astype(np.uint8))


@pytest.mark.parametrize("step,E_all", [(1, True), (5, False)])
def test_rounds_in_one_call_are_single_round_calls(q, step, E_all):
    """R rounds in one call = R calls with max_rounds = 1 and resume = 1, the caller raising extra between them.  With a long ladder and step 1 no
    block reaches its end, and the decode counts agree too"""
    rng = np.random.default_rng([step, 36])
    n, B, rounds = 8, 40, 3
    pos = RR.code(rng, n, "5g")
    E = len(pos) if E_all else 7
    xp = pos[:E].copy()
    ka, kbob = noisy_blocks(rng, n, B)
    syn, crc, xb = q.polar_recon_encode_ladder_host(n, pos, xp, ka, None, *RR.CRC32)
    code = dict(messages="f32", crc_len=32, crc_poly=RR.CRC32[1])
    whole = q.polar_recon_decode_rounds_host(n, pos, xp, kbob, syn, crc, xb, np.zeros(B, np.int32), step, rounds, **code)
    assert whole["open_per_round"][1] > 0 and (whole["status"] == OK).any()
    part = q.polar_recon_decode_rounds_host(n, pos, xp, kbob, syn, crc, xb, np.zeros(B, np.int32), step, 1, **code)
    per_round, decodes, corrected = [int(part["open_per_round"][0])], part["decodes"].copy(), part["corrected"].copy()
    for _ in range(rounds - 1):
        raised = np.where((part["status"] == EDECODE) & (part["extra"] < E), np.minimum(E, part["extra"] + step), part["extra"]).astype(np.int32)
        part = q.polar_recon_decode_rounds_host(n, pos, xp, part["keys"], syn, crc, xb, raised, step, 1, resume=True, status=part["status"], **code)
        per_round.append(int(part["open_per_round"][0]))
        decodes += part["decodes"]
        corrected = np.where(part["decodes"] > 0, part["corrected"], corrected)      # a block left alone keeps what the call before gave it
    same(part, whole, ("keys", "status", "extra"), "step=%d" % step)
    assert np.array_equal(corrected, whole["corrected"])
    if E_all:
        assert per_round == whole["open_per_round"].tolist() and np.array_equal(decodes, whole["decodes"])


@pytest.mark.parametrize("messages", ["i8", "f32"])
def test_every_information_bit_disclosed_is_always_ok(q, messages):
    """extra = E = K: Bob is told u whole, so every block of a valid length is OK whatever the noise, and corrected is the distance to Alice's key"""
    rng = np.random.default_rng(37)
    n, B = 7, 20
    N = 1 << n
    pos = RR.code(rng, n, "random")
    xp = LD.ladder(rng, pos, len(pos))
    ka, kbob, kb = RR.blocks(rng, n, B)
    kbob = kbob ^ rng.integers(0, 1 << 32, kbob.shape, dtype=np.uint64).astype(np.uint32)      # half of Bob's bits are wrong
    kb[3] = 0
    syn, crc, xb = q.polar_recon_encode_ladder_host(n, pos, xp, ka, kb, 11, 0x621)
    got = q.polar_recon_decode_rounds_host(n, pos, xp, kbob, syn, crc, xb, np.full(B, len(pos), np.int32), 1, 1, kb, messages=messages, crc_len=11, crc_poly=0x621)
    ok = kb >= 1
    mask = RR.key_mask(kb.astype(np.int64), ok, N)
    assert np.array_equal(got["status"], np.where(ok, OK, ESIZE))
    assert np.array_equal(R.unpack(got["keys"], N)[ok], (R.unpack(ka, N) * mask)[ok])
    assert np.array_equal(got["corrected"][ok], ((R.unpack(ka, N) ^ R.unpack(kbob, N)) * mask).sum(axis=1)[ok])


def test_bits_bob_does_not_hold_yet_change_nothing(q):
    rng = np.random.default_rng(38)
    n, B, E = 8, 30, 70
    pos = RR.code(rng, n, "5g")
    xp = pos[:E].copy()
    ka, kbob = noisy_blocks(rng, n, B)
    syn, crc, xb = q.polar_recon_encode_ladder_host(n, pos, xp, ka, None, 11, 0x621)
    extra = rng.integers(0, 20, B).astype(np.int32)
    step, rounds = 9, 3
    reach = np.minimum(E, extra + step * (rounds - 1))            # the furthest count a block can be decoded at
    junk = R.unpack(xb, E) ^ ((np.arange(E)[None, :] >= reach[:, None]) & (rng.random((B, E)) < 0.5)).astype(np.uint8)
    args = dict(step=step, max_rounds=rounds, messages="i8", crc_len=11, crc_poly=0x621)
    a = q.polar_recon_decode_rounds_host(n, pos, xp, kbob, syn, crc, xb, extra, **args)
    b = q.polar_recon_decode_rounds_host(n, pos, xp, kbob, syn, crc, R.pack(junk), extra, **args)
    assert (R.pack(junk) != xb).any()
    same(a, b, ROUND_KEYS, "junk past the count")


# ---- the operating point ---------------------------------------------------------------------------------------------------------------------------

def test_operating_point_with_a_crc32_verdict(q):
    """N = 1 024, K = 512 in the 5G order, 2 000 keys through a BSC of 6 %, float messages, step 16, 5 rounds, the ladder the least reliable
    information positions first.  The cap on the last round's count is the issue's condition (a quarter of what round 0 left open; the genie
    restatement gives 26 of 151), not a measurement"""
    n, pos, xp, ka, kbob = LD.operating_point()
    B, N, K = ka.shape[0], 1024, 512
    syn, crc, xb = q.polar_recon_encode_ladder_host(n, pos, xp, ka, None, *RR.CRC32)
    got = q.polar_recon_decode_rounds_host(n, pos, xp, kbob, syn, crc, xb, np.zeros(B, np.int32), 16, 5, messages="f32", crc_len=32, crc_poly=RR.CRC32[1])
    per_round = got["open_per_round"].tolist()
    print("open per round %s, still failed %d, extra bits %d" % (per_round, int((got["status"] != OK).sum()), int(got["extra"].sum())))
    assert per_round[0] == B and all(a >= b for a, b in zip(per_round, per_round[1:]))
    assert per_round[1] > 0 and per_round[-1] < per_round[1] / 4.0
    done = got["status"] == OK
    assert np.array_equal(got["keys"][done], ka[done]) and set(got["status"].tolist()) <= {OK, EDECODE}
    assert np.array_equal(got["extra"], 16 * (got["decodes"] - 1))
    leak = (N - K + 32) + got["extra"].astype(np.int64)           # per block: the plain session's leak and the bits disclosed to it
    assert int(leak.sum()) == B * (N - K + 32) + 16 * int(sum(per_round[1:]))


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------

def status_of(q, fn, *args, **kw):
    with pytest.raises(q.QldpcError) as e:
        fn(*args, **kw)
    assert str(e.value)
    return e.value.status


def test_refusals_of_the_rows_mirror(q):
    z = np.zeros((1, 8), np.int8)
    w = np.zeros((1, 1), np.uint32)
    assert status_of(q, q.polar_decode_rows_host, 0, [], np.zeros((1, 1), np.int8), w) == ESIZE
    assert status_of(q, q.polar_decode_rows_host, 21, [], np.zeros((1, 1), np.int8), w) == ESIZE
    assert status_of(q, q.polar_decode_rows_host, 3, [8], z, w) == ESIZE
    assert status_of(q, q.polar_decode_rows_host, 3, [1, 1], z, w) == EINVAL
    assert status_of(q, q.polar_decode_rows_host, 3, [1], z, w, maxq=127) == ESIZE
    assert status_of(q, q.polar_decode_rows_host, 3, [1], z, w, messages="f16") == EINVAL
    assert status_of(q, q.polar_decode_rows_host, 3, [1], z, np.zeros((2, 1), np.uint32)) == ESIZE
    assert status_of(q, q.polar_decode_rows_host, 3, [1], z, None) == EINVAL and "frozen_rows" in str(pytest.raises(q.QldpcError, q.polar_decode_rows_host, 3, [1], z, None).value)
    L = q._L
    assert L.qldpc_polar_decode_rows_host(3, 0, None, 0, 31, 1, None, None, w.ctypes.data_as(C.POINTER(C.c_uint32)), None, None, None, None) == EINVAL
    assert L.qldpc_polar_decode_rows_host(3, 0, None, 0, 31, -1, None, None, None, None, None, None, None) == EINVAL
    assert L.qldpc_polar_decode_rows_host(3, 0, None, 0, 31, 0, None, None, None, None, None, None, None) == OK      # no frames: nothing to do


def test_refusals_of_the_ladder_mirrors(q):
    n, pos = 4, np.array([3, 5, 9, 12, 15], np.int32)
    keys, syn, crc = np.zeros((2, 1), np.uint32), np.zeros((2, 1), np.uint32), np.zeros(2, np.uint32)
    xb, extra = np.zeros((2, 1), np.uint32), np.zeros(2, np.int32)
    enc = lambda xp, **kw: q.polar_recon_encode_ladder_host(n, pos, xp, keys, None, kw.pop("crc_len", 3), 3, **kw)
    assert status_of(q, enc, [3, 5, 9, 12, 15, 1]) == ESIZE                                         # more entries than information positions
    assert status_of(q, enc, [3, 3]) == EINVAL                                                     # an entry twice
    assert status_of(q, enc, [4]) == EINVAL                                                        # a frozen position
    assert status_of(q, enc, [16]) == EINVAL and status_of(q, enc, [-1]) == EINVAL                # no position
    assert status_of(q, enc, [3], crc_len=0) == ESIZE and status_of(q, enc, [3], crc_len=6) == ESIZE
    assert status_of(q, q.polar_recon_encode_ladder_host, 0, [], [], keys) == ESIZE
    assert [a.shape for a in enc([])] == [(2, 1), (2,), (2, 0)]
    dec = lambda xp=(3, 9), **kw: q.polar_recon_decode_rounds_host(n, pos, xp, keys, syn, crc, xb if len(xp) else None, kw.pop("extra", extra), kw.pop("step", 1),
                                                                     kw.pop("max_rounds", 1), crc_len=kw.pop("crc_len", 3), crc_poly=3, **kw)
    assert status_of(q, dec, step=0) == EINVAL and status_of(q, dec, max_rounds=0) == EINVAL and status_of(q, dec, resume=2, status=extra) == EINVAL
    assert status_of(q, dec, (3, 5, 9, 12, 15, 1)) == ESIZE and status_of(q, dec, (3, 3)) == EINVAL and status_of(q, dec, (4,)) == EINVAL
    assert status_of(q, dec, crc_len=0) == ESIZE and status_of(q, dec, messages="f16") == EINVAL and status_of(q, dec, maxq=127) == ESIZE
    assert status_of(q, dec, prior=0.0) == EINVAL and status_of(q, dec, pin=32.0) == EINVAL
    assert status_of(q, dec, resume=True) == EINVAL                                                # the binding's: resume without a status
    assert dec(())["status"].tolist() == dec()["status"].tolist()
    # the raw calls: a NULL required pointer, a negative block count, no blocks
    L, ip, up = q._L, C.POINTER(C.c_int), C.POINTER(C.c_uint32)
    P = lambda a, t: a.ctypes.data_as(t)
    xp = np.array([3, 9], np.int32)
    st = np.zeros(2, np.int32)

    def raw(B, keys_, crc_, xb_, extra_, status_, syn_=syn):
        return L.qldpc_polar_recon_decode_rounds_host(n, 5, P(pos, ip), 0, 31, 3, 3, 1.0, 31.0, 2, P(xp, ip), B, keys_, None, P(syn_, up) if syn_ is not None else None,
                                                      crc_, xb_, extra_, 1, 1, 0, status_, None, None, None)
    full = (P(keys, up), P(crc, up), P(xb, up), P(extra, ip), P(st, ip))
    assert raw(2, *full) == OK
    for k in range(5):
        assert raw(2, *[None if j == k else a for j, a in enumerate(full)]) == EINVAL, k
    assert raw(2, *full, syn_=None) == EINVAL
    assert raw(-1, *full) == EINVAL and raw(0, None, None, None, None, None) == OK
    assert L.qldpc_polar_recon_encode_ladder_host(n, 5, P(pos, ip), 3, 3, 2, P(xp, ip), 2, P(keys, up), None, P(syn, up), P(crc, up), None) == EINVAL
    assert L.qldpc_polar_recon_encode_ladder_host(n, 5, P(pos, ip), 3, 3, 2, None, 2, P(keys, up), None, P(syn, up), P(crc, up), P(xb, up)) == EINVAL
    assert L.qldpc_polar_recon_encode_ladder_host(n, 5, P(pos, ip), 3, 3, 2, P(xp, ip), 2, None, None, P(syn, up), P(crc, up), P(xb, up)) == EINVAL


def test_ladder_extra_is_its_formula(q):
    """clamp(ceil(f h2(qber) key_bits) - (N - K), 0, E) at a handful of points, both clamps and the refusals"""
    for n, K, E, kb, qber, f in ((10, 512, 128, 1024, 0.06, 1.2), (10, 512, 128, 1024, 0.07, 1.3), (10, 512, 128, 1024, 0.02, 1.2), (10, 512, 128, 1024, 0.11, 1.5),
                                 (10, 512, 128, 700, 0.09, 1.2), (10, 700, 0, 1024, 0.1, 1.2), (5, 20, 20, 32, 0.5, 1.0), (16, 40000, 9000, 65536, 0.05, 1.1),
                                 (10, 512, 128, 1024, 0.0, 1.2), (10, 512, 128, 1, 0.25, 0.0)):
        assert q.polar_recon_ladder_extra(n, K, E, kb, qber, f) == LD.start_extra(n, K, E, kb, qber, f), (n, K, E, kb, qber, f)
    assert q.polar_recon_ladder_extra(10, 512, 128, 1024, 0.02, 1.2) == 0 and q.polar_recon_ladder_extra(10, 512, 128, 1024, 0.11, 1.5) == 128
    assert 0 < q.polar_recon_ladder_extra(10, 512, 128, 1024, 0.07, 1.4) < 128
    for args, want in (((0, 0, 0, 1, 0.1, 1.0), ESIZE), ((21, 0, 0, 1, 0.1, 1.0), ESIZE), ((4, 17, 0, 1, 0.1, 1.0), ESIZE), ((4, 8, 9, 1, 0.1, 1.0), ESIZE),
                       ((4, 8, -1, 1, 0.1, 1.0), ESIZE), ((4, 8, 8, 0, 0.1, 1.0), ESIZE), ((4, 8, 8, 17, 0.1, 1.0), ESIZE), ((4, 8, 8, 16, -0.1, 1.0), EINVAL),
                       ((4, 8, 8, 16, 0.6, 1.0), EINVAL), ((4, 8, 8, 16, float("nan"), 1.0), EINVAL), ((4, 8, 8, 16, 0.1, -1.0), EINVAL),
                       ((4, 8, 8, 16, 0.1, float("inf")), EINVAL)):
        assert status_of(q, q.polar_recon_ladder_extra, *args) == want, args


# ---- the sanitizer program ---------------------------------------------------------------------------------------------------------------------------

def test_host_code_under_asan_ubsan(tmp_path):
    """the new mirrors at every size up to 2^9 with every row malloc'ed at its exact size, and their refusals, as a stand-alone program (nothing
    loaded into Python is sanitised)"""
    exe = str(tmp_path / "polar_ladder_sanitize")
    csrc = os.path.join(ROOT, "qcrypto-ldpc_amd", "csrc")
    units = ["qldpc_polar_host.c", "qldpc_polar_ssc_host.c", "qldpc_polar_wide_host.c", "qldpc_polar_list_host.c", "qldpc_polar_recon_host.c", "qldpc_polar_ladder_host.c"]
    subprocess.check_call(["gcc", "-std=gnu11", "-g", "-O1", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-Wall", "-Wextra",
                           "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-o", exe, os.path.join(ROOT, "tests", "c", "polar_ladder_sanitize.c")] +
                          [os.path.join(csrc, u) for u in units] + ["-lm"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0 and "sanitizer pass ok" in r.stdout, r.stdout + r.stderr
