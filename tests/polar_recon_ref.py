"""The restatement the polar reconciliation tests hold the library to: the rule of a session (qldpc_polar_recon_core.h's header)
in numpy on unpacked bits, whole arrays at a time, with no position table and no rank: masks and fancy indexing only.  It stands on polar_ref.py's
encode / pack / unpack and on the library's polar_crc_host (tested against its own restatement in test_polar_list_host.py); the decoder between
prior and verdict is the library's host mirror of the decoder asked for, each of which has a restatement of its own.  Not a test module."""
import numpy as np

import polar_ref as R

OK, ESIZE, EDECODE = 0, -6, -9
CRC32 = (32, 0x04C11DB7)


def valid(key_bits, B, N):
    """key_bits int [B] or None -> (kb int64 [B], valid bool [B]); None means N everywhere"""
    kb = np.full(B, N, np.int64) if key_bits is None else np.asarray(key_bits, np.int64)
    return kb, (kb >= 1) & (kb <= N)


def key_mask(kb, ok, N):
    """bool [B, N]: the positions below key_bits; none where key_bits is out of range"""
    return (np.arange(N)[None, :] < kb[:, None]) & ok[:, None]


def alice(q, n, pos, keys, key_bits, crc_len, crc_poly):
    """keys uint32 [B, W] -> (syndrome uint32 [B, ceil((N - K) / 32)], crc uint32 [B])"""
    N = 1 << n
    B = keys.shape[0]
    kb, ok = valid(key_bits, B, N)
    x = R.unpack(keys, N) * key_mask(kb, ok, N)
    u = R.encode(x)
    frozen = np.ones(N, bool)
    frozen[pos] = False
    syn = R.pack(u[:, frozen]) if frozen.any() else np.zeros((B, 0), np.uint32)
    crc = q.polar_crc_host(crc_len, crc_poly, R.pack(u[:, pos]), len(pos))
    return syn, crc


def prior(n, pos, keys, syndrome, key_bits, messages, prior_level, pin_level):
    """-> (llr [B, N] int8 or float32, frozen uint32 [B, W])"""
    N = 1 << n
    B = keys.shape[0]
    kb, ok = valid(key_bits, B, N)
    y = R.unpack(keys, N).astype(bool)
    dt = np.int8 if messages == "i8" else np.float32
    llr = np.where(key_mask(kb, ok, N), np.where(y, dt(-prior_level), dt(prior_level)), dt(pin_level)).astype(dt)
    frozen = np.ones(N, bool)
    frozen[pos] = False
    fv = np.zeros((B, N), np.uint8)
    if frozen.any():
        fv[:, frozen] = R.unpack(syndrome, int(frozen.sum()))
    return llr, R.pack(fv)


def verdict(q, n, K, info, x, keys, key_bits, crc, pick, crc_len, crc_poly):
    """info uint32 [B, ceil(K/32)], x uint32 [B, W] decoded rows, keys uint32 [B, W] Bob's -> dict(keys, status, corrected)"""
    N = 1 << n
    B = keys.shape[0]
    kb, ok_kb = valid(key_bits, B, N)
    mask = key_mask(kb, ok_kb, N)
    xh, y = R.unpack(x, N).astype(bool), R.unpack(keys, N).astype(bool)
    match = (np.asarray(pick) >= 0) if pick is not None else (q.polar_crc_host(crc_len, crc_poly, info, K) == np.asarray(crc, np.uint32))
    good = ok_kb & match & ~(xh & ~mask).any(axis=1)
    status = np.where(~ok_kb, ESIZE, np.where(good, OK, EDECODE)).astype(np.int32)
    corrected = np.where(good, ((xh ^ y) & mask).sum(axis=1), -1).astype(np.int32)
    out = np.where(good[:, None], R.pack(xh.astype(np.uint8)), np.ascontiguousarray(keys, dtype=np.uint32))
    return dict(keys=out.astype(np.uint32), status=status, corrected=corrected)


def default_levels(messages, maxq, prior_level=None, pin_level=None):
    return (1 if prior_level is None else prior_level), ((maxq if messages == "i8" else float(1 << 24)) if pin_level is None else pin_level)


def bob(q, n, pos, keys, syndrome, crc, key_bits, messages, maxq, decoder, crc_len, crc_poly, prior_level=None, pin_level=None):
    """decoder: "sc", "ssc", "wide", or a list size -> dict(keys, status, corrected, pick (list only), llr, frozen)"""
    p, pin = default_levels(messages, maxq, prior_level, pin_level)
    llr, frozen = prior(n, pos, keys, syndrome, key_bits, messages, p, pin)
    pick = None
    if isinstance(decoder, int):
        dec = q.polar_list_decode_host(n, pos, llr, frozen, crc, messages, maxq, decoder, crc_len, crc_poly, want=("info", "x", "pick"))
        pick = dec["pick"]
    else:
        fn = dict(sc=q.polar_decode_host, ssc=q.polar_decode_ssc_host, wide=q.polar_decode_wide_host)[decoder]
        dec = fn(n, pos, llr, frozen, messages, maxq)
    out = verdict(q, n, len(pos), dec["info"], dec["x"], keys, key_bits, crc, pick, crc_len, crc_poly)
    out.update(llr=llr, frozen=frozen)
    if pick is not None:
        out["pick"] = pick
    return out


# ---- what the two suites share: codes, blocks and the constructed rows of the verdict's branches ------------------------------------------------

CODES = ("random", "clustered", "5g", "full")


def code(rng, n, kind):
    """info_pos of a code of N = 2^n: random positions in a random order; one run of neighbouring positions; the most reliable positions of the
    5G order (the polarization-weight order above N = 1024), most reliable last; K = N.  From n = 6 on neither K nor N - K is a multiple of 32
    (but for K = N)"""
    N = 1 << n
    if kind == "full":
        return np.arange(N, dtype=np.int32)
    K = max(1, N // 2 + (5 if n >= 6 else 0) + (int(rng.integers(0, 3)) if n >= 3 else 0))
    K = min(K, N - 1) if N > 1 else 1
    if n >= 6 and (K % 32 == 0 or (N - K) % 32 == 0):
        K += 1
    if kind == "random":
        return rng.permutation(N)[:K].astype(np.int32)
    if kind == "clustered":
        start = int(rng.integers(0, N - K + 1))
        return np.arange(start, start + K, dtype=np.int32)
    if N <= 1024:
        return R.nr_order(N)[N - K:].astype(np.int32)
    w = np.zeros(N)
    for j in range(n):
        w += ((np.arange(N) >> j) & 1) * 2.0 ** (j / 4.0)
    return np.argsort(w, kind="stable")[N - K:].astype(np.int32)


def crcs(K):
    """the CRCs of the suites that fit K information bits: 1 bit, CRC 11 (0x621), 32 bits"""
    return [c for c in ((1, 1), (11, 0x621), CRC32) if c[0] <= K]


def blocks(rng, n, B):
    """B blocks of Alice's and Bob's keys (uint32 [B, W], junk past key_bits on both sides) and key_bits int32 [B]: the key lengths N, N - 1, N - 37
    (where that is a length) and 1 in turn, and the three kinds of block in turn against them: no flips, 2 % flips, 25 % flips"""
    N = 1 << n
    lengths = [k for k in (N, N - 1, N - 37, 1) if k >= 1]
    kb = np.array([lengths[b % len(lengths)] for b in range(B)], np.int32)
    x = rng.integers(0, 2, (B, N), dtype=np.uint8)
    rate = np.array([(0.0, 0.02, 0.25)[(b // len(lengths)) % 3] for b in range(B)])
    flips = (rng.random((B, N)) < rate[:, None]).astype(np.uint8)
    junk = np.arange(N)[None, :] >= kb[:, None]
    alice_keys = np.where(junk, rng.integers(0, 2, (B, N), dtype=np.uint8), x)
    bob_keys = np.where(junk, rng.integers(0, 2, (B, N), dtype=np.uint8), x ^ flips)
    top = np.uint32(0xffffffff) if N >= 32 else np.uint32((0xffffffff << (32 - N)) & 0xffffffff)
    spare = rng.integers(0, 1 << 32, (2, B, 1), dtype=np.uint64).astype(np.uint32) & ~top      # bits past N of the only word of a short row
    return R.pack(alice_keys) | spare[0], R.pack(bob_keys) | spare[1], kb


def verdict_rows(q, rng, n, K, key_bits, crc_len, crc_poly):
    """the constructed rows that drive the verdict through each branch, five blocks of key length key_bits (1 <= key_bits <= N):
       0  remainder equal, pad clean           -> OK, the key becomes x^, corrected = the flips
       1  remainder equal, one pad bit set     -> EDECODE, the key untouched   (pad clean too where key_bits = N: then OK)
       2  remainder different (pick >= 0)      -> EDECODE without pick, OK with it
       3  remainder equal, pick = -1           -> EDECODE with pick, OK without it
       4  key_bits out of range                -> ESIZE
    -> dict(info, x, keys, key_bits, crc, pick) and the expected (status without pick, status with pick, flips of block 0)"""
    N = 1 << n
    B = 5
    xh = rng.integers(0, 2, (B, N), dtype=np.uint8)
    xh[:, key_bits:] = 0
    if key_bits < N:
        xh[1, int(rng.integers(key_bits, N))] = 1
    y = xh ^ (rng.random((B, N)) < 0.1).astype(np.uint8)
    y[:, key_bits:] = rng.integers(0, 2, (B, N - key_bits), dtype=np.uint8)
    info = rng.integers(0, 2, (B, K), dtype=np.uint8)
    rows = R.pack(info)
    crc = q.polar_crc_host(crc_len, crc_poly, rows, K)
    crc[2] ^= 1
    kb = np.full(B, key_bits, np.int32)
    kb[4] = (0, N + 1, -5)[key_bits % 3]
    pad1 = OK if key_bits == N else EDECODE
    want_sc = np.array([OK, pad1, EDECODE, OK, ESIZE], np.int32)
    want_list = np.array([OK, pad1, OK, EDECODE, ESIZE], np.int32)
    flips = (xh ^ y)[:, :key_bits].sum(axis=1).astype(np.int32)
    return (dict(info=rows, x=R.pack(xh), keys=R.pack(y), key_bits=kb, crc=crc, pick=np.array([0, 1, 2, -1, 0], np.int32)), want_sc, want_list, flips)
