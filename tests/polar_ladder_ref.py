"""The restatement the incremental-freezing tests hold the library to (qldpc_polar_ladder_core.h's header), in numpy on unpacked
bits and whole arrays.  The rows decode is polar_ref.decode run once per group of frames that share a frozen set.  The ladder rule is restated
from its text: the rank of a position in the disclosure order, the values scattered to the added positions, and the round loop.  It stands on
polar_ref.py (encode, decode, pack, unpack), on polar_list_ref.py's register CRC and on polar_recon_ref.py's key masks; it calls no C mirror.
Not a test module."""
import numpy as np

import polar_list_ref as LR
import polar_recon_ref as PR
import polar_ref as R

OK, ESIZE, EDECODE = PR.OK, PR.ESIZE, PR.EDECODE


# ---- the rows decode -----------------------------------------------------------------------------------------------------------------------

def decode_rows(llr, frozen_mask, rows, frozen_values=None, messages="i8", maxq=31):
    """llr [F, N]; frozen_mask bool [N] the code's; rows bool / uint8 [F, N] what each frame adds; frozen_values uint8 [F, N] or None
    -> (u, x, leaf) as polar_ref.decode gives them"""
    llr = np.asarray(llr)
    F, N = llr.shape
    eff = np.asarray(frozen_mask, bool)[None, :] | np.asarray(rows).astype(bool)
    sets, group = np.unique(eff, axis=0, return_inverse=True)
    group = np.asarray(group).reshape(-1)
    u, x, leaf = np.zeros((F, N), np.uint8), np.zeros((F, N), np.uint8), None
    for g in range(len(sets)):
        sel = np.flatnonzero(group == g)
        ug, xg, lg = R.decode(llr[sel], sets[g], None if frozen_values is None else np.asarray(frozen_values)[sel], messages, maxq)
        if leaf is None:
            leaf = np.zeros((F, N), lg.dtype)
        u[sel], x[sel], leaf[sel] = ug, xg, lg
    if leaf is None:
        leaf = np.zeros((F, N), np.int64 if messages == "i8" else np.float32)
    return u, x, leaf


# ---- the ladder ------------------------------------------------------------------------------------------------------------------------------

def rank_table(N, extra_pos):
    """rank int64 [N]: m where extra_pos[m] is the position, a number above every count elsewhere"""
    rank = np.full(N, 1 << 40, np.int64)
    rank[np.asarray(extra_pos, np.int64)] = np.arange(len(extra_pos))
    return rank


def alice(n, pos, extra_pos, keys, key_bits, crc_len, crc_poly):
    """keys uint32 [B, W] -> (syndrome, crc, extra_bits uint32 [B, ceil(E / 32)])"""
    N = 1 << n
    B = keys.shape[0]
    kb, ok = PR.valid(key_bits, B, N)
    u = R.encode(R.unpack(keys, N) * PR.key_mask(kb, ok, N))
    frozen = np.ones(N, bool)
    frozen[pos] = False
    syn = R.pack(u[:, frozen]) if frozen.any() else np.zeros((B, 0), np.uint32)
    xb = R.pack(u[:, np.asarray(extra_pos, np.int64)]) if len(extra_pos) else np.zeros((B, 0), np.uint32)
    return syn, LR.crc_bits(u[:, pos], crc_len, crc_poly), xb


def start_extra(n, K, E, key_bits, qber, f):
    h2 = 0.0 if qber <= 0.0 or qber >= 1.0 else -(qber * np.log2(qber) + (1.0 - qber) * np.log2(1.0 - qber))
    return int(min(max(np.ceil(f * h2 * key_bits) - ((1 << n) - K), 0), E))


def rounds(n, pos, extra_pos, keys, syndrome, crc, extra_bits, extra, step, max_rounds, key_bits=None, resume=False, status=None, messages="i8", maxq=31,
           crc_len=0, crc_poly=0, prior_level=None, pin_level=None):
    """Bob's rounds -> dict(keys, status, corrected, extra, decodes, open_per_round); with resume the rows of the blocks that are not open come
    back as given (corrected: -1)"""
    N, K, E = 1 << n, len(pos), len(extra_pos)
    keys = np.array(keys, np.uint32)
    B = keys.shape[0]
    kb, ok_kb = PR.valid(key_bits, B, N)
    extra = np.array(extra, np.int64)
    status = np.zeros(B, np.int32) if status is None else np.array(status, np.int32)
    corrected, decodes, per_round = np.full(B, -1, np.int32), np.zeros(B, np.int32), np.zeros(max_rounds, np.int32)
    candidate = (status == EDECODE) if resume else np.ones(B, bool)
    good_args = ok_kb & (extra >= 0) & (extra <= E)
    status[candidate & ~good_args] = ESIZE
    is_open = candidate & good_args
    p, pin = PR.default_levels(messages, maxq, prior_level, pin_level)
    dt = np.int8 if messages == "i8" else np.float32
    frozen = np.ones(N, bool)
    frozen[pos] = False
    rank = rank_table(N, extra_pos)
    syn_bits = R.unpack(syndrome, int(frozen.sum())) if frozen.any() else np.zeros((B, 0), np.uint8)
    xb_bits = R.unpack(extra_bits, E) if E else np.zeros((B, 0), np.uint8)
    for t in range(max_rounds):
        o = np.flatnonzero(is_open)
        if not len(o):
            break
        per_round[t] = len(o)
        decodes[o] += 1
        mask = PR.key_mask(kb[o], ok_kb[o], N)
        y = R.unpack(keys[o], N).astype(bool)
        llr = np.where(mask, np.where(y, dt(-p), dt(p)), dt(pin)).astype(dt)
        added = rank[None, :] < extra[o, None]                    # bool [n_open, N]: the positions each block's count adds
        fv = np.zeros((len(o), N), np.uint8)
        if frozen.any():
            fv[:, frozen] = syn_bits[o]
        if E:
            looked_at = np.arange(E)[None, :] < extra[o, None]    # Bob holds the first extra[b] bits of a row and no more
            fv[:, np.asarray(extra_pos, np.int64)] = xb_bits[o] * looked_at
        u, x, _ = decode_rows(llr, frozen, added, fv, messages, maxq)
        match = LR.crc_bits(u[:, pos], crc_len, crc_poly) == np.asarray(crc, np.uint32)[o]
        xh = x.astype(bool)
        good = match & ~(xh & ~mask).any(axis=1)
        status[o] = np.where(good, OK, EDECODE)
        corrected[o] = np.where(good, ((xh ^ y) & mask).sum(axis=1), -1)
        keys[o[good]] = R.pack(x[good])
        again = ~good & (extra[o] < E) & (t + 1 < max_rounds)
        extra[o[again]] = np.minimum(E, extra[o[again]] + step)
        is_open[:] = False
        is_open[o[again]] = True
    return dict(keys=keys, status=status, corrected=corrected, extra=extra.astype(np.int32), decodes=decodes, open_per_round=per_round)


# ---- what the two suites share -------------------------------------------------------------------------------------------------------------------

def ladder(rng, pos, E):
    """E of the information positions in a random order"""
    return rng.permutation(np.asarray(pos, np.int32))[:E].astype(np.int32)


def operating_point(B=2000, qber=0.06, seed=20263):
    """N = 1 024, K = 512 in the 5G order, the ladder its 128 least reliable information positions, least reliable first: Alice's keys and Bob's
    through a BSC -> (n, pos, extra_pos, alice uint32 [B, 32], bob uint32 [B, 32])"""
    n, N, K = 10, 1024, 512
    pos = R.nr_order(N)[N - K:].astype(np.int32)
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 2, (B, N), dtype=np.uint8)
    y = x ^ (rng.random((B, N)) < qber).astype(np.uint8)
    return n, pos, pos[:128].copy(), R.pack(x), R.pack(y)
