"""The restatement the SC-Flip tests hold the library to (qldpc_polar_flip_core.h's header), in numpy on unpacked bits: the key
of a leaf and its order as a stable argsort on (magnitude, position), the trials as frames of polar_ladder_ref.decode_rows, settle and the resume
rule.  It stands on polar_ladder_ref.py (the rows decode, the rank table, the first pass) and through it on polar_ref.py, polar_list_ref.py and
polar_recon_ref.py; it calls no C mirror.  Not a test module."""
import numpy as np

import polar_ladder_ref as LD
import polar_list_ref as LR
import polar_recon_ref as PR
import polar_ref as R

OK, ESIZE, EDECODE = PR.OK, PR.ESIZE, PR.EDECODE


def magnitude(leaf):
    """int leaves: |leaf|; float32 leaves: the bit pattern of |leaf| (monotone for finite values, 0 for both zeros)"""
    leaf = np.asarray(leaf)
    if leaf.dtype == np.float32:
        return (np.ascontiguousarray(leaf).view(np.uint32) & np.uint32(0x7fffffff)).astype(np.int64)
    return np.abs(leaf.astype(np.int64))


def select(leaf, frozen_mask, n_flips, rank=None, extra=None):
    """leaf [F, N]; frozen_mask bool [N]; rank int [N] and extra int [F], or None -> pos int32 [F, n_flips]: the candidates in ascending
    (magnitude, position), -1 where there are fewer"""
    leaf = np.asarray(leaf)
    F, N = leaf.shape
    cand = np.repeat(~np.asarray(frozen_mask, bool)[None, :], F, axis=0)
    if rank is not None:
        cand &= np.asarray(rank, np.int64)[None, :] >= (np.zeros(F, np.int64) if extra is None else np.asarray(extra, np.int64))[:, None]
    mag = magnitude(leaf)
    pos = np.full((F, n_flips), -1, np.int32)
    for f in range(F):
        idx = np.flatnonzero(cand[f])                             # ascending positions: a stable sort leaves ties to the lower one
        best = idx[np.argsort(mag[f, idx], kind="stable")][:n_flips]
        pos[f, :len(best)] = best
    return pos


def flip(n, pos, keys, syndrome, crc, n_flips, extra_pos=(), extra_bits=None, extra=None, key_bits=None, resume=False, status=None, messages="i8", maxq=31,
         crc_len=0, crc_poly=0, prior_level=None, pin_level=None):
    """Bob's flip call -> dict(keys, status, corrected, flip_pos, decodes, n_tried, accepted): accepted[b] = the trials of open block b that passed
    the verdict test (a list; what the two-winners test looks at)"""
    N, E, T = 1 << n, len(extra_pos), n_flips
    keys = np.array(keys, np.uint32)
    B = keys.shape[0]
    extra = np.zeros(B, np.int64) if extra is None else np.array(extra, np.int64)
    xb = np.zeros((B, 0), np.uint32) if extra_bits is None else extra_bits
    kb, ok_kb = PR.valid(key_bits, B, N)
    flip_pos = np.full(B, -1, np.int32)
    if not resume:                                                # the first pass: one round of the ladder rule
        first = LD.rounds(n, pos, extra_pos, keys, syndrome, crc, xb, extra, 1, 1, key_bits, False, None, messages, maxq, crc_len, crc_poly, prior_level, pin_level)
        keys, status, corrected, decodes = first["keys"], first["status"], first["corrected"], first["decodes"]
        is_open = status == EDECODE
    else:
        status = np.array(status, np.int32)
        corrected, decodes = np.full(B, -1, np.int32), np.zeros(B, np.int32)
        candidate = status == EDECODE
        good_args = ok_kb & (extra >= 0) & (extra <= E)
        status[candidate & ~good_args] = ESIZE
        is_open = candidate & good_args
    o = np.flatnonzero(is_open)
    accepted = {}
    if len(o):
        p, pin = PR.default_levels(messages, maxq, prior_level, pin_level)
        dt = np.int8 if messages == "i8" else np.float32
        frozen = np.ones(N, bool)
        frozen[pos] = False
        rank = LD.rank_table(N, extra_pos)
        mask = PR.key_mask(kb[o], ok_kb[o], N)
        y = R.unpack(keys[o], N).astype(bool)
        llr = np.where(mask, np.where(y, dt(-p), dt(p)), dt(pin)).astype(dt)
        added = rank[None, :] < extra[o, None]
        fv = np.zeros((len(o), N), np.uint8)
        if frozen.any():
            fv[:, frozen] = R.unpack(syndrome, int(frozen.sum()))[o]
        if E:
            fv[:, np.asarray(extra_pos, np.int64)] = R.unpack(xb, E)[o] * (np.arange(E)[None, :] < extra[o, None])
        _, _, leaf = LD.decode_rows(llr, frozen, added, fv, messages, maxq)      # the probe
        flips = select(leaf.astype(dt) if messages != "i8" else leaf, frozen, T, rank, extra[o])
        for k, b in enumerate(o):
            rows, values = np.repeat(added[k][None, :], T, axis=0), np.repeat(fv[k][None, :], T, axis=0)
            for t in range(T):
                if flips[k, t] >= 0:
                    rows[t, flips[k, t]] = True
                    values[t, flips[k, t]] = leaf[k, flips[k, t]] >= 0      # the inverse of SC's decision (leaf < 0)
            u, x, _ = LD.decode_rows(np.repeat(llr[k][None, :], T, axis=0), frozen, rows, values, messages, maxq)
            match = LR.crc_bits(u[:, pos], crc_len, crc_poly) == np.uint32(np.asarray(crc, np.uint32)[b])
            xh = x.astype(bool)
            good = match & ~(xh & ~mask[k][None, :]).any(axis=1) & (flips[k] >= 0)
            accepted[int(b)] = np.flatnonzero(good).tolist()
            decodes[b] += 1 + T
            if good.any():
                t = int(np.flatnonzero(good)[0])
                status[b], flip_pos[b] = OK, flips[k, t]
                corrected[b] = int(((xh[t] ^ y[k]) & mask[k]).sum())
                keys[b] = R.pack(x[t:t + 1])[0]
            else:
                status[b], corrected[b] = EDECODE, -1
    return dict(keys=keys, status=status.astype(np.int32), corrected=corrected.astype(np.int32), flip_pos=flip_pos, decodes=decodes.astype(np.int32), n_tried=len(o),
                accepted=accepted)
