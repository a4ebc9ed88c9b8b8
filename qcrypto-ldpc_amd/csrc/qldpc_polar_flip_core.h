/*
 * qldpc_polar_flip_core.h -- the rule of SC-Flip trials in a polar reconciliation session (qldpc_polar_recon_create_flip, _decode_flip;
 * Afisiadis, Balatsoukas-Stimming, Burg 2014): a block whose decode failed the verdict is decoded again with the decision at one of its T least
 * reliable information leaves inverted, and the first trial that passes the verdict is kept.  It is local to Bob: no packet, no added leak.
 * Plain C on top of qldpc_polar_ladder_core.h (entry, the added flags and, through it, the session's prior and verdict: none restated here),
 * shared by the kernels (qldpc_kernels_polar_flip.h), the host mirrors (qldpc_polar_flip_host.c) and the session (qldpc_polar_recon.hip).
 *
 * Successive cancellation is causal: the decisions before leaf p do not depend on the one at p.  So "decode with the decision at p inverted" IS
 * "decode with p frozen to the inverse of SC's decision there", and a trial is one more frame of the rows form of the decoder.
 *
 *   candidate  position i of a block is a candidate iff the code does not freeze it and the block's ladder count does not add it
 *              (rank[i] >= extra).  Pad positions are x-domain and play no part.
 *   key        (mag << 32) | i, 64 bits.  int8 leaves: mag = |leaf|, 0 .. 127 (the decoder clamps to -(maxq + 1) .. maxq, maxq <= 126).  float
 *              leaves: mag = the bit pattern of fabsf(leaf), monotone over the finite non-negative floats; -0.0 and +0.0 both give 0.  Every key
 *              is below 2^63; PFL_NO_KEY is above every key.
 *   flips      the T flips of a block are its T smallest keys, ascending: ties in magnitude go to the lower position (on a BSC prior ties are
 *              the normal case, so the order is part of the contract).  With fewer than T candidates the remaining entries are -1: void.
 *              Found by T passes: pass t takes the smallest key that is >= lo, lo = 0 at first and the last minimum + 1 after
 *              (pfl_pass_key per position, pfl_pass_next between passes).
 *   trial t    the block's base inputs (prior, frozen values, added flags at its extra) plus the flag of p_t, whose frozen value is
 *              (leaf[p_t] >= 0): the inverse of SC's decision (leaf < 0).  No u row is needed.  A void trial gets the base inputs and is never
 *              accepted, whatever its decode returns.
 *   accept     prc_accept_block on the trial's info and x rows: CRC match and clean pad, nothing written.
 *   settle     the winner is the lowest t whose trial is accepted (pfl_winner on the accept bits of a block).  The block then is PRC_OK, its
 *              key row becomes that trial's x^ (prc_take_block), corrected the flips against Bob's row, flip_pos = p_t.  With no winner the
 *              block stays PRC_EDECODE, its key untouched, corrected -1, flip_pos -1.  Either way its decode count goes up by 1 + T.
 *   entry      pld_entry, unchanged: resume, key_bits and extra refusals.
 *   limits     T in {1, 2, 4, 8, 16, 32}: the trials of a block are one aligned run of lanes inside a wave.
 */
#ifndef QLDPC_POLAR_FLIP_CORE_H
#define QLDPC_POLAR_FLIP_CORE_H

#include "qldpc_polar_ladder_core.h"

#define PFL_FN PLD_FN
#define PFL_MAX_FLIPS 32
#define PFL_NO_KEY 0xffffffffffffffffull

PFL_FN int pfl_flips_pow2(int t) { return t >= 1 && (t & (t - 1)) == 0; }

PFL_FN uint32_t pfl_mag_i8(int leaf) { return (uint32_t)(leaf < 0 ? -leaf : leaf); }
PFL_FN uint32_t pfl_mag_f32(float leaf)
{
    union { float f; uint32_t u; } v;
    v.f = leaf;
    return v.u & 0x7fffffffu;                                    /* the bits of fabsf(leaf) */
}
/* the frozen value of a flipped leaf: the inverse of SC's decision (leaf < 0) */
PFL_FN unsigned pfl_flip_bit_i8(int leaf) { return leaf >= 0; }
PFL_FN unsigned pfl_flip_bit_f32(float leaf) { return leaf >= 0.0f; }

/* the key of position i in a pass whose floor is lo: PFL_NO_KEY where i is no candidate or its key is below lo.  frozen: the code's flag of i;
 * rank_i: the ladder's entry (PLD_NO_RANK without a ladder) */
PFL_FN uint64_t pfl_pass_key(uint32_t mag, size_t i, unsigned frozen, int rank_i, int extra, uint64_t lo)
{
    const uint64_t key = (uint64_t)mag << 32 | (uint64_t)i;
    return frozen || rank_i < extra || key < lo ? PFL_NO_KEY : key;
}
/* the entry a pass's minimum gives, and the next pass's floor (once void, every later pass is) */
PFL_FN int pfl_pass_pos(uint64_t best) { return best == PFL_NO_KEY ? -1 : (int)(uint32_t)best; }
PFL_FN uint64_t pfl_pass_next(uint64_t best) { return best == PFL_NO_KEY ? PFL_NO_KEY : best + 1u; }

/* the winner among the T trials of a block: accept = bit t set iff trial t is accepted (void trials cleared).  -1: nobody */
PFL_FN int pfl_winner(uint32_t accept) { return accept ? __builtin_ctz(accept) : -1; }

/* ---- host side ---- */

/* the T flips of one block from its leaf row [N] (int8 or float), the code's frozen mask [W], the ladder's rank table (NULL: no ladder) and the
 * block's count: pos[T] */
static inline void pfl_select_row(int log2_n, int i8, const void *leaf, const uint32_t *fmask, const int *rank, int extra, int n_flips, int *pos)
{
    const size_t N = (size_t)1 << log2_n;
    uint64_t lo = 0u;
    for (int t = 0; t < n_flips; t++) {
        uint64_t best = PFL_NO_KEY;
        for (size_t i = 0; i < N && lo != PFL_NO_KEY; i++) {
            const uint32_t mag = i8 ? pfl_mag_i8(((const int8_t *)leaf)[i]) : pfl_mag_f32(((const float *)leaf)[i]);
            const uint64_t k = pfl_pass_key(mag, i, pl_bit(fmask[i >> 5], (int)(i & 31u)), rank ? rank[i] : PLD_NO_RANK, extra, lo);
            if (k < best) best = k;
        }
        pos[t] = pfl_pass_pos(best);
        lo = pfl_pass_next(best);
    }
}

#endif /* QLDPC_POLAR_FLIP_CORE_H */
