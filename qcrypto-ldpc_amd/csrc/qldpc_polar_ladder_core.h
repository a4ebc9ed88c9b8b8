/*
 * qldpc_polar_ladder_core.h -- the rule of incremental freezing in a polar reconciliation session (qldpc_polar_recon_*_ladder, _decode_rounds): a
 * block that failed is decoded again with more positions frozen, the same code at a lower rate.  Plain C on top of qldpc_polar_recon_core.h (the
 * key mask, the gather, the prior, the frozen row, the verdict: none restated here), shared by the kernels (qldpc_kernels_polar_ladder.h), the
 * host mirrors (qldpc_polar_ladder_host.c) and the session (qldpc_polar_recon.hip).
 *
 *   ladder     a disclosure order extra_pos[E], 0 <= E <= K: distinct information positions of the session's code, in the order in which they are
 *              given up (the caller would pass the least reliable first).  rank[i] = m where extra_pos[m] = i, PLD_NO_RANK at every other
 *              position.  Per block an integer extra in 0 .. E: the first `extra` entries are frozen for that block, so the sets are nested.
 *   Alice      besides syndrome and crc, a row of We = ceil(E / 32) words: the bits of u at extra_pos[0 .. E), MSB-first, the tail zero
 *              (prc_gather_word through extra_pos).  She sends a prefix of it per round; the leak of a block is N - K + crc_len + extra.
 *   Bob        position i of a block is frozen iff the code freezes it or rank[i] < extra (pld_ladder_bits gives the added flags; the decoder ORs
 *              them in, pl_rows_frozen).  Its frozen value is the syndrome's bit (prc_frozen_bits) at a frozen position of the code and bit
 *              rank[i] of Alice's row at an added one.  No bit of that row at or beyond `extra` is looked at.
 *   entry      pld_entry: with resume = 0 every block is a candidate; with resume = 1 only a block whose status is PRC_EDECODE, and every other
 *              block is left alone in every output but its decode count.  A candidate with a key_bits outside 1 .. N or an extra outside 0 .. E is
 *              refused (status PRC_ESIZE, corrected -1, key and extra untouched); every other candidate is open.
 *   round t    the open blocks are decoded at their extra with the SC decoder in its rows form, and get the session's verdict
 *              (prc_verdict_block, unchanged).  A block that is PRC_OK is closed.  A block that failed at extra = e stays open iff e < E and
 *              t + 1 < max_rounds (pld_stays_open), with extra <- min(E, e + step) (pld_next_extra); otherwise it is closed as PRC_EDECODE and its
 *              extra stays e: on return extra is the count the block's last decode ran with.
 *   start      pld_start_extra (host only, a suggestion the session never takes by itself): the count at which a block of key_bits bits at a
 *              given QBER has leaked f times the Slepian-Wolf bound, clamp(ceil(f h2(qber) key_bits) - (N - K), 0, E).
 */
#ifndef QLDPC_POLAR_LADDER_CORE_H
#define QLDPC_POLAR_LADDER_CORE_H

#include "qldpc_polar_recon_core.h"

#define PLD_FN PRC_FN
#define PLD_NO_RANK 0x7fffffff     /* above every extra: such a position is never added */
enum { PLD_KEEP = 0, PLD_OPEN = 1, PLD_REFUSE = -1 };

PLD_FN int pld_extra_ok(int extra, int n_extra) { return extra >= 0 && extra <= n_extra; }
/* words of Alice's extra row */
PLD_FN uint32_t pld_extra_words(int n_extra) { return pmc_words(n_extra); }

/* what a call makes of a block on entry; status_in is looked at with resume only */
PLD_FN int pld_entry(int resume, int status_in, int key_bits, int log2_n, int extra, int n_extra)
{
    if (resume && status_in != PRC_EDECODE) return PLD_KEEP;
    return prc_key_bits_ok(key_bits, log2_n) && pld_extra_ok(extra, n_extra) ? PLD_OPEN : PLD_REFUSE;
}

/* bits b0 .. b0 + nb - 1 (MSB-first) of word w of a block's two ladder rows: *flags = the positions its `extra` adds to the frozen set, *values =
 * their bits of Alice's row xbits (not looked at where extra = 0).  rank: the N entries of the table */
PLD_FN void pld_ladder_bits(const int *rank, int log2_n, size_t w, int b0, int nb, int extra, const uint32_t *xbits, uint32_t *flags, uint32_t *values)
{
    const size_t N = (size_t)1 << log2_n;
    uint32_t fl = 0u, va = 0u;
    for (int b = b0; b < b0 + nb && 32u * w + (size_t)b < N; b++) {
        const int r = rank[32u * w + (size_t)b];
        if (r < extra) {
            fl |= 1u << (31 - b);
            va |= pl_bit(xbits[r >> 5], r) << (31 - b);
        }
    }
    *flags = fl;
    *values = va;
}

/* after a failed decode at extra = e in round t */
PLD_FN int pld_stays_open(int e, int n_extra, int t, int max_rounds) { return e < n_extra && t + 1 < max_rounds; }
PLD_FN int pld_next_extra(int e, int n_extra, int step) { return step >= n_extra - e ? n_extra : e + step; }

/* ---- host side ---- */

/* the rank table of a ladder from the code's frozen mask (W words, 1 = frozen): rank[N].  0, PRC_ESIZE where n_extra is outside 0 .. n_info, or -1
 * (QLDPC_EINVAL) where an entry is no information position of the code or comes twice */
static inline int pld_rank_table(int log2_n, const uint32_t *fmask, int n_info, int n_extra, const int *extra_pos, int *rank)
{
    const long N = 1l << log2_n;
    if (n_extra < 0 || n_extra > n_info) return PRC_ESIZE;
    if (n_extra > 0 && !extra_pos) return -1;
    for (long i = 0; i < N; i++) rank[i] = PLD_NO_RANK;
    for (int m = 0; m < n_extra; m++) {
        const int p = extra_pos[m];
        if (p < 0 || p >= N || pl_bit(fmask[p >> 5], p) || rank[p] != PLD_NO_RANK) return -1;
        rank[p] = m;
    }
    return 0;
}

/* the binary entropy in bits; 0 at 0 and 1 */
static inline double pld_h2(double q) { return q <= 0.0 || q >= 1.0 ? 0.0 : -(q * __builtin_log2(q) + (1.0 - q) * __builtin_log2(1.0 - q)); }

static inline int pld_start_extra(int log2_n, int n_info, int n_extra, int key_bits, double qber, double f)
{
    const double want = __builtin_ceil(f * pld_h2(qber) * (double)key_bits) - (double)((1l << log2_n) - n_info);
    return !(want > 0.0) ? 0 : (want >= (double)n_extra ? n_extra : (int)want);
}

#endif /* QLDPC_POLAR_LADDER_CORE_H */
