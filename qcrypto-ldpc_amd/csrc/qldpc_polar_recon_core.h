/*
 * qldpc_polar_recon_core.h -- the rule of a polar reconciliation session (qldpc_polar_recon_*): which bits of a key go where, what Alice sends,
 * what Bob's decoder is handed and when a block counts as reconciled.  Plain C on top of qldpc_polar_mc_core.h (pmc_words, pmc_crc_word, the
 * quads of a row) and through it of qldpc_polar_list_core.h (the CRC's register step pll_crc_step, not restated here) and qldpc_polar_core.h (the
 * packing), shared by the kernels (qldpc_kernels_polar_recon.h), by the host mirrors (qldpc_polar_recon_host.c) and by the session
 * (qldpc_polar_recon.hip), so that the CPU suite runs what the lanes run.
 *
 * A session belongs to one code (log2_n, info_pos[K]) and one CRC (crc_len 1 .. 32, crc_poly).  A block is a key of key_bits bits,
 * 1 <= key_bits <= N, packed MSB-first in a row of W = ceil(N / 32) words.
 *
 *   padding    positions key_bits .. N - 1 are 0 for both parties; Alice's side ignores what the caller left there (prc_key_mask).  On Alice's
 *              side a key_bits outside 1 .. N leaves no bit of the key: she sends the syndrome and the crc of the all-zero key.
 *   Alice      u = encode(x).  syndrome = the bits of u at the frozen positions in ascending position order (fpos[]), packed MSB-first into
 *              Wf = ceil((N - K) / 32) words, the tail zero.  crc = the remainder over the K bits u[info_pos[m]], m = 0 .. K - 1, in the caller's
 *              order: what qldpc_polar_crc_host gives on the decoder's info row.  Leak: N - K + crc_len bits.
 *   prior      Bob's LLR of position i is +prior where y_i = 0 and -prior where y_i = 1 for i < key_bits, and +pin for i >= key_bits (PRC_LEVEL).
 *              prior and pin are the session's: integers 1 <= prior <= pin <= maxq with int8 messages, finite 0 < prior <= pin <= 1e30 with
 *              floats.  Nothing is computed: a level is one of three constants.
 *              No QBER enters.  On a BSC every unknown position carries the same magnitude log((1 - e) / e); min-sum f takes minima and signs
 *              and g adds and subtracts, so a common factor of all finite inputs goes through every belief unchanged and the decisions do not
 *              depend on it.  Magnitude 1 is then the choice that leaves an int8 context the most room before sat clamps a sum, and a float
 *              context exact integers; pin only has to stay above every sum of priors that can meet it (maxq, the clamp itself; 2^24 > N).
 *   frozen     Bob's frozen row: the syndrome scattered back, bit of rank r to the r-th frozen position; bits at other positions are 0.  Word w
 *              takes the ranks fprefix[w] .. (the frozen positions before word w: the prefix popcounts of the frozen mask), then the bits
 *              inside the word in order (prc_frozen_bits).
 *   decode     the wrapped context's own decoder, asked for info and x (and pick with the list decoder, which is handed Alice's crc).
 *   verdict    status = PRC_OK iff the remainder of the decoded info row equals Alice's crc (SC contexts) or pick >= 0 (list contexts), AND every
 *              bit of x^ at positions >= key_bits is 0; PRC_EDECODE otherwise.  corrected = popcount((x^ ^ y) over the first key_bits bits) where
 *              OK, else -1.  Bob's key row becomes x^ where OK and is left untouched otherwise.  The picked path is the only one looked at.
 *              A key_bits outside 1 .. N: status PRC_ESIZE, corrected -1, the key untouched, and the block's LLR row is all +pin.
 */
#ifndef QLDPC_POLAR_RECON_CORE_H
#define QLDPC_POLAR_RECON_CORE_H

#include "qldpc_polar_mc_core.h"

#define PRC_FN MC_FN
enum { PRC_OK = 0, PRC_ESIZE = -6, PRC_EDECODE = -9 };      /* QLDPC_OK, QLDPC_ESIZE, QLDPC_EDECODE of include/qldpc.h */
#define PRC_F32_MAX 1e30f
#define PRC_F32_PIN 16777216.0f    /* 2^24: the binding's default pin with float messages */

PRC_FN int prc_key_bits_ok(int key_bits, int log2_n) { return key_bits >= 1 && key_bits <= (1 << log2_n); }
/* the key bits a side works with: key_bits, or 0 (no bit of the row) where it is out of range */
PRC_FN int prc_key_bits(int key_bits, int log2_n) { return prc_key_bits_ok(key_bits, log2_n) ? key_bits : 0; }
/* the bits of word w of a row that lie below key_bits (0 <= key_bits <= N) */
PRC_FN uint32_t prc_key_mask(int key_bits, uint32_t w)
{
    const long lo = 32l * (long)w;
    return key_bits <= lo ? 0u : (key_bits >= lo + 32 ? 0xffffffffu : 0xffffffffu << (32 - (key_bits - (int)lo)));
}

/* bit m of a gathered row: row[pos[m]] */
PRC_FN unsigned prc_pick_bit(const uint32_t *row, const int *pos, size_t m)
{
    const int p = pos[m];
    return pl_bit(row[p >> 5], p);
}
/* word j of the row gathered through pos[count]: Alice's syndrome with fpos, her info row with info_pos.  The tail is zero */
PRC_FN uint32_t prc_gather_word(const uint32_t *row, const int *pos, int count, size_t j)
{
    uint32_t word = 0u;
    for (size_t b = 0; b < 32u && 32u * j + b < (size_t)count; b++) word |= prc_pick_bit(row, pos, 32u * j + b) << (31u - b);
    return word;
}
/* the remainder of an info row of n_info bits */
PRC_FN uint32_t prc_row_crc(const uint32_t *info, int n_info, int crc_len, uint32_t crc_poly)
{
    uint32_t r = 0u;
    for (uint32_t j = 0; j < pmc_words(n_info); j++) r = pmc_crc_word(r, info[j], pmc_msg_bits(j, n_info), crc_len, crc_poly);
    return r;
}

/* Bob's level of position i whose key bit is `bit`: key_bits = prc_key_bits() of the block */
#define PRC_LEVEL(i, bit, key_bits, prior, pin) ((long)(i) < (long)(key_bits) ? ((bit) ? -(prior) : (prior)) : (pin))

/* bits b0 .. b0 + nb - 1 (MSB-first) of a word of Bob's frozen row: fmask_w = the word's frozen mask, first = the frozen positions before the
 * word, syn = the block's syndrome (not looked at where the mask has no bit) */
PRC_FN uint32_t prc_frozen_bits(const uint32_t *syn, uint32_t fmask_w, uint32_t first, int b0, int nb)
{
    uint32_t out = 0u, r = first + (b0 ? (uint32_t)__builtin_popcount(fmask_w >> (32 - b0)) : 0u);
    for (int b = b0; b < b0 + nb; b++)
        if ((fmask_w >> (31 - b)) & 1u) {
            out |= pl_bit(syn[r >> 5], (int)(r & 31u)) << (31 - b);
            r++;
        }
    return out;
}

/* The pure part of the verdict, for a block whose key_bits is in 1 .. N: 1 iff the remainder of the decoded info row equals Alice's crc (or, with
 * have_pick, the list decoder's pick is >= 0) and every bit of x^ at positions >= key_bits is 0.  Nothing is written: several decodes of one
 * block may be tested side by side (the flip trials of qldpc_polar_flip_core.h) before one of them takes the key.  The words of x that hold pad
 * bits are read from the top */
PRC_FN int prc_accept_block(int log2_n, int n_info, int crc_len, uint32_t crc_poly, const uint32_t *info, const uint32_t *x, int have_pick, int32_t pick,
                            int key_bits, uint32_t crc)
{
    if (have_pick ? pick < 0 : prc_row_crc(info, n_info, crc_len, crc_poly) != crc) return 0;
    const long W = pl_words(log2_n), wb = key_bits >> 5;      /* the first word with a pad bit, W where there is none */
    for (long w = W - 1; w >= wb; w--)
        if (x[w] & ~prc_key_mask(key_bits, (uint32_t)w)) return 0;
    return 1;
}

/* The write of the verdict, for a block that prc_accept_block accepted: Bob's row becomes x^, its pad words 0 as x^'s are.  Returns the flips:
 * popcount((x^ ^ y) over the first key_bits bits) */
PRC_FN int prc_take_block(int log2_n, const uint32_t *x, uint32_t *key, int key_bits)
{
    const long W = pl_words(log2_n), wb = key_bits >> 5;
    int flips = 0;
    for (long w = 0; w < wb; w++) {
        const uint32_t xw = x[w];
        flips += __builtin_popcount(xw ^ key[w]);
        key[w] = xw;
    }
    if (wb < W) {
        const uint32_t xb = x[wb];
        flips += __builtin_popcount((xb ^ key[wb]) & prc_key_mask(key_bits, (uint32_t)wb));
        key[wb] = xb;
        for (long w = wb + 1; w < W; w++) key[w] = 0u;
    }
    return flips;
}

/* The verdict of one block.  info = the decoded info row, x = x^, key = Bob's row (rewritten where the block is OK), have_pick: the list
 * decoder's pick decides in the CRC's place: the test of prc_accept_block, then the write of prc_take_block */
PRC_FN void prc_verdict_block(int log2_n, int n_info, int crc_len, uint32_t crc_poly, const uint32_t *info, const uint32_t *x, int have_pick, int32_t pick,
                              uint32_t *key, int key_bits, uint32_t crc, int *status, int *corrected)
{
    *corrected = -1;
    if (!prc_key_bits_ok(key_bits, log2_n)) { *status = PRC_ESIZE; return; }
    *status = PRC_EDECODE;
    if (!prc_accept_block(log2_n, n_info, crc_len, crc_poly, info, x, have_pick, pick, key_bits, crc)) return;
    *status = PRC_OK;
    *corrected = prc_take_block(log2_n, x, key, key_bits);
}

/* ---- host side ---- */

/* the tables of a code from its frozen mask (W words, 1 = frozen): fprefix[W] = the frozen positions before each word, fpos[N - K] = the frozen
 * positions in ascending order.  Either may be NULL.  Returns N - K */
static inline int prc_tables(int log2_n, const uint32_t *fmask, int *fprefix, int *fpos)
{
    const long W = pl_words(log2_n);
    int r = 0;
    for (long w = 0; w < W; w++) {
        if (fprefix) fprefix[w] = r;
        for (int b = 0; b < 32; b++)
            if ((fmask[w] >> (31 - b)) & 1u) {
                if (fpos) fpos[r] = (int)(32 * w + b);
                r++;
            }
    }
    return r;
}

/* the levels of a session: 0, or -1 where they are refused; with int8 messages the two integers, with floats the two floats */
static inline int prc_levels(int i8, int maxq, double prior, double pin, int *pi, int *qi, float *pf, float *qf)
{
    if (i8) {
        if (!(prior >= 1.0 && prior <= pin && pin <= (double)maxq) || (double)(int)prior != prior || (double)(int)pin != pin) return -1;
        *pi = (int)prior; *qi = (int)pin; *pf = (float)*pi; *qf = (float)*qi;
        return 0;
    }
    if (!(prior > 0.0 && prior <= pin && pin <= 1e30)) return -1;      /* a NaN fails here */
    const float p = (float)prior, q = (float)pin;
    if (!(p > 0.0f && p <= q && q <= PRC_F32_MAX)) return -1;           /* a prior that rounds to 0 */
    *pf = p; *qf = q; *pi = 0; *qi = 0;
    return 0;
}

#endif /* QLDPC_POLAR_RECON_CORE_H */
