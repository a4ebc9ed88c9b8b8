/*
 * qldpc_weakest_core.h -- the definition of "the d least reliable variable nodes of a frame" (blind reconciliation: qldpc_fetch_weakest_dev,
 * qldpc_recon_decode_blind), plain C, shared by the kernel (qk_weakest in qldpc_engine.hip) and by its host mirror (qldpc_weakest_host in
 * qldpc_blind_host.c), so that the CPU suite runs what the lanes run.
 *
 *   key      of VN v = the bit pattern of |post[v]| as uint32 (bits & 0x7fffffff): non-negative floats order as integers, -0 equals +0,
 *            a NaN is the most reliable value there is
 *   order    ascending (key, v)
 *   result   a packed row of ceil(N / 32) words, MSB-first (helpers.h:65-70), a bit set for the min(d, candidates) first candidates of that order
 *
 * The select is a radix select over the keys, most significant 8-bit digit first: per digit a histogram of the candidates that agree with the
 * digits chosen so far, and a walk along its 256 bins that finds the bin holding the element of rank `rem` (1-based) and leaves in `rem` its rank
 * inside that bin.  After four digits the threshold key T is known and rem of the candidates equal to T are taken, the first ones in index order.
 * Counts are 32-bit: N passes 65 535 in every workload of the project.
 */
#ifndef QLDPC_WEAKEST_CORE_H
#define QLDPC_WEAKEST_CORE_H

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define WK_FN __host__ __device__ static inline
#else
#define WK_FN static inline
#endif

#define WK_DIGITS 4      /* 8-bit digits of a key, most significant first */
#define WK_BINS 256

WK_FN uint32_t wk_key_of_bits(uint32_t float_bits) { return float_bits & 0x7fffffffu; }
/* digit p (0 = most significant) of a key */
WK_FN uint32_t wk_digit(uint32_t key, int p) { return (key >> (24 - 8 * p)) & 0xffu; }
/* does `key` agree with `prefix` in the digits before p? */
WK_FN int wk_agrees(uint32_t key, uint32_t prefix, int p) { return p == 0 || (key >> (32 - 8 * p)) == (prefix >> (32 - 8 * p)); }
/* the candidate bits of word w of a row of N VNs: cand_row == NULL means every VN; bits at v >= N are cleared */
WK_FN uint32_t wk_cand_word(const uint32_t *cand_row, int w, int N)
{
    uint32_t c = cand_row ? cand_row[w] : 0xffffffffu;
    if (w == (N - 1) / 32 && (N & 31)) c &= 0xffffffffu << (32 - (N & 31));
    return c;
}
/* the bin of hist[WK_BINS] (entries `stride` words apart) that holds the element of 1-based rank *rem; *rem becomes its rank inside that bin and
 * *in_bin the bin's count.  *rem must be in 1 .. the sum of the bins. */
WK_FN uint32_t wk_pick(const uint32_t *hist, int stride, uint32_t *rem, uint32_t *in_bin)
{
    uint32_t r = *rem, b = 0, h = hist[0];
    while (b < WK_BINS - 1 && r > h) { r -= h; b++; h = hist[(size_t)b * stride]; }
    *rem = r; *in_bin = h;
    return b;
}
/* is a candidate with this key taken?  T = threshold key, rem = how many of the candidates equal to T are taken, *run = how many of them came
 * before this one in index order (advanced here) */
WK_FN int wk_taken(uint32_t key, uint32_t T, uint32_t rem, uint32_t *run)
{
    if (key < T) return 1;
    if (key != T) return 0;
    return (*run)++ < rem;
}

#endif /* QLDPC_WEAKEST_CORE_H */
