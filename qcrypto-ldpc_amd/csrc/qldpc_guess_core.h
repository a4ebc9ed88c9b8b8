/*
 * qldpc_guess_core.h -- the definition of a guessing round: a frame whose decode failed is decoded again with its g least reliable VNs pinned to each of
 * the 2^g possible values, and a trial whose syndrome comes out zero is kept.  Nothing is disclosed.  Plain C, shared by the kernels (qk_guess_expand,
 * qk_guess_pick in qldpc_kernels_guess.h) and by their host mirrors (qldpc_guess_trial_host, qldpc_guess_pick_host in qldpc_guess_host.c), so that the
 * CPU suite runs what the lanes run.
 *
 *   guess set  the row qldpc_fetch_weakest_dev(cand, take, d = g) gives for the frame: a packed set of at most g VNs, ceil(N / 32) words, MSB-first;
 *              `hard` is the frame's packed hard-decision row (qldpc_fetch_packed_dev) of the same run
 *   rank       of a VN of the set = the set bits before it in ascending VN order: only the set matters, not the order of the select
 *   trial t    0 <= t < T = 2^g pins the VN v of rank j to hard[v] ^ ((t >> j) & 1); ranks >= popcount(row) do not exist and the bits of t above
 *              them are ignored; a rank >= g (a row of more than g bits) sees a zero bit of t; trial 0 pins the frame's own decisions
 *   rows       known row of a trial = the guess row; value row = (hard ^ deposit(t)) on the set bits and 0 elsewhere: what qldpc_load_known_dev reads
 *   winner     the lowest t whose decode ends with ok = 1, or -1; n_ok = the number of such trials; the frame is AMBIGUOUS when some ok trial's hard
 *              row differs from the winner's in any of the N valid bits (the padding of the last word does not count)
 */
#ifndef QLDPC_GUESS_CORE_H
#define QLDPC_GUESS_CORE_H

#include <stdint.h>

#if defined(__HIPCC__)
#define GS_FN __host__ __device__ static inline
#else
#define GS_FN static inline
#endif

#define GS_MAX_BITS 10             /* QLDPC_GUESS_MAX_BITS of include/qldpc.h */
#define GS_MAX_SLOTS (1u << 24)    /* n_src T of one call */

/* the valid bits of word w of a row of N VNs */
GS_FN uint32_t gs_valid(int w, int N)
{
    return (w == (N - 1) / 32 && (N & 31)) ? 0xffffffffu << (32 - (N & 31)) : 0xffffffffu;
}
GS_FN unsigned gs_popc(uint32_t x) { return (unsigned)__builtin_popcount(x); }
/* the bits of t from bit `rank0` on, laid onto the set bits of `weak` in ascending VN order (MSB first): rank0 = the set bits of the row before
 * this word */
GS_FN uint32_t gs_deposit(uint32_t weak, uint32_t t, unsigned rank0)
{
    uint32_t out = 0, bits = rank0 < 32u ? t >> rank0 : 0u;
    for (uint32_t m = weak; m && bits; bits >>= 1) {
        const uint32_t top = 0x80000000u >> __builtin_clz(m);
        if (bits & 1u) out |= top;
        m &= ~top;
    }
    return out;
}
/* the value word of trial t */
GS_FN uint32_t gs_value_word(uint32_t weak, uint32_t hard, uint32_t t, unsigned rank0) { return (hard ^ gs_deposit(weak, t, rank0)) & weak; }
/* do two hard rows differ in a valid bit of word w? */
GS_FN int gs_differs(uint32_t a, uint32_t b, int w, int N) { return ((a ^ b) & gs_valid(w, N)) != 0u; }
/* the winner so far (-1: none) after trial t with verdict ok; any order of the trials gives the lowest */
GS_FN int gs_better(int winner, int t, int ok) { return (ok && (winner < 0 || t < winner)) ? t : winner; }

#endif /* QLDPC_GUESS_CORE_H */
