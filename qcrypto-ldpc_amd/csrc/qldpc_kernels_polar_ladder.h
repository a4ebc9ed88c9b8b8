/*
 * qldpc_kernels_polar_ladder.h -- the kernels of incremental freezing in the polar reconciliation sessions (qldpc_polar_recon_encode_ladder_dev,
 * _decode_rounds), gfx950, wave64.  Every rule is qldpc_polar_ladder_core.h's and, through it, qldpc_polar_recon_core.h's: the slot kernels call
 * the functions prc_prior and prc_verdict call.  qldpc_polar_recon.hip launches them around the rows form of the SC decoder.
 *
 *   pld_extra_rows   Alice: a wave per block, one more prc_gather_row of the block's u row, through the ladder's extra_pos[].
 *   pld_entry_blocks Bob, once a call: a lane per block, pld_entry.  A refused block gets its status, an open one is appended to the open list.
 *   pld_slot_prior   Bob, every round: prc_prior for slot s = block open[s], a lane per quad of positions.  Besides the LLR quad and its four bits
 *                    of the frozen row (the syndrome's, or Alice's extra row where the block's count adds the position) the lane forms its four
 *                    added flags; the eight lanes of a word OR both together by shuffles every lane of the wave takes part in.  The first lane of
 *                    a slot counts the decode.  Its body is pld_slot_prior_lane, which the flip trials share (qldpc_kernels_polar_flip.h).
 *   pld_slot_verdict Bob, every round: a lane per slot, prc_verdict_block on the slot's info and x rows and the block's key, crc and key_bits.
 *                    A block that failed and stays open gets its next count and is appended to the NEXT round's open list.
 *
 * The open list is filled by pld_append: a wave ballots who appends, its first such lane takes the wave's places with ONE atomic add on the
 * counter, and every appending lane stores its block at its rank among them.  The order of a list is not defined and nothing depends on it: a
 * slot's outputs go to its block.  No lane leaves before the ballot.  Indices are 64 bits wide; no spinning, no LDS, nothing between workgroups
 * but the counter.
 */
#ifndef QLDPC_KERNELS_POLAR_LADDER_H
#define QLDPC_KERNELS_POLAR_LADDER_H

#include "qldpc_kernels_polar_recon.h"
#include "qldpc_polar_ladder_core.h"

/* every lane of the wave calls it; list has room for every block of the call */
__device__ static inline void pld_append(bool add, int block, int *__restrict__ list, int *__restrict__ count)
{
    const unsigned long long m = __ballot((int)add);
    if (!m) return;                                              /* the wave's */
    const int lane = (int)(threadIdx.x & 63u), first = __ffsll(m) - 1;
    int base = 0;
    if (lane == first) base = atomicAdd(count, __popcll(m));
    base = __shfl(base, first, 64);
    if (add) list[(size_t)base + (size_t)__popcll(m & ((1ull << lane) - 1ull))] = block;
}

/* u [n][W] (the session's row after Alice's encode) -> extra_bits [n][We]; grid = ceil(n / 4), 256 lanes */
__global__ __launch_bounds__(PRC_LANES) void pld_extra_rows(const uint32_t *__restrict__ u, const int *__restrict__ extra_pos, uint32_t *__restrict__ extra_bits,
                                                            unsigned n, unsigned W, unsigned E)
{
    const unsigned lane = threadIdx.x & 63u;
    const size_t f = (size_t)blockIdx.x * (PRC_LANES / 64u) + (threadIdx.x >> 6), We = pld_extra_words((int)E);
    if (f >= n) return;                                          /* the whole wave */
    prc_gather_row(u + f * W, extra_pos, E, extra_bits + f * We, lane);
}

/* key_bits [n] or NULL, extra [n] or NULL (every count 0), status [n] (read with resume) -> status, corrected (or NULL) of the refused, decodes [n] (or NULL) = 0, the
   open list and *count (zero before) */
__global__ __launch_bounds__(PRC_LANES) void pld_entry_blocks(const int *__restrict__ key_bits, const int *__restrict__ extra, int *__restrict__ status,
                                                              int *__restrict__ corrected, int *__restrict__ decodes, int *__restrict__ open, int *__restrict__ count,
                                                              unsigned n, int log2_n, int n_extra, int resume)
{
    const size_t b = (size_t)blockIdx.x * PRC_LANES + threadIdx.x;
    int what = PLD_KEEP;
    if (b < n) {
        what = pld_entry(resume, resume ? status[b] : 0, key_bits ? key_bits[b] : 1 << log2_n, log2_n, extra ? extra[b] : 0, n_extra);
        if (decodes) decodes[b] = 0;
        if (what == PLD_REFUSE) {
            status[b] = PRC_ESIZE;
            if (corrected) corrected[b] = -1;
        }
    }
    pld_append(what == PLD_OPEN, (int)b, open, count);
}

/* The slot prior of one lane, a quad of positions: slot s takes the inputs of block b.  Every lane of the wave calls it (the shuffles), active or
   not.  flip >= 0: position `flip` of the slot is frozen besides, to flip_bit (a flip trial, qldpc_kernels_polar_flip.h); -1: nothing more */
template <class T>
__device__ static inline void pld_slot_prior_lane(bool active, size_t s, unsigned q, size_t b, int flip, unsigned flip_bit, const uint32_t *__restrict__ keys,
                                                  const int *__restrict__ key_bits, const uint32_t *__restrict__ syn, const uint32_t *__restrict__ xbits,
                                                  const int *__restrict__ extra, const uint32_t *__restrict__ fmask, const int *__restrict__ fprefix,
                                                  const int *__restrict__ rank, void *__restrict__ llr, uint32_t *__restrict__ frozen, uint32_t *__restrict__ flags,
                                                  int *__restrict__ decodes, int log2_n, unsigned W, unsigned Wf, unsigned We, T prior, T pin)
{
    const unsigned lq = log2_n >= 2 ? (unsigned)log2_n - 2u : 0u, Qn = 1u << lq, group = Qn < 8u ? Qn : 8u;      /* lanes of a frozen word */
    uint32_t fz = 0u, fl = 0u;
    if (active) {
        const int kb = prc_key_bits(key_bits ? key_bits[b] : 1 << log2_n, log2_n);
        const uint32_t bits = pmc_quad_bits(keys + b * W, q);
        T l[4];
#pragma unroll
        for (unsigned k = 0; k < 4; k++) l[k] = PRC_LEVEL(4u * q + k, (bits >> (3u - k)) & 1u, kb, prior, pin);
        if constexpr (std::is_same<T, int>::value) {
            int8_t *p = (int8_t *)llr + (s << log2_n) + 4u * (size_t)q;
            if (log2_n >= 2)
                *(uint32_t *)p = ((uint32_t)l[0] & 0xffu) | ((uint32_t)l[1] & 0xffu) << 8 | ((uint32_t)l[2] & 0xffu) << 16 | ((uint32_t)l[3] & 0xffu) << 24;
            else { p[0] = (int8_t)l[0]; p[1] = (int8_t)l[1]; }      /* N = 2: positions 2 and 3 do not exist */
        } else {
            float *p = (float *)llr + (s << log2_n) + 4u * (size_t)q;
            if (log2_n >= 2) *(float4 *)p = make_float4((float)l[0], (float)l[1], (float)l[2], (float)l[3]);
            else { p[0] = (float)l[0]; p[1] = (float)l[1]; }
        }
        const unsigned w = q >> 3;
        uint32_t va;
        pld_ladder_bits(rank, log2_n, w, (int)(4u * (q & 7u)), 4, extra ? extra[b] : 0, xbits + b * We, &fl, &va);
        fz = prc_frozen_bits(syn + b * Wf, fmask[w], (uint32_t)fprefix[w], (int)(4u * (q & 7u)), 4) | va;
        if (flip >= 0 && (unsigned)flip >> 2 == q) {             /* a candidate: neither the code nor the ladder has set its bits */
            const uint32_t m = 1u << (31 - (flip & 31));
            fl |= m;
            fz = (fz & ~m) | (flip_bit ? m : 0u);
        }
        if (q == 0u && decodes) decodes[b]++;                    /* the slot's only lane with q = 0, the block's only slot */
    }
    for (unsigned k = 1; k < group; k <<= 1) {                   /* group is the launch's: every lane shuffles */
        fz |= (uint32_t)__shfl_xor((int)fz, (int)k, 64);
        fl |= (uint32_t)__shfl_xor((int)fl, (int)k, 64);
    }
    if (active && (q & (group - 1u)) == 0u) {
        frozen[s * W + (q >> 3)] = fz;
        flags[s * W + (q >> 3)] = fl;
    }
}

/* slot s = block open[s] (open NULL: block s): keys, key_bits, syn, xbits [.][We], extra (NULL: 0) of the block -> llr [n_open][N], frozen
   [n_open][W], flags [n_open][W]; total = n_open quads lanes.  rank: the ladder's table [N] */
template <class T>
__global__ __launch_bounds__(PRC_LANES) void pld_slot_prior(const int *__restrict__ open, const uint32_t *__restrict__ keys, const int *__restrict__ key_bits,
                                                            const uint32_t *__restrict__ syn, const uint32_t *__restrict__ xbits, const int *__restrict__ extra,
                                                            const uint32_t *__restrict__ fmask, const int *__restrict__ fprefix, const int *__restrict__ rank,
                                                            void *__restrict__ llr, uint32_t *__restrict__ frozen, uint32_t *__restrict__ flags, int *__restrict__ decodes,
                                                            size_t total, int log2_n, unsigned W, unsigned Wf, unsigned We, T prior, T pin)
{
    const size_t i = (size_t)blockIdx.x * PRC_LANES + threadIdx.x;
    const unsigned lq = log2_n >= 2 ? (unsigned)log2_n - 2u : 0u;
    const bool active = i < total;
    const size_t s = active ? i >> lq : 0u;
    pld_slot_prior_lane<T>(active, s, (unsigned)(i & ((1u << lq) - 1u)), active ? (open ? (size_t)open[s] : s) : 0u, -1, 0u, keys, key_bits, syn, xbits, extra, fmask,
                           fprefix, rank, llr, frozen, flags, decodes, log2_n, W, Wf, We, prior, pin);
}

/* slot s = block open[s]: info [n_open][Wi], x [n_open][W] -> status, corrected (or NULL), keys, extra of the block, and the next round's list.
   t: the round; count_next is zero before */
__global__ __launch_bounds__(PRC_LANES) void pld_slot_verdict(const int *__restrict__ open, const uint32_t *__restrict__ info, const uint32_t *__restrict__ x,
                                                              uint32_t *__restrict__ keys, const int *__restrict__ key_bits, const uint32_t *__restrict__ crc,
                                                              int *__restrict__ extra, int *__restrict__ status, int *__restrict__ corrected, int *__restrict__ open_next,
                                                              int *__restrict__ count_next, unsigned n_open, int log2_n, int K, int crc_len, uint32_t crc_poly,
                                                              int n_extra, int step, int t, int max_rounds)
{
    const size_t s = (size_t)blockIdx.x * PRC_LANES + threadIdx.x, W = (size_t)pl_words(log2_n), Wi = pmc_words(K);
    bool again = false;
    int block = 0;
    if (s < n_open) {
        block = open[s];
        const size_t b = (size_t)block;
        int st, co;
        prc_verdict_block(log2_n, K, crc_len, crc_poly, info + s * Wi, x + s * W, 0, 0, keys + b * W, key_bits ? key_bits[b] : 1 << log2_n, crc[b], &st, &co);
        status[b] = st;
        if (corrected) corrected[b] = co;
        const int e = extra[b];
        again = st == PRC_EDECODE && pld_stays_open(e, n_extra, t, max_rounds);
        if (again) extra[b] = pld_next_extra(e, n_extra, step);
    }
    pld_append(again, block, open_next, count_next);
}

#endif /* QLDPC_KERNELS_POLAR_LADDER_H */
