/*
 * qldpc_kernels_guess.h -- the two kernels of a guessing round (qldpc_guess_expand_dev, qldpc_guess_pick_dev).  The rule is stated in
 * qldpc_guess_core.h; these lanes and the host mirrors call the same functions.
 *
 * qk_guess_expand: the known and value rows of the n_src T trial slots, slot s T + t, in the layout qldpc_load_known_dev reads.  blockIdx.x = the
 *     source, the waves of the gridDim.y workgroups of a source deal its T trials among them.  A wave walks the row a trip of 64 words at a time, one
 *     word per lane: the rank of a word's first bit = the set bits of the trips before it (a carry, the same in every lane) + the exclusive prefix sum
 *     of the popcounts over the lanes of the trip (shuffles).  The guess and hard words of a trip are loaded once and serve every trial of the wave;
 *     each output word is written once by one plain 4-byte store per lane, 256 contiguous bytes per wave.  No atomics, no LDS.
 * qk_guess_pick: one workgroup per source.  The T ok flags a trip of GS_LANES at a time: every wave ballots its 64 flags, the lowest set bit and the
 *     popcount per wave go through LDS, and every lane folds the partial results into the winner and n_ok.  Then the waves deal the trials among them
 *     once more: a wave compares the row of an ok trial with the winner's over the valid bits (the tail of the last word masked) and any difference
 *     sets the flag in LDS.  Last, the winner's row is copied to out_hard[s]; without a winner that row is not touched.
 */
#ifndef QLDPC_KERNELS_GUESS_H
#define QLDPC_KERNELS_GUESS_H

#include "qldpc_guess_core.h"

#define GS_LANES 256
#define GS_WAVES (GS_LANES / 64)

/* weak, hard [n_src][W]; known, value [n_src T][W], T = 1 << g */
static __global__ __launch_bounds__(GS_LANES) void qk_guess_expand(const uint32_t *__restrict__ weak, const uint32_t *__restrict__ hard, uint32_t *__restrict__ known,
                                                                   uint32_t *__restrict__ value, int W, int g)
{
    const unsigned lane = threadIdx.x & 63u, T = 1u << g;
    const unsigned wave = blockIdx.y * GS_WAVES + (threadIdx.x >> 6), waves = gridDim.y * GS_WAVES;
    if (wave >= T) return;      /* the whole wave */
    const size_t s = blockIdx.x, src = s * (size_t)W;
    unsigned carry = 0;
    for (int w0 = 0; w0 < W; w0 += 64) {
        const int w = w0 + (int)lane;
        const uint32_t k = w < W ? weak[src + w] : 0u, h = w < W ? hard[src + w] : 0u;
        unsigned incl = gs_popc(k);
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned up = __shfl_up(incl, d, 64);
            if (lane >= (unsigned)d) incl += up;
        }
        const unsigned rank0 = carry + incl - gs_popc(k);
        carry += __shfl(incl, 63, 64);
        if (w >= W) continue;      /* the shuffles of this trip are behind us; the last trip only */
        for (unsigned t = wave; t < T; t += waves) {
            const size_t dst = (s * T + t) * (size_t)W + (size_t)w;
            known[dst] = k;
            value[dst] = gs_value_word(k, h, t, rank0);
        }
    }
}

/* ok [n_src T]; trial_hard [n_src T][W]; winner, n_ok, ambiguous [n_src]; out_hard [n_src][W] */
static __global__ __launch_bounds__(GS_LANES) void qk_guess_pick(const int *__restrict__ ok, const uint32_t *__restrict__ trial_hard, int *__restrict__ winner,
                                                                 int *__restrict__ n_ok, int *__restrict__ ambiguous, uint32_t *__restrict__ out_hard, int N, int W, int g)
{
    __shared__ int s_first[GS_WAVES], s_count[GS_WAVES], s_amb;
    const unsigned t0 = threadIdx.x, lane = t0 & 63u, wave = t0 >> 6, T = 1u << g;
    const size_t s = blockIdx.x;
    const int *flags = ok + s * T;
    const uint32_t *rows = trial_hard + s * T * (size_t)W;
    int best = -1, count = 0;
    if (t0 == 0) s_amb = 0;
    for (unsigned base = 0; base < T; base += GS_LANES) {      /* T is uniform: every lane takes every trip */
        const unsigned t = base + t0;
        const unsigned long long m = __ballot(t < T && flags[min(t, T - 1u)] != 0);
        if (lane == 0) { s_first[wave] = m ? (int)(base + wave * 64u) + __ffsll((long long)m) - 1 : -1; s_count[wave] = __popcll(m); }
        __syncthreads();
        for (unsigned k = 0; k < GS_WAVES; k++) { best = gs_better(best, s_first[k], s_first[k] >= 0); count += s_count[k]; }
        __syncthreads();
    }
    if (best >= 0) {
        const uint32_t *win = rows + (size_t)best * W;
        for (unsigned t = wave; t < T; t += GS_WAVES) {      /* t is wave-uniform */
            if (t == (unsigned)best || flags[t] == 0) continue;
            int differs = 0;
            for (int w = (int)lane; w < W; w += 64) differs |= gs_differs(rows[(size_t)t * W + w], win[w], w, N);
            if (__any(differs) && lane == 0) s_amb = 1;
        }
        for (int w = (int)t0; w < W; w += GS_LANES) out_hard[s * (size_t)W + w] = win[w];
    }
    __syncthreads();
    if (t0 == 0) { winner[s] = best; n_ok[s] = count; ambiguous[s] = s_amb; }
}

#endif /* QLDPC_KERNELS_GUESS_H */
