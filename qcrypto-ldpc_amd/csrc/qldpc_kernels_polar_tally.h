/*
 * qldpc_kernels_polar_tally.h -- the kernel of qldpc_polar_tally_dev: the tally form of pl_decode (qldpc_kernels_polar.h).  The rule is
 * qldpc_polar_tally_core.h's.
 *
 * pl_tally is the genie decode of 64 frames by a wave, a frame a lane: the level steps (pl_block_beliefs), the leaf block (pl_node) and the x row
 * of pl_decode, with every position frozen (the frozen word is all ones) to the frame's true word.  It writes no U row, no leaf array and needs
 * no pl_outputs launch.  Per leaf block a lane packs its 32 leaf beliefs and its truth word into one wrong word and one tie word, the wave
 * transposes the 64 x 64 bits (qldpc_wave_transpose.h), after which lane c < 32 holds the wrong bits of position c of all 64 frames and lane
 * 32 + c their tie bits, ONE popcount each: the partial of the wave.  Then one no-return 64-bit atomic add per lane whose count is not zero, to
 * 32 neighbouring counts (256 bytes) of the wrong row and 32 of the tie row.  Counts are integers: the order of the adds does not matter.
 *
 * A lane past n_frames does NOT return: the transpose needs every lane.  It walks the zeros pl_load put at its place in the scratch, reads no
 * row of the caller's, and its two words are cleared before the transpose, so it adds nothing.  TOP instances (N < 32) tally S positions.
 * Every index is 64 bits wide.
 */
#ifndef QLDPC_KERNELS_POLAR_TALLY_H
#define QLDPC_KERNELS_POLAR_TALLY_H

#include "qldpc_kernels_polar.h"
#include "qldpc_polar_tally_core.h"
#include "qldpc_wave_transpose.h"

__device__ __forceinline__ unsigned plt_tie(int L) { return plt_tie_i8(L); }
__device__ __forceinline__ unsigned plt_tie(float L) { return plt_tie_f32(L); }
__device__ __forceinline__ unsigned plt_wrong(int L, unsigned u) { return plt_wrong_i8(L, u); }
__device__ __forceinline__ unsigned plt_wrong(float L, unsigned u) { return plt_wrong_f32(L, u); }

/* grid = groups, 64 lanes; SL, TOP as pl_decode's.  truth: the frames' true rows [n_frames][W]; B, Xs: the context's scratch; tally: [2][N], added to */
template <class M, int SL, bool TOP>
__global__ __launch_bounds__(PL_GROUP) void pl_tally(M m, int n, int n_frames, const typename M::mem *__restrict__ llr, const uint32_t *__restrict__ truth,
                                                     typename M::mem *B, uint32_t *Xs, unsigned long long *__restrict__ tally)
{
    typedef typename M::mem mem;
    typedef typename M::reg reg;
    constexpr int S = 1 << SL;
    const unsigned lane = threadIdx.x;
    const size_t g = blockIdx.x, frame = g * PL_GROUP + lane;
    const bool alive = frame < (size_t)n_frames;
    const size_t N = (size_t)1 << n, W = (size_t)pl_words(n);
    uint32_t *X = Xs + g * W * PL_GROUP + lane;
    const pl_quad<mem> *V = nullptr;
    pl_quad<mem> *Vw = nullptr;
    if constexpr (!TOP) { Vw = (pl_quad<mem> *)(B + g * pl_group_elems(n)) + lane; V = Vw; }
    reg R[32], leaf[32];
    for (size_t j = 0; j < (TOP ? (size_t)1 : W); j++) {
        if constexpr (TOP) {
#pragma unroll
            for (int i = 0; i < S; i++) R[i] = alive ? m.load(llr[frame * N + i]) : (reg)0;
        } else {
            pl_block_beliefs(m, n, j, V, Vw, X, R);
        }
        const uint32_t t = alive ? truth[frame * W + j] : 0u;
        uint32_t u = 0u, x = 0u;
        pl_node<S, 0>(m, R, 0xffffffffu, t, u, x, leaf);
        X[j * PL_GROUP] = x;
        pl_combine_words(X, (long)j, PL_GROUP);
        uint32_t wrong = 0u, tie = 0u;                           /* plt_block_words_* on registers */
#pragma unroll
        for (int i = 0; i < S; i++) {
            tie |= plt_tie(leaf[i]) << i;
            wrong |= plt_wrong(leaf[i], (t >> (31 - i)) & 1u) << i;
        }
        if (!alive) wrong = tie = 0u;
        const unsigned long long count = (unsigned long long)__popcll(qk_transpose64((unsigned long long)tie << 32 | wrong, (int)lane));
        const size_t c = lane & 31u, row = lane >> 5;            /* row 0: wrong, row 1: ties */
        if (c < (size_t)S && count) atomicAdd(&tally[row * N + j * S + c], count);
    }
}

#endif /* QLDPC_KERNELS_POLAR_TALLY_H */
