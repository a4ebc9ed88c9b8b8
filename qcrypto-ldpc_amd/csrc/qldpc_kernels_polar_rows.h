/*
 * qldpc_kernels_polar_rows.h -- the kernel of qldpc_polar_decode_rows_dev: the rows form of pl_decode (qldpc_kernels_polar.h), a frozen set per
 * frame.  The rule is qldpc_polar_core.h's: pl_rows_frozen on top of the SC decoder.
 *
 * pl_decode_rows is pl_decode with one more operand.  In pl_decode the frozen flags of a 32-leaf block are one wave-uniform word, fmask[j];
 * here a lane loads one more word, word j of its own frame's row, and ORs it in.  Nothing else changes, and nothing diverges: the traversal of
 * the tree never looks at the flags, which reach a leaf only as an operand of pl_leaf_bit, a select.  So the 64 frames of a wave may sit at 64
 * different rates and still take every level step (pl_block_beliefs), leaf block (pl_node) and combine (pl_combine_words) together.
 *
 * The scratch, its layout, pl_load before and pl_outputs after are the lanes form's.  A lane past n_frames returns at once and stores nothing;
 * every index is 64 bits wide.
 */
#ifndef QLDPC_KERNELS_POLAR_ROWS_H
#define QLDPC_KERNELS_POLAR_ROWS_H

#include "qldpc_kernels_polar.h"

/* grid = groups, 64 lanes; SL, TOP and every argument as pl_decode's.  frows: the frames' frozen flags [n_frames][W], which add to fmask */
template <class M, int SL, bool TOP>
__global__ __launch_bounds__(PL_GROUP) void pl_decode_rows(M m, int n, int n_frames, const typename M::mem *__restrict__ llr, const uint32_t *__restrict__ fmask,
                                                           const uint32_t *__restrict__ fval, const uint32_t *__restrict__ frows, typename M::mem *B, uint32_t *Us,
                                                           uint32_t *Xs, typename M::mem *__restrict__ leaf_out)
{
    typedef typename M::mem mem;
    typedef typename M::reg reg;
    constexpr int S = 1 << SL;
    const unsigned lane = threadIdx.x;
    const size_t g = blockIdx.x, frame = g * PL_GROUP + lane;
    if (frame >= (size_t)n_frames) return;                       /* stores nothing; no other lane waits for this one */
    const size_t N = (size_t)1 << n, W = (size_t)pl_words(n);
    uint32_t *U = Us + g * W * PL_GROUP + lane, *X = Xs + g * W * PL_GROUP + lane;
    const pl_quad<mem> *V = nullptr;
    pl_quad<mem> *Vw = nullptr;
    if constexpr (!TOP) { Vw = (pl_quad<mem> *)(B + g * pl_group_elems(n)) + lane; V = Vw; }
    reg R[32], leaf[32];
    for (size_t j = 0; j < (TOP ? (size_t)1 : W); j++) {
        if constexpr (TOP) {
#pragma unroll
            for (int i = 0; i < S; i++) R[i] = m.load(llr[frame * N + i]);
        } else {
            pl_block_beliefs(m, n, j, V, Vw, X, R);
        }
        uint32_t u = 0u, x = 0u;
        pl_node<S, 0>(m, R, pl_rows_frozen(fmask[j], frows[frame * W + j]), fval ? fval[frame * W + j] : 0u, u, x, leaf);
        U[j * PL_GROUP] = u;
        X[j * PL_GROUP] = x;
        pl_combine_words(X, (long)j, PL_GROUP);
        if (leaf_out) {
#pragma unroll
            for (int i = 0; i < S; i++) leaf_out[frame * N + j * S + i] = (mem)leaf[i];
        }
    }
}

#endif /* QLDPC_KERNELS_POLAR_ROWS_H */
