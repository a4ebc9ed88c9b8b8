/*
 * qldpc_kernels_polar_ssc.h -- the kernel of the simplified SC decoder (the rule, its one difference from SC and the plan are
 * qldpc_polar_ssc_core.h's), in the lanes form of qldpc_kernels_polar.h: a wave decodes 64 frames, a lane holds one frame, the scratch, the u
 * and x rows, pl_load, pl_pair32, pl_store32 and pl_outputs are that file's as they are.
 *
 * The plan depends on the code alone, so the control flow stays wave-uniform: pl_ssc_decode loops over the steps of the plan (in device memory,
 * read with wave-uniform indices) where pl_decode loops over the leaf blocks.
 *
 *   descent    before a step at leaf block j whose node sits at level lam: from top(j), as pl_block_beliefs, down to level lam for a rate-1
 *              node or a mixed block and only to level lam + 1 for a rate-0 node (for one that is a right child: no level at all).  The
 *              node's own level is never stored: nobody reads it afterwards.
 *   rate 0     the U words are the frame's frozen words, the X words their encoding over the node: pl_enc_word per word, then the word
 *              butterflies of the node in the lane's own rows.
 *   rate 1     each X word is the 32 sign bits of 32 beliefs of level lam, packed out of pl_pair32's registers (a rate-1 root reads the signs
 *              of level n itself); the U words are the node's encoding of X, skipped when the call asks for neither u nor info.
 *   mixed      pl_ssc_node: pl_node with a wave-uniform test of the block's frozen word at every node of 2 .. 32 leaves; no leaf[] array.
 *   after      the nodes that end with the step's last block are combined, from twice the step's size (pl_ssc_combine).
 * Frames of n <= 5 are one such block, read from the caller's rows (the five TOP instances).  No LDS, no barrier, no atomics; a lane past
 * n_frames returns at once; every index is 64 bits wide.
 */
#ifndef QLDPC_KERNELS_POLAR_SSC_H
#define QLDPC_KERNELS_POLAR_SSC_H

#include "qldpc_kernels_polar.h"
#include "qldpc_polar_ssc_core.h"

/* the 32 sign bits (L < 0) of R[], MSB-first */
template <class R> __device__ __forceinline__ uint32_t pl_ssc_signs32(const R *L)
{
    uint32_t c = 0u;
#pragma unroll
    for (int k = 0; k < 32; k++) c |= (uint32_t)(L[k] < 0) << (31 - k);
    return c;
}

/* a node of S = 2^SL leaves whose first leaf is bit POS of the block's words: beliefs L[S] in registers -> decisions into u, the returned bits
   of every finished node into x.  `frozen` is wave-uniform, so every branch is one the whole wave takes */
template <int SL, int POS, class M>
__device__ __forceinline__ void pl_ssc_node(const M &m, const typename M::reg *L, uint32_t frozen, uint32_t value, uint32_t &u, uint32_t &x)
{
    constexpr int S = 1 << SL;
    constexpr uint32_t FIELD = (0xffffffffu << (32 - S)) >> POS;
    if ((frozen & FIELD) == FIELD) {
        u |= value & FIELD;
        x |= pl_enc_word(value & FIELD, SL);
    } else if ((frozen & FIELD) == 0u) {
        uint32_t c = 0u;
#pragma unroll
        for (int k = 0; k < S; k++) c |= (uint32_t)(L[k] < 0) << (31 - POS - k);
        x |= c;
        u |= pl_enc_word(c, SL);
    } else if constexpr (SL > 0) {                               /* a single leaf is one of the two above */
        constexpr int H = S / 2;
        typename M::reg l[H];
#pragma unroll
        for (int k = 0; k < H; k++) l[k] = m.f(L[k], L[k + H]);
        pl_ssc_node<SL - 1, POS>(m, l, frozen, value, u, x);
#pragma unroll
        for (int k = 0; k < H; k++) l[k] = m.g(L[k], L[k + H], (x >> (31 - POS - k)) & 1u);
        pl_ssc_node<SL - 1, POS + H>(m, l, frozen, value, u, x);
        x ^= (x << H) & ((0xffffffffu << (32 - H)) >> POS);
    }
}

/* grid = groups, 64 lanes.  SL = log2 of a leaf block; TOP: the block is the whole frame (n = SL <= 5), read from the caller's rows, and the plan
   is not looked at.  steps: the code's plan [n_steps][PL_SSC_STEP]; want_u: the call reads the U rows (d_u or d_info asked for); the other
   arguments are pl_decode's */
template <class M, int SL, bool TOP>
__global__ __launch_bounds__(PL_GROUP) void pl_ssc_decode(M m, int n, int n_frames, const typename M::mem *__restrict__ llr, const uint32_t *__restrict__ fmask,
                                                          const uint32_t *__restrict__ fval, const int *__restrict__ steps, int n_steps, bool want_u,
                                                          typename M::mem *B, uint32_t *Us, uint32_t *Xs)
{
    typedef typename M::mem mem;
    typedef typename M::reg reg;
    const unsigned lane = threadIdx.x;
    const size_t g = blockIdx.x, frame = g * PL_GROUP + lane;
    if (frame >= (size_t)n_frames) return;                       /* stores nothing; no other lane waits for this one */
    const size_t N = (size_t)1 << n, W = (size_t)pl_words(n);
    uint32_t *U = Us + g * W * PL_GROUP + lane, *X = Xs + g * W * PL_GROUP + lane;
    reg R[32];
    if constexpr (TOP) {
        constexpr int S = 1 << SL;
#pragma unroll
        for (int i = 0; i < S; i++) R[i] = m.load(llr[frame * N + i]);
        uint32_t u = 0u, x = 0u;
        pl_ssc_node<SL, 0>(m, R, fmask[0], fval ? fval[frame] : 0u, u, x);
        U[0] = u;
        X[0] = x;
    } else {
        pl_quad<mem> *Vw = (pl_quad<mem> *)(B + g * pl_group_elems(n)) + lane;
        const pl_quad<mem> *V = Vw;
        for (int i = 0; i < n_steps; i++) {
            const size_t j = (size_t)steps[i * PL_SSC_STEP];
            const int lam = steps[i * PL_SSC_STEP + 1], kind = steps[i * PL_SSC_STEP + 2];
            const size_t cnt = (size_t)1 << (lam - PL_SUB_LOG);
            const int top = j == 0 ? n - 1 : pl_ctz((long)j) + PL_SUB_LOG;
            for (int l = top; l >= (kind == PL_SSC_RATE0 ? lam + 1 : lam); l--) {      /* level l from level l + 1 */
                const size_t qs = pl_level_off(n, l + 1) / 4u, qd = pl_level_off(n, l) / 4u, h = (size_t)1 << l;
                const bool is_g = j != 0 && l == top, own = l == lam;      /* own: the node's level (rate 1 or mixed), used and not stored */
                const size_t w0 = j - (h >> 5);                  /* g: the node of h leaves that ends where the step begins */
                for (size_t k = 0; k < h; k += 32u) {
                    const uint32_t cw = is_g ? X[(w0 + (k >> 5)) * PL_GROUP] : 0u;
                    pl_pair32(m, V, qs + k / 4u, qs + (h + k) / 4u, is_g, cw, R);
                    if (!own) pl_store32<M>(Vw, qd + k / 4u, R);
                    else if (kind == PL_SSC_RATE1) X[(j + (k >> 5)) * PL_GROUP] = pl_ssc_signs32(R);
                }
            }
            if (kind == PL_SSC_RATE0) {
                for (size_t k = 0; k < cnt; k++) {
                    const uint32_t u = fval ? fval[frame * W + j + k] : 0u;
                    U[(j + k) * PL_GROUP] = u;
                    X[(j + k) * PL_GROUP] = pl_enc_word(u, PL_SUB_LOG);
                    pl_ssc_combine(X, (long)(j + k), PL_GROUP, 1, (long)cnt);
                }
            } else if (kind == PL_SSC_RATE1) {
                if (lam == n) {                                  /* a rate-1 root: the signs of level n itself */
                    for (size_t k = 0; k < cnt; k++) {
                        uint32_t c = 0u;
#pragma unroll
                        for (int q = 0; q < 8; q++) {
                            const pl_quad<mem> v = V[(8u * k + q) * PL_GROUP];
#pragma unroll
                            for (int e = 0; e < 4; e++) c |= (uint32_t)(v.v[e] < 0) << (31 - 4 * q - e);
                        }
                        X[k * PL_GROUP] = c;
                    }
                }
                if (want_u)
                    for (size_t k = 0; k < cnt; k++) {
                        U[(j + k) * PL_GROUP] = pl_enc_word(X[(j + k) * PL_GROUP], PL_SUB_LOG);
                        pl_ssc_combine(U, (long)(j + k), PL_GROUP, 1, (long)cnt);
                    }
            } else {
                uint32_t u = 0u, x = 0u;
                pl_ssc_node<PL_SUB_LOG, 0>(m, R, fmask[j], fval ? fval[frame * W + j] : 0u, u, x);
                U[j * PL_GROUP] = u;
                X[j * PL_GROUP] = x;
            }
            pl_ssc_combine(X, (long)(j + cnt - 1), PL_GROUP, (long)cnt, (long)W);
        }
    }
}

#endif /* QLDPC_KERNELS_POLAR_SSC_H */
