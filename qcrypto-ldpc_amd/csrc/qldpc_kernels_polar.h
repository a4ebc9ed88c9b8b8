/*
 * qldpc_kernels_polar.h -- the kernels of qldpc_polar_*: the SC decoder with lanes over frames, and the encoder.  The rules are qldpc_polar_core.h's.
 *
 * DECODER.  The SC traversal is the same for every frame, so a wave of 64 lanes decodes 64 frames (a GROUP) without divergence and without talking
 * to any other lane: no barrier, no LDS, no atomics.  A lane's decisions are packed words of its own, which is the rows' format already: the 32
 * decisions of a leaf block are ONE register, its re-encoded word is shifts and masks, and every partial-sum combine above a block is a word XOR.
 *
 *   beliefs    of the current path, per group: the levels n (the input), n - 1, .., 6 (level l = 2^l beliefs), 2N - 64 elements per lane, in the
 *              context's scratch.  Four neighbouring elements of a lane lie together and the lanes' quads follow each other (element e of lane t at
 *              (e / 4 * 64 + t) * 4 + e % 4), so that a wave reads or writes 64 quads in a row with one dword (int8) or dwordx4 (float) per lane.
 *              pl_load transposes the caller's frame-major rows into level n (and clamps int8 levels).
 *   levels >= 6  pl_decode produces level l from level l + 1 in steps of 32 elements: 16 quad loads issued together, 32 f or g (pl_pair32), 8 quad stores
 *              (pl_store32); the list decoder's levels >= 5 take the same step.  g reads its 32 re-encoded bits from one word of the lane's x row.
 *              pl_block_beliefs is that descent for one leaf block, which the tally form (qldpc_kernels_polar_tally.h) takes too.
 *   levels <= 5  a leaf block (32 leaves; all N where N < 32, then read from the caller's rows directly) lives in registers: 32 + 16 + .. + 1
 *              beliefs, the recursion unrolled by templates, the frozen flags of the block one wave-uniform word and its frozen values one word of
 *              the frame's frozen row.
 *   u, x rows  [group][word][lane] in the scratch; x holds the re-encoded word of every finished node (pl_combine_words with stride 64) and is the
 *              root's word at the end.  pl_outputs writes the rows the caller asked for, and the info bits in the order of info_pos.
 * A lane past n_frames returns at once and stores nothing; every index is 64 bits wide (max_frames N passes 2^31).
 *
 * ENCODER.  pl_encode_tiles: a workgroup takes PL_ENC_TILE words of one row into LDS, the stages below 32 inside each word on the way in
 * (pl_enc_word), the word stages up to the tile in LDS.  pl_encode_columns: the stages above a tile, a thread per column of words PL_ENC_TILE
 * apart, in place (nobody else touches its column).  The kernels that are no templates are static: the list decoder's unit
 * (qldpc_kernels_polar_list.h) includes this file too.
 */
#ifndef QLDPC_KERNELS_POLAR_H
#define QLDPC_KERNELS_POLAR_H

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "qldpc_polar_core.h"

#define PL_GROUP 64                /* frames of a wave */
#define PL_ENC_TILE_LOG 10
#define PL_ENC_TILE (1 << PL_ENC_TILE_LOG)      /* words of a row a workgroup of the encoder holds in LDS */
#define PL_ENC_LANES 256

template <class T> struct alignas(4 * sizeof(T)) pl_quad { T v[4]; };

/* the two message types: mem = what the scratch and the caller's rows hold, reg = what a lane computes with */
struct pl_msg_i8 {
    typedef int8_t mem;
    typedef int reg;
    int maxq;
    __device__ __forceinline__ reg load(mem v) const { return pl_i8_load((int)v, maxq); }
    __device__ __forceinline__ reg f(reg a, reg b) const { return pl_i8_f(a, b); }
    __device__ __forceinline__ reg g(reg a, reg b, unsigned c) const { return pl_i8_g(a, b, c, maxq); }
};
struct pl_msg_f32 {
    typedef float mem;
    typedef float reg;
    __device__ __forceinline__ reg load(mem v) const { return v; }
    __device__ __forceinline__ reg f(reg a, reg b) const { return pl_f32_f(a, b); }
    __device__ __forceinline__ reg g(reg a, reg b, unsigned c) const { return pl_f32_g(a, b, c); }
};

/* elements per lane before level l in a group's scratch, and a group's elements */
__host__ __device__ static inline size_t pl_level_off(int n, int l) { return ((size_t)2 << n) - ((size_t)2 << l); }
__host__ __device__ static inline size_t pl_group_elems(int n) { return n > PL_SUB_LOG ? (((size_t)2 << n) - 64u) * PL_GROUP : 0; }

/* frame-major rows -> level n of every group; grid = groups x N / 64 (tiles of a group together), 256 lanes, a tile of 64 frames x 64 elements through LDS */
template <class M>
__global__ __launch_bounds__(256) void pl_load(M m, int n, int n_frames, const typename M::mem *__restrict__ llr, typename M::mem *__restrict__ B)
{
    typedef typename M::mem mem;
    __shared__ mem tile[64][64 + 4];
    const size_t N = (size_t)1 << n, tiles = N / 64u, e0 = ((size_t)blockIdx.x % tiles) * 64u, g = (size_t)blockIdx.x / tiles;
    const unsigned t = threadIdx.x, c = t & 63u, r0 = t >> 6;
    for (unsigned r = r0; r < 64u; r += 4u) {                    /* row r of the tile: frame 64 g + r, elements e0 .. e0 + 63 */
        const size_t frame = g * PL_GROUP + r;
        tile[r][c] = frame < (size_t)n_frames ? (mem)m.load(llr[frame * N + e0 + c]) : (mem)0;
    }
    __syncthreads();
    pl_quad<mem> *V = (pl_quad<mem> *)(B + g * pl_group_elems(n)) + c;      /* lane c of the group */
    for (unsigned q = r0; q < 16u; q += 4u) {
        pl_quad<mem> v;
#pragma unroll
        for (int e = 0; e < 4; e++) v.v[e] = tile[c][4u * q + e];
        V[(e0 / 4u + q) * PL_GROUP] = v;
    }
}

/* out[k] = f or g of elements k and k + h (quads qa + k / 4 and qb + k / 4 of the lane), k < 32; cw: the 32 re-encoded bits g reads */
template <class M>
__device__ __forceinline__ void pl_pair32(const M &m, const pl_quad<typename M::mem> *V, size_t qa, size_t qb, bool is_g, uint32_t cw, typename M::reg *out)
{
    pl_quad<typename M::mem> a[8], b[8];
#pragma unroll
    for (int i = 0; i < 8; i++) a[i] = V[(qa + i) * PL_GROUP];
#pragma unroll
    for (int i = 0; i < 8; i++) b[i] = V[(qb + i) * PL_GROUP];
    if (is_g) {
#pragma unroll
        for (int k = 0; k < 32; k++) out[k] = m.g((typename M::reg)a[k >> 2].v[k & 3], (typename M::reg)b[k >> 2].v[k & 3], (cw >> (31 - k)) & 1u);
    } else {
#pragma unroll
        for (int k = 0; k < 32; k++) out[k] = m.f((typename M::reg)a[k >> 2].v[k & 3], (typename M::reg)b[k >> 2].v[k & 3]);
    }
}

/* the 32 beliefs R[] of a level step -> the quads q0 .. q0 + 7 of the lane */
template <class M>
__device__ __forceinline__ void pl_store32(pl_quad<typename M::mem> *V, size_t q0, const typename M::reg *R)
{
#pragma unroll
    for (int i = 0; i < 8; i++) {
        pl_quad<typename M::mem> v;
#pragma unroll
        for (int e = 0; e < 4; e++) v.v[e] = (typename M::mem)R[4 * i + e];
        V[(q0 + i) * PL_GROUP] = v;
    }
}

/* a node of S leaves whose first leaf is bit POS (MSB-first) of the block's words: beliefs L[S] in registers -> decisions into u, the re-encoded
   bits of every finished node into x, leaf beliefs into leaf[] */
template <int S, int POS, class M>
__device__ __forceinline__ void pl_node(const M &m, const typename M::reg *L, uint32_t frozen, uint32_t value, uint32_t &u, uint32_t &x, typename M::reg *leaf)
{
    if constexpr (S == 1) {
        const uint32_t bit = pl_leaf_bit(L[0] < 0, (frozen >> (31 - POS)) & 1u, (value >> (31 - POS)) & 1u);
        u |= bit << (31 - POS);
        x |= bit << (31 - POS);
        leaf[POS] = L[0];
    } else {
        constexpr int H = S / 2;
        typename M::reg l[H];
#pragma unroll
        for (int k = 0; k < H; k++) l[k] = m.f(L[k], L[k + H]);
        pl_node<H, POS>(m, l, frozen, value, u, x, leaf);
#pragma unroll
        for (int k = 0; k < H; k++) l[k] = m.g(L[k], L[k + H], (x >> (31 - POS - k)) & 1u);
        pl_node<H, POS + H>(m, l, frozen, value, u, x, leaf);
        x ^= (x << H) & ((0xffffffffu << (32 - H)) >> POS);
    }
}

/* the 32 beliefs R[] of leaf block j of a frame of n > 5 levels: the levels above the block that change with it, from the lane's quads V (= Vw)
   and its x row X (stride PL_GROUP), written back level by level; level 5 stays in registers */
template <class M>
__device__ __forceinline__ void pl_block_beliefs(const M &m, int n, size_t j, const pl_quad<typename M::mem> *V, pl_quad<typename M::mem> *Vw, const uint32_t *X,
                                                 typename M::reg *R)
{
    const int top = j == 0 ? n - 1 : pl_ctz((long)j) + PL_SUB_LOG;
    for (int l = top; l > PL_SUB_LOG; l--) {               /* level l from level l + 1 */
        const size_t qs = pl_level_off(n, l + 1) / 4u, qd = pl_level_off(n, l) / 4u, h = (size_t)1 << l;
        const bool is_g = j != 0 && l == top;
        const size_t w0 = j - (h >> 5);                  /* g: the node of h leaves that ends where block j begins */
        for (size_t k = 0; k < h; k += 32u) {
            const uint32_t cw = is_g ? X[(w0 + (k >> 5)) * PL_GROUP] : 0u;
            pl_pair32(m, V, qs + k / 4u, qs + (h + k) / 4u, is_g, cw, R);
            pl_store32<M>(Vw, qd + k / 4u, R);
        }
    }
    const bool is_g = j != 0 && top == PL_SUB_LOG;
    const size_t q6 = pl_level_off(n, PL_SUB_LOG + 1) / 4u;
    pl_pair32(m, V, q6, q6 + 8u, is_g, is_g ? X[(j - 1u) * PL_GROUP] : 0u, R);
}

/* grid = groups, 64 lanes.  SL = log2 of a leaf block; TOP: the block is the whole frame (n = SL <= 5) and is read from the caller's rows.
   fmask: the code's frozen flags, a row; fval: the frames' frozen values [n_frames][W] or NULL; Us, Xs: [groups][W][64]; leaf: [n_frames][N] or NULL */
template <class M, int SL, bool TOP>
__global__ __launch_bounds__(PL_GROUP) void pl_decode(M m, int n, int n_frames, const typename M::mem *__restrict__ llr, const uint32_t *__restrict__ fmask,
                                                      const uint32_t *__restrict__ fval, typename M::mem *B, uint32_t *Us, uint32_t *Xs,
                                                      typename M::mem *__restrict__ leaf_out)
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
        pl_node<S, 0>(m, R, fmask[j], fval ? fval[frame * W + j] : 0u, u, x, leaf);
        U[j * PL_GROUP] = u;
        X[j * PL_GROUP] = x;                                     /* = pl_enc_word(u, SL) */
        pl_combine_words(X, (long)j, PL_GROUP);
        if (leaf_out) {
#pragma unroll
            for (int i = 0; i < S; i++) leaf_out[frame * N + j * S + i] = (mem)leaf[i];
        }
    }
}

/* the rows the caller asked for, from the scratch: a thread per (group, word, lane), lanes fastest; info bit m = u[info_pos[m]] */
static __global__ __launch_bounds__(256) void pl_outputs(int n, int n_frames, int n_info, const int *__restrict__ info_pos, const uint32_t *__restrict__ Us,
                                                  const uint32_t *__restrict__ Xs, uint32_t *__restrict__ d_u, uint32_t *__restrict__ d_info, uint32_t *__restrict__ d_x)
{
    const size_t W = (size_t)pl_words(n), Wi = ((size_t)n_info + 31u) / 32u;
    const size_t idx = (size_t)blockIdx.x * 256u + threadIdx.x, lane = idx & 63u, w = (idx >> 6) % W, g = (idx >> 6) / W, frame = g * PL_GROUP + lane;
    if (frame >= (size_t)n_frames) return;
    const uint32_t *U = Us + g * W * PL_GROUP + lane;
    if (d_u) d_u[frame * W + w] = U[w * PL_GROUP];
    if (d_x) d_x[frame * W + w] = Xs[(g * W + w) * PL_GROUP + lane];
    if (d_info && w < Wi) d_info[frame * Wi + w] = pl_info_word(U, PL_GROUP, info_pos, n_info, w);
}

/* grid = frames x tiles of a row (a row's tiles together), PL_ENC_LANES lanes: T = min(W, PL_ENC_TILE) words of a row, the stages inside a word and the word stages below T.
   In place allowed: a workgroup reads its tile whole before it writes it */
static __global__ __launch_bounds__(PL_ENC_LANES) void pl_encode_tiles(int n, const uint32_t *u, uint32_t *x)
{
    __shared__ uint32_t s[PL_ENC_TILE];
    const size_t W = (size_t)pl_words(n), T = W < PL_ENC_TILE ? W : PL_ENC_TILE;
    const size_t base = (size_t)blockIdx.x * T;                /* W is a multiple of T */
    const unsigned t = threadIdx.x;
    const int sl = pl_sub_log(n);
    const uint32_t valid = pl_row_mask(n);
    for (size_t w = t; w < T; w += PL_ENC_LANES) s[w] = pl_enc_word(u[base + w] & valid, sl);
    __syncthreads();
    for (size_t h = 1; h < T; h <<= 1) {
        for (size_t p = t; p < T / 2u; p += PL_ENC_LANES) {
            const size_t a = (p / h) * 2u * h + p % h;
            s[a] ^= s[a + h];
        }
        __syncthreads();
    }
    for (size_t w = t; w < T; w += PL_ENC_LANES) x[base + w] = s[w];
}

/* the stages h = PL_ENC_TILE, 2 PL_ENC_TILE, .. of rows of W > PL_ENC_TILE words: a thread per (frame, column o < PL_ENC_TILE), in place on the words
   o + r PL_ENC_TILE, r < R = W / PL_ENC_TILE */
static __global__ __launch_bounds__(PL_ENC_LANES) void pl_encode_columns(int n, int n_frames, uint32_t *x)
{
    const size_t W = (size_t)pl_words(n), R = W >> PL_ENC_TILE_LOG;
    const size_t idx = (size_t)blockIdx.x * PL_ENC_LANES + threadIdx.x, o = idx & (PL_ENC_TILE - 1u), frame = idx >> PL_ENC_TILE_LOG;
    if (frame >= (size_t)n_frames) return;
    uint32_t *col = x + frame * W + o;
    for (size_t h = 1; h < R; h <<= 1)
        for (size_t p = 0; p < R / 2u; p++) {
            const size_t a = (p / h) * 2u * h + p % h;
            col[a << PL_ENC_TILE_LOG] ^= col[(a + h) << PL_ENC_TILE_LOG];
        }
}

#endif /* QLDPC_KERNELS_POLAR_H */
