/*
 * qldpc_kernels_polar_wide.h -- the WIDE form of the SC decoder of qldpc_polar_*: one workgroup per frame, lanes over the beliefs of a node.  The
 * rules are qldpc_polar_core.h's, the message types and the leaf block (pl_node) qldpc_kernels_polar.h's, the memory plan
 * qldpc_polar_wide_core.h's.  Every f and g is element-wise, so this form equals the lanes form and the host mirror bit for bit.
 *
 *   schedule   the one pl_decode walks: before leaf block j the levels top .. 6 are produced from the level above, top = n - 1 for j = 0 and
 *              ctz(j) + 5 otherwise; for j > 0 level top is a g over the re-encoded words that end where block j begins.
 *   a level    all lanes stride over its quads: one dword (int8) or dwordx4 (float) from each half of the level above, four f or g, one store.
 *              Level n - 1 reads the caller's row element by element (no alignment is asked of it) and clamps int8 levels.  One workgroup
 *              barrier follows each level.
 *   leaf block the first 32 lanes of wave 0, leaf t on lane t (plw_leaf_lanes): level 5 from the 64 beliefs of level 6 in LDS, then the 62 node
 *              visits of the block's serial chain, each one f or g on every lane and one or two lane moves.  A lone wave issues an instruction
 *              every 4 cycles whatever its lanes do, so the block costs what it has instructions: on one lane (pl_node<32, 0>, kept behind
 *              leaf_lanes = 0) it has about 3 500 and takes 5.7 us, on 32 lanes about 1 600 and takes 3.8 us (profiles/polar_wide_cost.json);
 *              this is where a frame's time goes.  What the block needs is on chip: the window's frozen flags and values, its decisions and its
 *              re-encoded words; the nodes below 64 words are combined there (pl_combine_words), a stage on as many lanes as it has words.
 *   a window   of PLW_WIN blocks ends with its words written out by 64 lanes and the combines of 64 words and more spread over all lanes, a
 *              barrier between two stages.
 *   barriers   every one sits in control flow that depends on n, C and j only, which all lanes share; no lane returns early (grid = n_frames).
 *              A frame's scratch and rows are touched by its own workgroup only: no atomics, no spinning, nothing between workgroups.
 * Every index is 64 bits wide (max_frames N passes 2^31).
 */
#ifndef QLDPC_KERNELS_POLAR_WIDE_H
#define QLDPC_KERNELS_POLAR_WIDE_H

#include "qldpc_kernels_polar.h"
#include "qldpc_polar_wide_core.h"

/* level dst (h elements) from the 2h elements of src.  RAW: src is the caller's row.  g reads bit k of the node that starts at word w0: from the
   window xw where in_win, else from the row X */
template <class M, bool RAW>
__device__ __forceinline__ void plw_level(const M &m, const typename M::mem *src, typename M::mem *dst, size_t h, bool is_g, bool in_win,
                                          const uint32_t *xw, const uint32_t *X, size_t w0, unsigned tid, unsigned lanes)
{
    typedef typename M::mem mem;
    typedef typename M::reg reg;
    for (size_t q = tid; q < h / 4u; q += lanes) {
        const size_t k = 4u * q;
        reg a[4], b[4];
        if constexpr (RAW) {
#pragma unroll
            for (int e = 0; e < 4; e++) { a[e] = m.load(src[k + e]); b[e] = m.load(src[h + k + e]); }
        } else {
            const pl_quad<mem> va = *(const pl_quad<mem> *)(src + k), vb = *(const pl_quad<mem> *)(src + h + k);
#pragma unroll
            for (int e = 0; e < 4; e++) { a[e] = (reg)va.v[e]; b[e] = (reg)vb.v[e]; }
        }
        pl_quad<mem> v;
        if (is_g) {
            const size_t w = w0 + (k >> 5);
            const uint32_t cw = (in_win ? xw[w & (PLW_WIN - 1u)] : X[w]) << (k & 31u);      /* bit k + e at 31 - e */
#pragma unroll
            for (int e = 0; e < 4; e++) v.v[e] = (mem)m.g(a[e], b[e], (cw >> (31 - e)) & 1u);
        } else {
#pragma unroll
            for (int e = 0; e < 4; e++) v.v[e] = (mem)m.f(a[e], b[e]);
        }
        *(pl_quad<mem> *)(dst + k) = v;
    }
}

/* belief k of level 5 of a leaf block from a and b, the beliefs k and 32 + k of level 6 as they lie in memory (RAW: in the caller's row, to be
   clamped; else in LDS): a g with bit k of cw, the re-encoded word of the block before, or an f.  The loads are the caller's: a lane of the
   32-lane block reads its two beliefs, the one-lane block reads level 6 by quads, which holds its instruction count */
template <class M, bool RAW>
__device__ __forceinline__ typename M::reg plw_level5(const M &m, typename M::mem a, typename M::mem b, bool is_g, uint32_t cw, unsigned k)
{
    typedef typename M::reg reg;
    const reg ra = RAW ? m.load(a) : (reg)a, rb = RAW ? m.load(b) : (reg)b;
    return is_g ? m.g(ra, rb, (cw >> (31u - k)) & 1u) : m.f(ra, rb);
}

/* lane t's copy of the value of lane t ^ (1 << log) among the first 32 lanes of a wave, all 32 at work: moves inside a row of 16 lanes
   (quad permutes; a quad reverse and a half-row mirror make t ^ 4; a row rotation by 8), a swizzle across the two rows */
__device__ __forceinline__ int plw_xor_lane(int v, int log)
{
    switch (log) {
    case 0: return __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, false);      /* quad_perm:[1,0,3,2] */
    case 1: return __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, false);      /* quad_perm:[2,3,0,1] */
    case 2: return __builtin_amdgcn_update_dpp(0, __builtin_amdgcn_update_dpp(0, v, 0x1B, 0xF, 0xF, false), 0x141, 0xF, 0xF, false);      /* [3,2,1,0], row_half_mirror */
    case 3: return __builtin_amdgcn_update_dpp(0, v, 0x128, 0xF, 0xF, false);     /* row_ror:8 */
    default: return __builtin_amdgcn_ds_swizzle(v, 0x401F);                       /* bit mode: and 0x1f, or 0, xor 0x10 */
    }
}
__device__ __forceinline__ float plw_xor_lane(float v, int log) { return __int_as_float(plw_xor_lane(__float_as_int(v), log)); }

/* A leaf block over the first 32 lanes of a wave, leaf t on lane t: what pl_node<32, 0> computes on one lane, in under half the instructions.
   b5: the lane's belief of level 5.  Lane t holds, per level l, the belief of its place in the node of 2^l leaves around it; before leaf i the
   levels top .. 0 (top = 4 for i = 0, else ctz(i)) are renewed, level l from the lane's own belief of level l + 1 and that of lane t ^ 2^l: a g
   (with the re-encoded bit of lane t ^ 2^l) at level top for i > 0, an f elsewhere.  Every lane computes, and the lanes of the node that holds
   leaf i read lanes of the node above only, so what the others compute is never used.  xb: the lane's re-encoded bit of the last finished node
   around it.  -> the block's decisions and re-encoded word (the same on every lane) and the lane's leaf belief */
template <class M>
__device__ __forceinline__ void plw_leaf_lanes(const M &m, typename M::reg b5, unsigned t, uint32_t frozen, uint32_t value, uint32_t &u, uint32_t &x,
                                               typename M::reg &leaf)
{
    typedef typename M::reg reg;
    reg B[6];
    B[5] = b5;
    leaf = b5;
    const unsigned fz = (frozen >> (31u - t)) & 1u, fv = (value >> (31u - t)) & 1u;
    int xb = 0;
#pragma unroll
    for (int i = 0; i < 32; i++) {
        const int top = i == 0 ? 4 : __builtin_ctz((unsigned)i);
#pragma unroll
        for (int l = 4; l >= 0; l--) {
            if (l > top) continue;
            /* f is symmetric in its two beliefs, bit for bit; a g counts on the lanes of the second half only, whose own belief is b */
            const reg own = B[l + 1], other = plw_xor_lane(own, l);
            if (i != 0 && l == top) B[l] = m.g(other, own, (unsigned)plw_xor_lane(xb, l));
            else B[l] = m.f(own, other);
        }
        if (t == (unsigned)i) {
            leaf = B[0];
            xb = (int)pl_leaf_bit(B[0] < 0, fz, fv);
        }
#pragma unroll
        for (int l = 0; l < 5; l++) {                             /* the nodes that end with leaf i: first half ^= second half */
            if (!((i >> l) & 1)) break;
            const int o = plw_xor_lane(xb, l);
            if ((t >> l) == (((unsigned)i >> l) ^ 1u)) xb ^= o;   /* the first half of the node of 2^(l + 1) leaves that ends with leaf i */
        }
    }
    x = __brev((uint32_t)__ballot(xb));                           /* lane t is bit t of the ballot and bit 31 - t of a word */
    u = pl_enc_word(x, PL_SUB_LOG);                               /* the encoder is an involution: the decisions from their re-encoded word */
}

/* grid = n_frames, LANES lanes, plw_lds_elems(n, C) elements of dynamic LDS; n >= 6, C = plw_chip(n, the context's chip level).
   leaf_lanes: the leaf block on 32 lanes (plw_leaf_lanes) or, 0, on one (pl_node).
   fmask: the code's frozen flags, a row; fval: the frames' frozen values [n_frames][W] or NULL; S: [n_frames][plw_scratch_elems(n, C)];
   Us, Xs: the context's rows [n_frames][W], used where the caller gives no d_u / d_x; d_info, leaf_out: [n_frames][..] or NULL */
template <class M, int LANES>
__global__ __launch_bounds__(LANES) void plw_decode(M m, int n, int C, int leaf_lanes, const typename M::mem *__restrict__ llr, const uint32_t *__restrict__ fmask,
                                                    const uint32_t *__restrict__ fval, typename M::mem *S, uint32_t *Us, uint32_t *Xs, uint32_t *d_u,
                                                    uint32_t *d_x, uint32_t *__restrict__ d_info, int n_info, const int *__restrict__ info_pos,
                                                    typename M::mem *__restrict__ leaf_out)
{
    typedef typename M::mem mem;
    typedef typename M::reg reg;
    extern __shared__ __align__(16) unsigned char plw_lds[];
    __shared__ uint32_t xw[PLW_WIN], uw[PLW_WIN], fmw[PLW_WIN], fvw[PLW_WIN];
    mem *lds = (mem *)plw_lds;
    const unsigned tid = threadIdx.x;
    const size_t frame = blockIdx.x, N = (size_t)1 << n, W = N >> 5, win = plw_win_words(n);
    const mem *in = llr + frame * N;
    mem *Sf = S + frame * plw_scratch_elems(n, C);
    uint32_t *U = (d_u ? d_u : Us) + frame * W, *X = (d_x ? d_x : Xs) + frame * W;
    for (size_t j = 0; j < W; j++) {
        const size_t jw = j & (PLW_WIN - 1u);
        if (jw == 0 && tid < win) {                              /* the window's frozen flags and values; the last window's were read before its flush */
            fmw[tid] = fmask[j + tid];
            fvw[tid] = fval ? fval[frame * W + j + tid] : 0u;
        }
        const int top = j == 0 ? n - 1 : pl_ctz((long)j) + PL_SUB_LOG;
        if (top > PL_SUB_LOG || jw == 0) __syncthreads();       /* lane 0 is done with level 6 and with the window's words */
        for (int l = top; l > PL_SUB_LOG; l--) {                  /* level l from level l + 1 */
            const size_t h = (size_t)1 << l, w0 = j - (h >> 5);  /* g: the node of h leaves that ends where block j begins */
            const bool is_g = j != 0 && l == top, in_win = plw_g_in_window(l);
            if (l > C) {
                if (l + 1 == n) plw_level<M, true>(m, in, Sf + plw_level_off(n, l), h, is_g, in_win, xw, X, w0, tid, LANES);
                else plw_level<M, false>(m, Sf + plw_level_off(n, l + 1), Sf + plw_level_off(n, l), h, is_g, in_win, xw, X, w0, tid, LANES);
            } else {
                if (l + 1 == n) plw_level<M, true>(m, in, lds + plw_lds_off(C, l), h, is_g, in_win, xw, X, w0, tid, LANES);
                else if (l + 1 > C) plw_level<M, false>(m, Sf + plw_level_off(n, l + 1), lds + plw_lds_off(C, l), h, is_g, in_win, xw, X, w0, tid, LANES);
                else plw_level<M, false>(m, lds + plw_lds_off(C, l + 1), lds + plw_lds_off(C, l), h, is_g, in_win, xw, X, w0, tid, LANES);
            }
            __syncthreads();
        }
        /* the leaf block: level 5 is a g after a block with no level above to renew; level 6 is the caller's row or the lowest level in LDS */
        const bool is_g5 = j != 0 && top == PL_SUB_LOG, raw6 = n == PL_SUB_LOG + 1;
        const mem *l6 = lds + plw_lds_off(C, PL_SUB_LOG + 1);
        if (leaf_lanes) {                                         /* leaf t on lane t */
            if (tid < 32u) {
                uint32_t u, x;
                reg leaf;
                const uint32_t cw = is_g5 ? xw[jw - 1u] : 0u;
                const reg b5 = raw6 ? plw_level5<M, true>(m, in[tid], in[32u + tid], is_g5, cw, tid) : plw_level5<M, false>(m, l6[tid], l6[32u + tid], is_g5, cw, tid);
                plw_leaf_lanes(m, b5, tid, fmw[jw], fvw[jw], u, x, leaf);
                if (leaf_out) leaf_out[frame * N + j * 32u + tid] = (mem)leaf;
                if (tid == 0) {
                    uw[jw] = u;
                    xw[jw] = x;
                }
                /* pl_combine_words below a window, a stage on as many lanes as it has words.  These lanes are one wave, whose LDS accesses
                   are served in the order it issues them; the wave barrier keeps the compiler from changing that order */
                for (size_t h = 1; h < PLW_WIN && (j & h); h <<= 1) {
                    __builtin_amdgcn_wave_barrier();
                    if (tid < h) xw[jw + 1u - 2u * h + tid] ^= xw[jw + 1u - h + tid];
                }
                __builtin_amdgcn_wave_barrier();
            }
        } else if (tid == 0) {                                    /* the leaf block on one lane */
            reg R[32], leaf[32];
            const uint32_t cw = is_g5 ? xw[jw - 1u] : 0u;
            if (raw6) {
#pragma unroll
                for (int k = 0; k < 32; k++) R[k] = plw_level5<M, true>(m, in[k], in[32 + k], is_g5, cw, (unsigned)k);
            } else {
                const pl_quad<mem> *V = (const pl_quad<mem> *)l6;
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    const pl_quad<mem> a = V[i], b = V[8 + i];
#pragma unroll
                    for (int e = 0; e < 4; e++) R[4 * i + e] = plw_level5<M, false>(m, a.v[e], b.v[e], is_g5, cw, (unsigned)(4 * i + e));
                }
            }
            uint32_t u = 0u, x = 0u;
            pl_node<32, 0>(m, R, fmw[jw], fvw[jw], u, x, leaf);
            uw[jw] = u;
            xw[jw] = x;                                           /* = pl_enc_word(u, 5) */
            for (size_t h = 1; h < PLW_WIN && (j & h); h <<= 1)   /* pl_combine_words below a window, which holds every such node whole */
                for (size_t k = 0; k < h; k++) xw[jw + 1u - 2u * h + k] ^= xw[jw + 1u - h + k];
            if (leaf_out) {
#pragma unroll
                for (int i = 0; i < 32; i++) leaf_out[frame * N + j * 32u + i] = (mem)leaf[i];
            }
        }
        if (jw == PLW_WIN - 1u || j == W - 1u) {                  /* the window is full: out with its words, then the combines of 64 words and more */
            __syncthreads();
            const size_t base = j - jw;
            if (tid < win) { U[base + tid] = uw[tid]; X[base + tid] = xw[tid]; }
            for (size_t h = PLW_WIN; j & h; h <<= 1) {
                __syncthreads();
                for (size_t k = tid; k < h; k += LANES) X[j + 1u - 2u * h + k] ^= X[j + 1u - h + k];
            }
        }
    }
    __syncthreads();
    if (d_info) {                                                 /* info bit i = u[info_pos[i]], the caller's order */
        const size_t Wi = ((size_t)n_info + 31u) / 32u;
        for (size_t w = tid; w < Wi; w += LANES) d_info[frame * Wi + w] = pl_info_word(U, 1, info_pos, n_info, w);
    }
}

#endif /* QLDPC_KERNELS_POLAR_WIDE_H */
