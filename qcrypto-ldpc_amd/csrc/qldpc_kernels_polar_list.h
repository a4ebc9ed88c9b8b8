/*
 * qldpc_kernels_polar_list.h -- the kernels of qldpc_polar_list_*: the CRC-aided SC list decoder with lanes over frames.  The rules are
 * qldpc_polar_list_core.h's, the encoder of the post-pass qldpc_kernels_polar.h's.
 *
 * DECODER.  As in the SC kernel a wave of 64 lanes decodes 64 frames (a GROUP), and a lane holds ALL paths of its frame.  The traversal and the
 * number of live paths P (it depends only on how many information leaves have passed) are then the same for every lane; only values and path
 * indices differ per lane, so no lane waits for another, nothing diverges, and there is no barrier, no LDS and no atomic.
 *
 *   no copy on a fork   every belief level l < n and every bit level has L slots per lane and a word of L slot pointers (nibbles) per lane, held in
 *              registers.  A step that writes level l writes path k's result into slot k and resets the word (every path rewrites the level in
 *              that step, and a level is read only while a lower one is written); a read of level l + 1 goes through the path's pointer; at an
 *              information leaf new path k inherits all of its parent's pointers (pll_perm on the words that are still to be read).
 *   beliefs    per group, in the context's scratch, in quads as the SC kernel's (quad Q of lane t at (Q 64 + t) of the group): level n, the
 *              input, max(1, N / 4) quads, then for l = 1 .. n - 1 the L slots of max(1, 2^l / 4) quads each (pll_quad_off).  Level 0, a path's
 *              leaf belief, is a register.  Levels >= 5 are produced 32 elements at a time (pl_pair32: 16 quad loads issued together).
 *   bits       the 32 re-encoded bits of the open leaf block are one register per path, moved by selects on a fork.  A finished left node of 2^b
 *              blocks is written into slot k of bit level b ([word][lane] in the scratch, pll_bit_off); g at that level and the combine when the
 *              right sibling finishes read it through the pointer, and the combine writes a higher level, so no step reads the level it writes.
 *   survivors  pll_select_*: a branch-free rank over at most 16 (metric, index) keys in registers; the parents' values by selects.
 *   decisions  u is not carried: the involution gives u = encode(x).  pll_roots copies the L root words of a frame into rows, pl_encode_tiles
 *              encodes them, pll_crc takes every path's remainder and pll_outputs picks and writes what the caller asked for.
 * A lane past n_frames returns at once and stores nothing; every index is 64 bits wide.
 */
#ifndef QLDPC_KERNELS_POLAR_LIST_H
#define QLDPC_KERNELS_POLAR_LIST_H

#include "qldpc_kernels_polar.h"
#include "qldpc_polar_list_core.h"

#define PLL_PTR_A 16               /* belief levels 1 .. 15 have a word of slot pointers */
#define PLL_PTR_B 12               /* bit levels 0 .. 11 */

/* the metric of a message type */
template <class M> struct pll_metric;
template <> struct pll_metric<pl_msg_i8> {
    typedef uint32_t type;
    __device__ static __forceinline__ type pen(int D) { return pll_i8_pen(D); }
    __device__ static __forceinline__ type none() { return 0xffffffffu; }
    __device__ static __forceinline__ uint32_t select(int P, int n_new, const type *m, const type *mf, int L) { return pll_select_i8(L, P, n_new, m, mf); }
};
template <> struct pll_metric<pl_msg_f32> {
    typedef float type;
    __device__ static __forceinline__ type pen(float D) { return pll_f32_pen(D); }
    __device__ static __forceinline__ type none() { return __builtin_inff(); }
    __device__ static __forceinline__ uint32_t select(int P, int n_new, const type *m, const type *mf, int L) { return pll_select_f32(L, P, n_new, m, mf); }
};

/* quads per lane of a slot of level l, before level l (1 <= l < n; level n, one slot, lies first), and of a group */
__host__ __device__ static inline size_t pll_quads(int l) { return l >= 2 ? (size_t)1 << (l - 2) : 1; }
__host__ __device__ static inline size_t pll_quad_off(int n, int L, int l) { return pll_quads(n) + (size_t)L * (l >= 2 ? (size_t)1 << (l - 2) : 0); }
__host__ __device__ static inline size_t pll_group_quads(int n, int L) { return pll_quads(n) + (size_t)L * (n >= 2 ? (size_t)1 << (n - 2) : 0); }

/* word i of a register array by a wave-uniform index: selects, so that the array stays in registers */
template <int CNT> __device__ __forceinline__ uint32_t pll_get(const uint32_t (&a)[CNT], int i)
{
    uint32_t v = 0u;
#pragma unroll
    for (int k = 0; k < CNT; k++) v = k == i ? a[k] : v;
    return v;
}
template <int CNT> __device__ __forceinline__ void pll_set(uint32_t (&a)[CNT], int i, uint32_t v)
{
#pragma unroll
    for (int k = 0; k < CNT; k++) a[k] = k == i ? v : a[k];
}

/* frame-major rows -> level n of every group, clamped; a thread per (group, quad, lane), lanes fastest */
template <class M>
__global__ __launch_bounds__(256) void pll_load(M m, int n, int L, int n_frames, const typename M::mem *__restrict__ llr, typename M::mem *__restrict__ A)
{
    typedef typename M::mem mem;
    const size_t N = (size_t)1 << n, QN = pll_quads(n);
    const size_t idx = (size_t)blockIdx.x * 256u + threadIdx.x, lane = idx & 63u, Q = (idx >> 6) % QN, g = (idx >> 6) / QN, frame = g * PL_GROUP + lane;
    if (frame >= (size_t)n_frames) return;
    pl_quad<mem> v;
#pragma unroll
    for (int e = 0; e < 4; e++) v.v[e] = 4u * Q + e < N ? (mem)m.load(llr[frame * N + 4u * Q + e]) : (mem)0;
    ((pl_quad<mem> *)A)[(g * pll_group_quads(n, L) + Q) * PL_GROUP + lane] = v;
}

/* grid = groups, 64 lanes.  fmask: the code's frozen flags, a row; fval: the frames' frozen values [n_frames][W] or NULL; A: the belief scratch;
   Bt: the bit levels, [group][word][lane]; metric_out: [n_frames][L] */
template <class M, int L>
__global__ __launch_bounds__(PL_GROUP) void pll_decode(M m, int n, int n_frames, const uint32_t *__restrict__ fmask, const uint32_t *__restrict__ fval,
                                                       typename M::mem *A, uint32_t *Bt, typename pll_metric<M>::type *__restrict__ metric_out)
{
    typedef typename M::mem mem;
    typedef typename M::reg reg;
    typedef pll_metric<M> MT;
    typedef typename MT::type met;
    const unsigned lane = threadIdx.x;
    const size_t g = blockIdx.x, frame = g * PL_GROUP + lane;
    if (frame >= (size_t)n_frames) return;                       /* stores nothing; no other lane waits for this one */
    const size_t N = (size_t)1 << n, W = (size_t)pl_words(n);
    pl_quad<mem> *V = (pl_quad<mem> *)A + g * pll_group_quads(n, L) * PL_GROUP + lane;
    uint32_t *X = Bt + g * pll_bit_words(L, n) * PL_GROUP + lane;
    uint32_t ptr_a[PLL_PTR_A], ptr_b[PLL_PTR_B], xw[L];
    met metric[L];
    reg D[L];
#pragma unroll
    for (int k = 0; k < PLL_PTR_A; k++) ptr_a[k] = PLL_IDENT;
#pragma unroll
    for (int k = 0; k < PLL_PTR_B; k++) ptr_b[k] = PLL_IDENT;
#pragma unroll
    for (int k = 0; k < L; k++) { xw[k] = 0u; metric[k] = 0; D[k] = 0; }
    int P = 1;
    uint32_t fm = 0u, fv = 0u;
    for (size_t i = 0; i < N; i++) {
        const int p = (int)(i & 31u);
        const size_t j = i >> 5;
        if (p == 0) { fm = fmask[j]; fv = fval ? fval[frame * W + j] : 0u; }
        const int top = i == 0 ? n - 1 : pl_ctz((long)i);
        for (int l = top; l >= 0; l--) {                         /* level l of every path from its level l + 1 */
            const bool is_g = i != 0 && l == top;
            const uint32_t pa = l + 1 == n ? 0u : pll_get(ptr_a, l + 1);
            const uint32_t pb = is_g && l >= PL_SUB_LOG ? pll_get(ptr_b, l - PL_SUB_LOG) : 0u;
            const size_t src0 = l + 1 == n ? 0 : pll_quad_off(n, L, l + 1), sq = pll_quads(l + 1);
#pragma unroll
            for (int k = 0; k < L; k++) {
                if (k >= P) continue;
                const size_t src = src0 + (l + 1 == n ? 0 : (size_t)pll_nib(pa, k) * sq);
                if (l >= PL_SUB_LOG) {                            /* 32 elements a step; g reads a word of the left sibling's slot */
                    const size_t hq = (size_t)1 << (l - 2), dst = pll_quad_off(n, L, l) + (size_t)k * hq;
                    const uint32_t *cw = X + (pll_bit_off(L, l - PL_SUB_LOG) + (size_t)pll_nib(pb, k) * (hq >> 3)) * PL_GROUP;
                    for (size_t q = 0; q < hq; q += 8u) {
                        reg R[32];
                        pl_pair32(m, V, src + q, src + hq + q, is_g, is_g ? cw[(q >> 3) * PL_GROUP] : 0u, R);
                        pl_store32<M>(V, dst + q, R);
                    }
                } else if (l >= 2) {                              /* 4, 8 or 16 elements; g reads the h places before p of the open block */
                    const size_t hq = (size_t)1 << (l - 2), dst = pll_quad_off(n, L, l) + (size_t)k * hq;
                    const int c0 = p - (1 << l);
                    for (size_t q = 0; q < hq; q++) {
                        const pl_quad<mem> a = V[(src + q) * PL_GROUP], b = V[(src + hq + q) * PL_GROUP];
                        pl_quad<mem> v;
#pragma unroll
                        for (int e = 0; e < 4; e++)
                            v.v[e] = (mem)(is_g ? m.g((reg)a.v[e], (reg)b.v[e], (xw[k] >> (31 - (c0 + 4 * (int)q + e))) & 1u) : m.f((reg)a.v[e], (reg)b.v[e]));
                        V[(dst + q) * PL_GROUP] = v;
                    }
                } else {                                          /* levels 1 and 0: one quad in; level 1 keeps a quad of its own, level 0 is D */
                    const pl_quad<mem> s = V[src * PL_GROUP];
                    if (l == 1) {
                        pl_quad<mem> v;
                        v.v[0] = (mem)(is_g ? m.g((reg)s.v[0], (reg)s.v[2], (xw[k] >> (31 - (p - 2))) & 1u) : m.f((reg)s.v[0], (reg)s.v[2]));
                        v.v[1] = (mem)(is_g ? m.g((reg)s.v[1], (reg)s.v[3], (xw[k] >> (31 - (p - 1))) & 1u) : m.f((reg)s.v[1], (reg)s.v[3]));
                        v.v[2] = (mem)0; v.v[3] = (mem)0;
                        V[(pll_quad_off(n, L, 1) + (size_t)k) * PL_GROUP] = v;
                    } else {
                        D[k] = is_g ? m.g((reg)s.v[0], (reg)s.v[1], (xw[k] >> (31 - (p - 1))) & 1u) : m.f((reg)s.v[0], (reg)s.v[1]);
                    }
                }
            }
            if (l) pll_set(ptr_a, l, PLL_IDENT);
        }
        if ((fm >> (31 - p)) & 1u) {                              /* frozen: every path takes the value and pays where its belief disagrees */
            const uint32_t bit = (fv >> (31 - p)) & 1u;
#pragma unroll
            for (int k = 0; k < L; k++) {
                if (k >= P) continue;
                if ((uint32_t)(D[k] < 0) != bit) metric[k] += MT::pen(D[k]);
                xw[k] |= bit << (31 - p);
            }
        } else {                                                  /* information: 2P candidates, the n_new smallest survive */
            const int n_new = 2 * P < L ? 2 * P : L;
            met mk[L], mf[L];
#pragma unroll
            for (int k = 0; k < L; k++) { mk[k] = metric[k]; mf[k] = metric[k] + MT::pen(D[k]); }
            const uint32_t sel = MT::select(P, n_new, mk, mf, L);
            uint32_t par = 0u, nx[L];
#pragma unroll
            for (int r = 0; r < L; r++) {
                if (r >= n_new) continue;
                const uint32_t c = pll_nib(sel, r) & 7u, flip = pll_nib(sel, r) >> 3;
                met cm = mk[0], cf = mf[0];
                uint32_t cx = xw[0], neg = (uint32_t)(D[0] < 0);
#pragma unroll
                for (int k = 1; k < L; k++) {
                    const bool is = c == (uint32_t)k;
                    cm = is ? mk[k] : cm; cf = is ? mf[k] : cf; cx = is ? xw[k] : cx; neg = is ? (uint32_t)(D[k] < 0) : neg;
                }
                metric[r] = flip ? cf : cm;
                nx[r] = cx | ((neg ^ flip) << (31 - p));
                par |= c << (4 * r);
            }
#pragma unroll
            for (int r = 0; r < L; r++) xw[r] = r < n_new ? nx[r] : xw[r];
            /* the pointers that are still to be read: level l' before its next rewrite iff bit l' - 1 of i is 0; bit level b iff bit b of j is 1 */
#pragma unroll
            for (int k = 1; k < PLL_PTR_A; k++)
                if (k < n && !((i >> (k - 1)) & 1u)) ptr_a[k] = pll_perm(ptr_a[k], par, L);
#pragma unroll
            for (int k = 0; k < PLL_PTR_B; k++)
                if ((j >> k) & 1u) ptr_b[k] = pll_perm(ptr_b[k], par, L);
            P = n_new;
        }
        /* every node of the open block that ends with this leaf, smallest first */
        for (int h = 1; p & h; h <<= 1) {
            const uint32_t first = (0xffffffffu << (32 - h)) >> (p + 1 - 2 * h);
#pragma unroll
            for (int k = 0; k < L; k++) xw[k] ^= (xw[k] << h) & first;
        }
        if (p == 31 || i == N - 1u) {                             /* the block is complete: the node of 2^t blocks that ends with it, into bit level t */
            const int t = pll_done_level((long)j);
            const size_t sz = (size_t)1 << t;
#pragma unroll
            for (int k = 0; k < L; k++) {
                if (k >= P) continue;
                uint32_t *dst = X + (pll_bit_off(L, t) + (size_t)k * sz) * PL_GROUP;
                dst[(sz - 1u) * PL_GROUP] = xw[k];
                for (int b = 0; b < t; b++) {
                    const size_t s = (size_t)1 << b;
                    const uint32_t *left = X + (pll_bit_off(L, b) + (size_t)pll_nib(pll_get(ptr_b, b), k) * s) * PL_GROUP;
                    for (size_t e = 0; e < s; e++) dst[(sz - 2u * s + e) * PL_GROUP] = left[e * PL_GROUP] ^ dst[(sz - s + e) * PL_GROUP];
                }
                xw[k] = 0u;
            }
            pll_set(ptr_b, t, PLL_IDENT);
        }
    }
#pragma unroll
    for (int k = 0; k < L; k++) metric_out[frame * L + k] = k < P ? metric[k] : MT::none();
}

/* the root words of every path, from the top bit level (path k in slot k) into rows LX[n_frames][L][W], zeros past the P live paths;
   a thread per (group, slot, word, lane), lanes fastest */
__global__ __launch_bounds__(256) void pll_roots(int n, int L, int P, int n_frames, const uint32_t *__restrict__ Bt, uint32_t *__restrict__ LX)
{
    const size_t W = (size_t)pl_words(n), idx = (size_t)blockIdx.x * 256u + threadIdx.x, lane = idx & 63u, w = (idx >> 6) % W, k = (idx >> 6) / W % (size_t)L,
                 g = (idx >> 6) / W / (size_t)L, frame = g * PL_GROUP + lane;
    if (frame >= (size_t)n_frames) return;
    const size_t root = pll_bit_off(L, pll_done_level((long)W - 1));
    LX[(frame * (size_t)L + k) * W + w] = k < (size_t)P ? Bt[(g * pll_bit_words(L, n) + root + k * W + w) * PL_GROUP + lane] : 0u;
}

/* the remainder of every live path's information bits: a thread per (frame, path); LU[n_frames][L][W] the paths' decisions */
__global__ __launch_bounds__(256) void pll_crc(int n, int L, int P, int n_frames, int n_info, const int *__restrict__ info_pos, int crc_len, uint32_t crc_poly,
                                               const uint32_t *__restrict__ LU, uint32_t *__restrict__ rem)
{
    const size_t W = (size_t)pl_words(n), idx = (size_t)blockIdx.x * 256u + threadIdx.x, k = idx % (size_t)L, frame = idx / (size_t)L;
    if (frame >= (size_t)n_frames || k >= (size_t)P) return;
    const uint32_t *U = LU + idx * W;
    uint32_t r = 0u;
    for (int m = 0; m < n_info; m++) {
        const int pos = info_pos[m];
        r = pll_crc_step(r, pl_bit(U[pos >> 5], pos), crc_len, crc_poly);
    }
    rem[idx] = r;
}

/* the pick and the rows the caller asked for: a thread per (frame, word), words fastest; metric as its 32 bits */
__global__ __launch_bounds__(256) void pll_outputs(int n, int L, int P, int n_frames, int n_info, const int *__restrict__ info_pos, const uint32_t *__restrict__ rem,
                                                   const uint32_t *__restrict__ d_crc, const uint32_t *__restrict__ LU, const uint32_t *__restrict__ LX,
                                                   const uint32_t *__restrict__ Mt, uint32_t *__restrict__ d_u, uint32_t *__restrict__ d_info,
                                                   uint32_t *__restrict__ d_x, int32_t *__restrict__ d_pick, uint32_t *__restrict__ d_metric,
                                                   uint32_t *__restrict__ d_list_x)
{
    const size_t W = (size_t)pl_words(n), Wi = ((size_t)n_info + 31u) / 32u, idx = (size_t)blockIdx.x * 256u + threadIdx.x, w = idx % W, frame = idx / W;
    if (frame >= (size_t)n_frames) return;
    const uint32_t want = d_crc ? d_crc[frame] : 0u;
    int first = -1;
    for (int k = P - 1; k >= 0; k--) first = rem[frame * (size_t)L + k] == want ? k : first;
    const size_t row = frame * (size_t)L + (size_t)(first < 0 ? 0 : first);
    const uint32_t *U = LU + row * W;
    if (d_u) d_u[frame * W + w] = U[w];
    if (d_x) d_x[frame * W + w] = LX[row * W + w];
    if (d_list_x)
        for (size_t k = 0; k < (size_t)L; k++) d_list_x[(frame * (size_t)L + k) * W + w] = LX[(frame * (size_t)L + k) * W + w];
    if (d_info && w < Wi) d_info[frame * Wi + w] = pl_info_word(U, 1, info_pos, n_info, w);
    if (w == 0) {
        if (d_pick) d_pick[frame] = first;
        if (d_metric)
            for (size_t k = 0; k < (size_t)L; k++) d_metric[frame * (size_t)L + k] = Mt[frame * (size_t)L + k];
    }
}

#endif /* QLDPC_KERNELS_POLAR_LIST_H */
