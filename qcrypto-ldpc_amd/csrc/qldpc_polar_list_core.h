/*
 * qldpc_polar_list_core.h -- the definition of the CRC-aided successive-cancellation LIST decoder of qldpc_polar_list_*.  Plain C on top of
 * qldpc_polar_core.h (f, g, sat, the clamp on load, the packing), shared by the kernels (qldpc_kernels_polar_list.h) and by the host mirror
 * (qldpc_polar_list_host.c).
 *
 *   paths      a list holds up to L paths, L in {1, 2, 4, 8}; a path has a metric >= 0: an exact uint32 with QLDPC_POLAR_I8 (N (maxq + 1) fits),
 *              a float with QLDPC_POLAR_F32.  Start: one live path, metric 0.
 *   order      leaves in natural order; every live path computes its leaf belief D as the SC decoder does (g with the re-encoded bits of the
 *              path's own left sibling).
 *   frozen     bit = the frame's frozen value (0 without a row); metric += |D| if (D < 0) != bit.  Nothing is reordered.
 *   info       P live paths give 2P candidates: KEEP c = path c with bit (D_c < 0) and metric m_c, FLIP c = path c with the other bit and metric
 *              m_c + |D_c| (one float add).  Candidate index: c for KEEP c, P + c for FLIP c.  The new list is the min(L, 2P) smallest in the order
 *              (metric, candidate index), new path k the k-th of them: pll_select_*.  The list is sorted at an information leaf and only there.
 *   CRC        crc_len 0 .. 32, crc_poly = the low crc_len coefficients (x^crc_len implied); register form, zero start, MSB first, no reflection,
 *              no final XOR (pll_crc_step), over a path's n_info information bits in the caller's order (bit m = u[info_pos[m]]).
 *   pick       the first path in list order whose remainder is the frame's expected value (crc[frame], 0 without a row); none: path 0, pick = -1.
 *              crc_len = 0: every path matches, pick = 0.  L = 1 with crc_len = 0 is the SC decoder bit for bit.
 *
 * Both sides hold the paths without copying them on a fork (the traversal and the number of live paths are the same for every frame): every belief
 * level l < n and every bit level (a finished left node of 2^b leaf blocks) has L slots and, per path, a slot pointer, one nibble of a word per
 * level (PLL_IDENT: path k -> slot k).  A step that writes a level writes path k's result into slot k and resets the level's word; reads go through
 * the pointer; a fork permutes the words (pll_perm).  A level is read only while a lower level is written, so no step reads what it writes.
 */
#ifndef QLDPC_POLAR_LIST_CORE_H
#define QLDPC_POLAR_LIST_CORE_H

#include <stddef.h>

#include "qldpc_polar_core.h"

#if defined(__HIPCC__)
#define PLL_FN __host__ __device__ static inline __attribute__((always_inline))
#define PLL_UNROLL _Pragma("unroll")
#else
#define PLL_FN static inline
#define PLL_UNROLL
#endif

#define PLL_MAX_L 8
#define PLL_MAX_LOG2N 16           /* the scratch grows with L N */
#define PLL_IDENT 0x76543210u      /* a level's slot pointers after it has been written: path k reads slot k */
#define PLL_FLIP 8u                /* pll_select_*: a nibble is parent | PLL_FLIP for a FLIP candidate */

PLL_FN unsigned pll_nib(uint32_t w, int k) { return (w >> (4 * k)) & 15u; }
/* a level's pointers after a fork: new path r has what its parent (nibble r of `par`) had */
PLL_FN uint32_t pll_perm(uint32_t w, uint32_t par, int L)
{
    uint32_t out = 0u;
    PLL_UNROLL
    for (int r = 0; r < L; r++) out |= pll_nib(w, (int)pll_nib(par, r)) << (4 * r);
    return out;
}

/* what a decision against the belief costs */
PLL_FN uint32_t pll_i8_pen(int D) { return (uint32_t)(D < 0 ? -D : D); }
PLL_FN float pll_f32_pen(float D) { return __builtin_fabsf(D); }

/* The survivors of an information leaf: m[c] the metric of KEEP c, mf[c] of FLIP c, c < P <= LMAX; returns a word whose nibble k < n_new names new
 * path k: parent | PLL_FLIP.  A rank over the 2P keys (metric, candidate index), every FLIP index above every KEEP index; LMAX is a constant at
 * the call, so that the loops unroll and the arrays stay registers. */
#define PLL_DEFINE_SELECT(NAME, MT)                                                                                   \
    PLL_FN uint32_t NAME(const int LMAX, int P, int n_new, const MT *m, const MT *mf)                                 \
    {                                                                                                                 \
        uint32_t sel = 0u;                                                                                            \
        PLL_UNROLL                                                                                                    \
        for (int c = 0; c < LMAX; c++) {                                                                              \
            if (c >= P) continue;                                                                                     \
            unsigned rk = 0u, rf = 0u;                                                                                \
            PLL_UNROLL                                                                                                \
            for (int b = 0; b < LMAX; b++) {                                                                          \
                if (b >= P) continue;                                                                                 \
                rk += (unsigned)((m[b] < m[c]) | ((m[b] == m[c]) & (b < c))) + (unsigned)(mf[b] < m[c]);              \
                rf += (unsigned)(m[b] <= mf[c]) + (unsigned)((mf[b] < mf[c]) | ((mf[b] == mf[c]) & (b < c)));         \
            }                                                                                                         \
            sel |= rk < (unsigned)n_new ? (uint32_t)c << (4u * (rk & 7u)) : 0u;                                       \
            sel |= rf < (unsigned)n_new ? ((uint32_t)c | PLL_FLIP) << (4u * (rf & 7u)) : 0u;                          \
        }                                                                                                             \
        return sel;                                                                                                   \
    }
PLL_DEFINE_SELECT(pll_select_i8, uint32_t)
PLL_DEFINE_SELECT(pll_select_f32, float)

/* ---- the CRC ---- */
PLL_FN uint32_t pll_crc_mask(int crc_len) { return crc_len >= 32 ? 0xffffffffu : (1u << crc_len) - 1u; }
PLL_FN uint32_t pll_crc_step(uint32_t r, unsigned bit, int crc_len, uint32_t crc_poly)
{
    if (crc_len == 0) return 0u;
    const unsigned top = ((r >> (crc_len - 1)) & 1u) ^ bit;
    r = (r << 1) & pll_crc_mask(crc_len);
    return top ? r ^ crc_poly : r;
}

/* ---- where a frame's levels lie, per path slot; the host counts elements and words, a wave quads (x 64 lanes) ---- */
/* the block of a frame that ends with leaf block j finishes a node of 2^t blocks, t = the trailing ones of j (log2 W for the last block) */
PLL_FN int pll_done_level(long j) { return pl_ctz(j + 1); }
/* words before bit level b (2^b words a slot, L slots), and of all levels b <= log2 W */
PLL_FN size_t pll_bit_off(int L, int b) { return (size_t)L * (((size_t)1 << b) - 1u); }
PLL_FN size_t pll_bit_words(int L, int log2_n) { return (size_t)L * (2u * (size_t)pl_words(log2_n) - 1u); }

/* ---- argument checks on top of the SC decoder's (the size against PLL_MAX_LOG2N), before the first HIP call; 0 or a qldpc_status value ---- */
PLL_FN int pll_check_list(int list_size) { return list_size == 1 || list_size == 2 || list_size == 4 || list_size == 8 ? 0 : PL_ESIZE; }
/* n_info < 0: a CRC without a code (qldpc_polar_crc_host) */
PLL_FN int pll_check_crc(int crc_len, uint32_t crc_poly, int n_info)
{
    if (crc_len < 0 || crc_len > 32) return PL_ESIZE;
    if (n_info >= 0 && crc_len > n_info) return PL_ESIZE;
    if (crc_poly & ~pll_crc_mask(crc_len)) return PL_ESIZE;
    return 0;
}
/* live paths after all leaves */
PLL_FN int pll_final_paths(int list_size, int n_info)
{
    int P = 1;
    for (int m = 0; m < n_info && P < list_size; m++) P *= 2;
    return P;
}

#endif /* QLDPC_POLAR_LIST_CORE_H */
