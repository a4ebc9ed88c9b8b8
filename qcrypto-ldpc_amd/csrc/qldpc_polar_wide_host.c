/*
 * qldpc_polar_wide_host.c -- qldpc_polar_decode_wide_host: the memory plan of the wide form of the SC decoder (qldpc_polar_wide_core.h) walked on
 * the host one element at a time, in the order qldpc_kernels_polar_wide.h's workgroup works: the scratch malloc'ed at exactly
 * plw_scratch_elems(n, PLW_CHIP_LOG) beliefs of the messages' own type, a second array of exactly plw_lds_elems beliefs for the LDS, the four
 * windows at exactly plw_win_words words, the u and x rows at exactly W words.  So the CPU suite and a sanitizer see every index the kernel forms.
 * Arguments, refusals and results are qldpc_polar_decode_host's.  A frame of n <= 5 is one leaf block read from the caller's row.
 */
#include <stdlib.h>
#include <string.h>

#include "qldpc_polar_int.h"
#include "qldpc_polar_wide_core.h"

/* what a frame's walk works on: the arrays of the plan, each at its exact size */
typedef struct plw_frame {
    int n, C, maxq;
    const uint32_t *fmask;         /* the code's frozen mask, a row */
    const uint32_t *fval;          /* the frame's frozen values, a row, or NULL */
    void *S, *lds;                 /* scratch and LDS beliefs */
    uint32_t *xw, *uw, *fmw, *fvw; /* the windows */
    uint32_t *U, *X;               /* the rows */
    void *leaf;                    /* the frame's leaf beliefs or NULL */
} plw_frame;

/* the walk of one frame for one message type: T the type in memory, R the type a lane computes with, LOAD / F / G the core's functions; the leaf
   block is the core's recursion over the lane's registers */
#define PLW_HOST_WALK(SUF, T, R, LOAD, F, G)                                                                                               \
    PL_HOST_LEAF_BLOCK(SUF, T, R, LOAD, F, G)                                                                                              \
    static void plw_walk_##SUF(const plw_frame *fr, const T *in)                                                                           \
    {                                                                                                                                      \
        const int n = fr->n, C = fr->C, maxq = fr->maxq;                                                                                   \
        (void)maxq;                                                                                                                        \
        const size_t N = (size_t)1 << n, W = N >> 5, win = plw_win_words(n);                                                               \
        T *S = (T *)fr->S, *lds = (T *)fr->lds;                                                                                            \
        for (size_t j = 0; j < W; j++) {                                                                                                   \
            const size_t jw = j & (PLW_WIN - 1u);                                                                                          \
            if (jw == 0)                                                                                                                   \
                for (size_t t = 0; t < win; t++) { fr->fmw[t] = fr->fmask[j + t]; fr->fvw[t] = fr->fval ? fr->fval[j + t] : 0u; }          \
            const int top = j == 0 ? n - 1 : pl_ctz((long)j) + PL_SUB_LOG;                                                                 \
            for (int l = top; l > PL_SUB_LOG; l--) {             /* level l from level l + 1 */                                            \
                const size_t h = (size_t)1 << l, w0 = j - (h >> 5);                                                                        \
                const int is_g = j != 0 && l == top, raw = l + 1 == n;                                                                     \
                const T *src = raw ? in : (l + 1 > C ? S + plw_level_off(n, l + 1) : lds + plw_lds_off(C, l + 1));                         \
                T *dst = l > C ? S + plw_level_off(n, l) : lds + plw_lds_off(C, l);                                                        \
                for (size_t k = 0; k < h; k++) {                                                                                           \
                    const R a = raw ? LOAD(src[k]) : (R)src[k], b = raw ? LOAD(src[h + k]) : (R)src[h + k];                                \
                    if (is_g) {                                                                                                            \
                        const size_t w = w0 + (k >> 5);                                                                                    \
                        dst[k] = (T)G(a, b, pl_bit(plw_g_in_window(l) ? fr->xw[w & (PLW_WIN - 1u)] : fr->X[w], (int)(k & 31u)));           \
                    } else dst[k] = (T)F(a, b);                                                                                            \
                }                                                                                                                          \
            }                                                                                                                              \
            R L[32];                                             /* the leaf block: level 5 from level 6 */                                \
            const int is_g = j != 0 && top == PL_SUB_LOG, raw = n == PL_SUB_LOG + 1;                                                       \
            const uint32_t cw = is_g ? fr->xw[jw - 1u] : 0u;                                                                               \
            const T *src = raw ? in : lds + plw_lds_off(C, PL_SUB_LOG + 1);                                                                \
            for (int k = 0; k < 32; k++) {                                                                                                 \
                const R a = raw ? LOAD(src[k]) : (R)src[k], b = raw ? LOAD(src[32 + k]) : (R)src[32 + k];                                  \
                L[k] = is_g ? G(a, b, pl_bit(cw, k)) : F(a, b);                                                                            \
            }                                                                                                                              \
            uint32_t u = 0u, x = 0u;                                                                                                       \
            pl_node_##SUF(maxq, L, 32, 0, fr->fmw[jw], fr->fvw[jw], &u, &x, fr->leaf ? (T *)fr->leaf + j * 32u : NULL);                   \
            fr->uw[jw] = u;                                                                                                                \
            fr->xw[jw] = x;                                                                                                                \
            for (size_t h = 1; h < PLW_WIN && (j & h); h <<= 1)  /* the combines inside the window */                                      \
                for (size_t k = 0; k < h; k++) fr->xw[jw + 1u - 2u * h + k] ^= fr->xw[jw + 1u - h + k];                                    \
            if (jw == PLW_WIN - 1u || j == W - 1u) {             /* the window goes out; the combines of 64 words and more on the row */   \
                const size_t base = j - jw;                                                                                                \
                for (size_t t = 0; t < win; t++) { fr->U[base + t] = fr->uw[t]; fr->X[base + t] = fr->xw[t]; }                             \
                for (size_t h = PLW_WIN; j & h; h <<= 1)                                                                                   \
                    for (size_t k = 0; k < h; k++) fr->X[j + 1u - 2u * h + k] ^= fr->X[j + 1u - h + k];                                    \
            }                                                                                                                              \
        }                                                                                                                                  \
    }                                                                                                                                      \
    /* n <= 5: the whole frame is one leaf block of s = N leaves, read from the caller's row */                                            \
    static void plw_small_##SUF(const plw_frame *fr, const T *in)                                                                          \
    {                                                                                                                                      \
        const int s = 1 << fr->n, maxq = fr->maxq;                                                                                         \
        (void)maxq;                                                                                                                        \
        R L[32];                                                                                                                           \
        for (int k = 0; k < s; k++) L[k] = LOAD(in[k]);                                                                                    \
        uint32_t u = 0u, x = 0u;                                                                                                           \
        pl_node_##SUF(maxq, L, s, 0, fr->fmask[0], fr->fval ? fr->fval[0] : 0u, &u, &x, (T *)fr->leaf);                                    \
        fr->U[0] = u;                                                                                                                      \
        fr->X[0] = x;                                                                                                                      \
    }

PL_HOST_MESSAGES(PLW_HOST_WALK)

int qldpc_polar_decode_wide_host(int log2_n, int n_info, const int *info_pos, int messages, int maxq, int n_frames, const void *llr,
                                 const uint32_t *frozen_u, uint32_t *u, uint32_t *info, uint32_t *x, void *leaf)
{
    uint32_t *mask;
    const int rc = pl_host_decode_args("polar_decode_wide_host", log2_n, n_info, info_pos, messages, maxq, n_frames, llr, &mask);
    if (rc) return rc;
    const int n = log2_n, wide = n > PL_SUB_LOG;
    const size_t N = (size_t)1 << n, W = (size_t)pl_words(n), Wi = ((size_t)n_info + 31u) / 32u, esz = messages == QLDPC_POLAR_I8 ? 1 : sizeof(float);
    const size_t win = wide ? plw_win_words(n) : 1, s_elems = plw_scratch_elems(n, PLW_CHIP_LOG), l_elems = plw_lds_elems(n, PLW_CHIP_LOG);
    plw_frame fr;
    memset(&fr, 0, sizeof(fr));
    fr.n = n; fr.C = plw_chip(n, PLW_CHIP_LOG); fr.maxq = maxq; fr.fmask = mask;
    /* an array the plan gives no element is not allocated at all: any access to it faults */
    fr.S = s_elems ? malloc(esz * s_elems) : NULL;
    fr.lds = l_elems ? malloc(esz * l_elems) : NULL;
    uint32_t *wins = (uint32_t *)malloc(sizeof(uint32_t) * 4 * win), *rows = (uint32_t *)malloc(sizeof(uint32_t) * 2 * W);
    if ((s_elems && !fr.S) || (l_elems && !fr.lds) || !wins || !rows) { free(fr.S); free(fr.lds); free(wins); free(rows); free(mask); return QLDPC_ENOMEM; }
    fr.xw = wins; fr.uw = wins + win; fr.fmw = wins + 2 * win; fr.fvw = wins + 3 * win;
    fr.U = rows; fr.X = rows + W;
    for (size_t f = 0; f < (size_t)n_frames; f++) {
        fr.fval = frozen_u ? frozen_u + f * W : NULL;
        fr.leaf = leaf ? (char *)leaf + esz * f * N : NULL;
        if (messages == QLDPC_POLAR_I8) {
            if (wide) plw_walk_i8(&fr, (const int8_t *)llr + f * N); else plw_small_i8(&fr, (const int8_t *)llr + f * N);
        } else {
            if (wide) plw_walk_f32(&fr, (const float *)llr + f * N); else plw_small_f32(&fr, (const float *)llr + f * N);
        }
        if (u) memcpy(u + f * W, fr.U, sizeof(uint32_t) * W);
        if (x) memcpy(x + f * W, fr.X, sizeof(uint32_t) * W);
        if (info)
            for (size_t w = 0; w < Wi; w++) info[f * Wi + w] = pl_info_word(fr.U, 1, info_pos, n_info, w);
    }
    free(fr.S); free(fr.lds); free(wins); free(rows); free(mask);
    return QLDPC_OK;
}
