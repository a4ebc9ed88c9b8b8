/*
 * qldpc_polar_ssc_host.c -- the host mirror of the simplified SC decoder (qldpc_polar_decode_ssc_host) and the plan of a code
 * (qldpc_polar_ssc_plan_host): plain C over the functions of qldpc_polar_ssc_core.h, one frame at a time, in the order the lanes of
 * qldpc_kernels_polar_ssc.h work: step by step of the plan, the levels above a step's node in a scratch of 2N - 1 beliefs, a mixed leaf block by
 * the core's recursion, the returned word of every finished node in the x row.
 */
#include <stdlib.h>
#include <string.h>

#include "qldpc_polar_int.h"
#include "qldpc_polar_ssc_core.h"

static size_t pls_off(int n, int l) { return ((size_t)2 << n) - ((size_t)2 << l); }

/* the decoder of one frame for one message type: B the scratch, level l (2^l beliefs) at pls_off(n, l); frozen, fval (or NULL), u, x: rows of
   the frame; steps: the code's plan */
#define PL_SSC_HOST_DECODER(SUF, TIN, T, LOAD, F, G)                                                                                      \
    PL_SSC_HOST_LEAF_BLOCK(SUF, TIN, T, LOAD, F, G)                                                                                       \
    static void pl_ssc_decode_##SUF(int n, int maxq, const TIN *llr, const uint32_t *frozen, const uint32_t *fval, const int *steps,      \
                                    long n_steps, T *B, uint32_t *u, uint32_t *x)                                                         \
    {                                                                                                                                     \
        const long N = 1l << n, W = pl_words(n);                                                                                          \
        (void)maxq;                                                                                                                       \
        for (long k = 0; k < N; k++) B[k] = LOAD(llr[k]);                                                                                 \
        if (n <= PL_SUB_LOG) {                                   /* the frame is one leaf block */                                        \
            u[0] = 0u; x[0] = 0u;                                                                                                         \
            pl_ssc_node_##SUF(maxq, B, n, 0, frozen[0], fval ? fval[0] : 0u, &u[0], &x[0]);                                               \
            return;                                                                                                                       \
        }                                                                                                                                 \
        for (long i = 0; i < n_steps; i++) {                                                                                              \
            const long j = steps[i * PL_SSC_STEP], cnt = 1l << (steps[i * PL_SSC_STEP + 1] - PL_SUB_LOG);                                 \
            const int lam = steps[i * PL_SSC_STEP + 1], kind = steps[i * PL_SSC_STEP + 2];                                                \
            const int top = j == 0 ? n - 1 : pl_ctz(j) + PL_SUB_LOG;                                                                      \
            for (int l = top; l >= (kind == PL_SSC_RATE0 ? lam + 1 : lam); l--) {                                                         \
                const T *src = B + pls_off(n, l + 1);                                                                                     \
                T *dst = B + pls_off(n, l);                                                                                               \
                const long h = 1l << l, c0 = (j << PL_SUB_LOG) - h;      /* g: the node of h leaves that ends where the step begins */    \
                if (j != 0 && l == top)                                                                                                   \
                    for (long k = 0; k < h; k++) dst[k] = G(src[k], src[k + h], pl_bit(x[(c0 + k) >> 5], (int)((c0 + k) & 31)));           \
                else                                                                                                                      \
                    for (long k = 0; k < h; k++) dst[k] = F(src[k], src[k + h]);                                                          \
            }                                                                                                                             \
            if (kind == PL_SSC_RATE0) {                                                                                                   \
                for (long k = 0; k < cnt; k++) {                                                                                          \
                    u[j + k] = fval ? fval[j + k] : 0u;                                                                                   \
                    x[j + k] = pl_enc_word(u[j + k], PL_SUB_LOG);                                                                         \
                    pl_ssc_combine(x, j + k, 1, 1, cnt);                                                                                  \
                }                                                                                                                         \
            } else if (kind == PL_SSC_RATE1) {                                                                                            \
                const T *L = B + pls_off(n, lam);                                                                                         \
                for (long k = 0; k < cnt; k++) {                                                                                          \
                    uint32_t c = 0u;                                                                                                      \
                    for (int b = 0; b < 32; b++) c |= (uint32_t)(L[32 * k + b] < 0) << (31 - b);                                          \
                    x[j + k] = c;                                                                                                         \
                    u[j + k] = pl_enc_word(c, PL_SUB_LOG);                                                                                \
                    pl_ssc_combine(u, j + k, 1, 1, cnt);                                                                                  \
                }                                                                                                                         \
            } else {                                                                                                                      \
                u[j] = 0u; x[j] = 0u;                                                                                                     \
                pl_ssc_node_##SUF(maxq, B + pls_off(n, PL_SUB_LOG), PL_SUB_LOG, 0, frozen[j], fval ? fval[j] : 0u, &u[j], &x[j]);         \
            }                                                                                                                             \
            pl_ssc_combine(x, j + cnt - 1, 1, cnt, W);                                                                                    \
        }                                                                                                                                 \
    }
PL_HOST_MESSAGES(PL_SSC_HOST_DECODER)

int qldpc_polar_ssc_plan_host(int log2_n, int n_info, const int *info_pos, int *steps, int *n_steps)
{
    uint32_t *mask;
    if (pl_check_size(log2_n, PL_MAX_LOG2N)) { qldpc_set_error("polar_ssc_plan_host: log2_n=%d (1 .. %d)", log2_n, PL_MAX_LOG2N); return QLDPC_ESIZE; }
    const int rc = pl_args_frozen_mask("polar_ssc_plan_host", log2_n, n_info, info_pos, &mask);
    if (rc) return rc;
    if (!steps || !n_steps) { qldpc_set_error("polar_ssc_plan_host: steps and n_steps are required"); free(mask); return QLDPC_EINVAL; }
    *n_steps = (int)pl_ssc_plan(log2_n, mask, steps);
    free(mask);
    return QLDPC_OK;
}

int qldpc_polar_decode_ssc_host(int log2_n, int n_info, const int *info_pos, int messages, int maxq, int n_frames, const void *llr,
                                const uint32_t *frozen_u, uint32_t *u, uint32_t *info, uint32_t *x)
{
    uint32_t *mask;
    const int rc = pl_host_decode_args("polar_decode_ssc_host", log2_n, n_info, info_pos, messages, maxq, n_frames, llr, &mask);
    if (rc) return rc;
    const long N = 1l << log2_n, W = pl_words(log2_n), Wi = (n_info + 31) / 32;
    void *B = malloc((messages == QLDPC_POLAR_I8 ? sizeof(int) : sizeof(float)) * 2 * (size_t)N);
    uint32_t *rows = (uint32_t *)malloc(sizeof(uint32_t) * 2 * (size_t)W);
    int *steps = (int *)malloc(sizeof(int) * PL_SSC_STEP * (size_t)pl_ssc_max_steps(log2_n));
    if (!B || !rows || !steps) { free(B); free(rows); free(steps); free(mask); return QLDPC_ENOMEM; }
    const long n_steps = pl_ssc_plan(log2_n, mask, steps);
    uint32_t *uf = rows, *xf = rows + W;
    for (long f = 0; f < n_frames; f++) {
        const uint32_t *fval = frozen_u ? frozen_u + f * W : NULL;
        if (messages == QLDPC_POLAR_I8) pl_ssc_decode_i8(log2_n, maxq, (const int8_t *)llr + f * N, mask, fval, steps, n_steps, (int *)B, uf, xf);
        else pl_ssc_decode_f32(log2_n, maxq, (const float *)llr + f * N, mask, fval, steps, n_steps, (float *)B, uf, xf);
        if (u) memcpy(u + f * W, uf, sizeof(uint32_t) * (size_t)W);
        if (x) memcpy(x + f * W, xf, sizeof(uint32_t) * (size_t)W);
        if (info)
            for (long w = 0; w < Wi; w++) info[f * Wi + w] = pl_info_word(uf, 1, info_pos, n_info, (size_t)w);
    }
    free(B); free(rows); free(steps); free(mask);
    return QLDPC_OK;
}
