/*
 * qldpc_polar_host.c -- the host mirrors of the polar encoder and SC decoder (qldpc_polar_encode_host, qldpc_polar_decode_host, and
 * qldpc_polar_decode_rows_host with a frozen set per frame): plain C over the
 * functions of qldpc_polar_core.h, one frame at a time, in the order the lanes of qldpc_kernels_polar.h work: leaf block by leaf block, the levels
 * above a block in a scratch of 2N - 1 beliefs, the levels inside it by the core's recursion, the re-encoded word of every finished node in the x
 * row.  And the argument checks of a code (qldpc_polar_int.h), which every unit of the subsystem calls.
 */
#include <stdlib.h>
#include <string.h>

#include "qldpc_polar_int.h"

int pl_args_scalars(const char *who, int log2_n, int max_log2_n, int messages, int maxq)
{
    if (pl_check_size(log2_n, max_log2_n)) { qldpc_set_error("%s: log2_n=%d (1 .. %d)", who, log2_n, max_log2_n); return QLDPC_ESIZE; }
    if (messages != QLDPC_POLAR_I8 && messages != QLDPC_POLAR_F32) { qldpc_set_error("%s: messages=%d (QLDPC_POLAR_I8 or QLDPC_POLAR_F32)", who, messages); return QLDPC_EINVAL; }
    if (pl_check_maxq(messages, maxq)) {
        qldpc_set_error("%s: maxq=%d (1 .. %d: f is not saturated and gives maxq + 1, which an int8 holds up to 127; use maxq <= %d)", who, maxq, PL_MAX_MAXQ, PL_MAX_MAXQ);
        return QLDPC_ESIZE;
    }
    return QLDPC_OK;
}

int pl_args_frozen_mask(const char *who, int log2_n, int n_info, const int *info_pos, uint32_t **frozen_mask)
{
    *frozen_mask = NULL;
    const long W = pl_words(log2_n);
    uint32_t *mask = (uint32_t *)calloc((size_t)W, sizeof(uint32_t));
    if (!mask) return QLDPC_ENOMEM;
    const int rc = pl_mark_info(log2_n, n_info, info_pos, mask);
    if (rc) {
        if (rc == PL_EINVAL) qldpc_set_error("%s: info_pos names a position twice (positions must be distinct)", who);
        else qldpc_set_error("%s: n_info=%d positions, each in 0 .. N - 1, are required (0 <= n_info <= N = %ld)", who, n_info, 1l << log2_n);
        free(mask);
        return rc;
    }
    const uint32_t valid = pl_row_mask(log2_n);
    for (long w = 0; w < W; w++) mask[w] = ~mask[w] & valid;
    *frozen_mask = mask;
    return QLDPC_OK;
}

int pl_host_decode_args(const char *who, int log2_n, int n_info, const int *info_pos, int messages, int maxq, int n_frames, const void *llr, uint32_t **frozen_mask)
{
    *frozen_mask = NULL;
    int rc = pl_args_scalars(who, log2_n, PL_MAX_LOG2N, messages, maxq);
    if (rc) return rc;
    if (n_frames < 0) { qldpc_set_error("%s: n_frames=%d is negative", who, n_frames); return QLDPC_EINVAL; }
    rc = pl_args_frozen_mask(who, log2_n, n_info, info_pos, frozen_mask);
    if (rc) return rc;
    if (n_frames > 0 && !llr) { qldpc_set_error("%s: llr is NULL", who); free(*frozen_mask); *frozen_mask = NULL; return QLDPC_EINVAL; }
    return QLDPC_OK;
}

int qldpc_polar_encode_host(int log2_n, int n_frames, const uint32_t *u, uint32_t *x)
{
    if (pl_check_size(log2_n, PL_MAX_LOG2N)) { qldpc_set_error("polar_encode_host: log2_n=%d (1 .. %d)", log2_n, PL_MAX_LOG2N); return QLDPC_ESIZE; }
    if (n_frames < 0) { qldpc_set_error("polar_encode_host: n_frames=%d is negative", n_frames); return QLDPC_EINVAL; }
    if (n_frames > 0 && (!u || !x)) { qldpc_set_error("polar_encode_host: NULL row pointer"); return QLDPC_EINVAL; }
    const long W = pl_words(log2_n);
    const int sl = pl_sub_log(log2_n);
    const uint32_t valid = pl_row_mask(log2_n);
    for (long f = 0; f < n_frames; f++) {
        const uint32_t *src = u + f * W;
        uint32_t *dst = x + f * W;
        for (long j = 0; j < W; j++) {
            dst[j] = pl_enc_word(src[j] & valid, sl);
            pl_combine_words(dst, j, 1);
        }
    }
    return QLDPC_OK;
}

static size_t pl_off(int n, int l) { return ((size_t)2 << n) - ((size_t)2 << l); }

/* the decoder of one frame for one message type: B the scratch, level l (2^l beliefs) at pl_off(n, l); frozen, fval (or NULL), u, x: rows of the
   frame; leaf: its leaf beliefs or NULL */
#define PL_HOST_DECODER(SUF, TIN, T, LOAD, F, G)                                                                                          \
    PL_HOST_LEAF_BLOCK(SUF, TIN, T, LOAD, F, G)                                                                                           \
    static void pl_decode_##SUF(int n, int maxq, const TIN *llr, const uint32_t *frozen, const uint32_t *fval, T *B, uint32_t *u,         \
                                uint32_t *x, TIN *leaf)                                                                                   \
    {                                                                                                                                     \
        const int sl = pl_sub_log(n);                                                                                                     \
        (void)maxq;                                                                                                                       \
        const long N = 1l << n, blocks = N >> sl;                                                                                         \
        for (long k = 0; k < N; k++) B[k] = LOAD(llr[k]);                                                                                 \
        for (long j = 0; j < blocks; j++) {                                                                                               \
            const int top = j == 0 ? n - 1 : pl_ctz(j) + sl;                                                                              \
            for (int l = top; l >= sl; l--) {                                                                                             \
                const T *src = B + pl_off(n, l + 1);                                                                                      \
                T *dst = B + pl_off(n, l);                                                                                                \
                const long h = 1l << l, c0 = (j << sl) - h;      /* g: the node of h leaves that ends where block j begins */             \
                if (j != 0 && l == top)                                                                                                   \
                    for (long k = 0; k < h; k++) dst[k] = G(src[k], src[k + h], pl_bit(x[(c0 + k) >> 5], (int)((c0 + k) & 31)));           \
                else                                                                                                                      \
                    for (long k = 0; k < h; k++) dst[k] = F(src[k], src[k + h]);                                                          \
            }                                                                                                                             \
            u[j] = 0u; x[j] = 0u;                                                                                                         \
            pl_node_##SUF(maxq, B + pl_off(n, sl), 1 << sl, 0, frozen[j], fval ? fval[j] : 0u, &u[j], &x[j], leaf ? leaf + (j << sl) : NULL); \
            pl_combine_words(x, j, 1);                           /* x[j] = pl_enc_word(u[j], sl) before it */                              \
        }                                                                                                                                 \
    }
PL_HOST_MESSAGES(PL_HOST_DECODER)

/* the two SC mirrors: with_rows = 0 is the code's frozen set for every frame, otherwise frozen_rows is [n_frames][W], each frame's additions to it */
static int pl_decode_frames(const char *who, int with_rows, int log2_n, int n_info, const int *info_pos, int messages, int maxq, int n_frames, const void *llr,
                            const uint32_t *frozen_u, const uint32_t *frozen_rows, uint32_t *u, uint32_t *info, uint32_t *x, void *leaf)
{
    uint32_t *mask;
    const int rc = pl_host_decode_args(who, log2_n, n_info, info_pos, messages, maxq, n_frames, llr, &mask);
    if (rc) return rc;
    if (with_rows && n_frames > 0 && !frozen_rows) { qldpc_set_error("%s: frozen_rows is NULL", who); free(mask); return QLDPC_EINVAL; }
    const long N = 1l << log2_n, W = pl_words(log2_n), Wi = (n_info + 31) / 32;
    void *B = malloc((messages == QLDPC_POLAR_I8 ? sizeof(int) : sizeof(float)) * 2 * (size_t)N);
    uint32_t *rows = (uint32_t *)malloc(sizeof(uint32_t) * 3 * (size_t)W);
    if (!B || !rows) { free(B); free(rows); free(mask); return QLDPC_ENOMEM; }
    uint32_t *uf = rows, *xf = rows + W, *ff = rows + 2 * W;
    for (long f = 0; f < n_frames; f++) {
        const uint32_t *fval = frozen_u ? frozen_u + f * W : NULL, *fz = mask;
        if (with_rows) {
            for (long w = 0; w < W; w++) ff[w] = pl_rows_frozen(mask[w], frozen_rows[f * W + w]);
            fz = ff;
        }
        if (messages == QLDPC_POLAR_I8) pl_decode_i8(log2_n, maxq, (const int8_t *)llr + f * N, fz, fval, (int *)B, uf, xf, leaf ? (int8_t *)leaf + f * N : NULL);
        else pl_decode_f32(log2_n, maxq, (const float *)llr + f * N, fz, fval, (float *)B, uf, xf, leaf ? (float *)leaf + f * N : NULL);
        if (u) memcpy(u + f * W, uf, sizeof(uint32_t) * (size_t)W);
        if (x) memcpy(x + f * W, xf, sizeof(uint32_t) * (size_t)W);
        if (info)
            for (long w = 0; w < Wi; w++) info[f * Wi + w] = pl_info_word(uf, 1, info_pos, n_info, (size_t)w);
    }
    free(B); free(rows); free(mask);
    return QLDPC_OK;
}

int qldpc_polar_decode_host(int log2_n, int n_info, const int *info_pos, int messages, int maxq, int n_frames, const void *llr,
                            const uint32_t *frozen_u, uint32_t *u, uint32_t *info, uint32_t *x, void *leaf)
{
    return pl_decode_frames("polar_decode_host", 0, log2_n, n_info, info_pos, messages, maxq, n_frames, llr, frozen_u, NULL, u, info, x, leaf);
}

int qldpc_polar_decode_rows_host(int log2_n, int n_info, const int *info_pos, int messages, int maxq, int n_frames, const void *llr,
                                 const uint32_t *frozen_u, const uint32_t *frozen_rows, uint32_t *u, uint32_t *info, uint32_t *x, void *leaf)
{
    return pl_decode_frames("polar_decode_rows_host", 1, log2_n, n_info, info_pos, messages, maxq, n_frames, llr, frozen_u, frozen_rows, u, info, x, leaf);
}
