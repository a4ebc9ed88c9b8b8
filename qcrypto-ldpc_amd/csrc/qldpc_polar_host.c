/*
 * qldpc_polar_host.c -- the host mirrors of the polar encoder and SC decoder (qldpc_polar_encode_host, qldpc_polar_decode_host): plain C over the
 * functions of qldpc_polar_core.h, one frame at a time, in the order the lanes of qldpc_kernels_polar.h work: leaf block by leaf block, the levels
 * above a block in a scratch of 2N - 1 beliefs, the levels inside it by recursion, the re-encoded word of every finished node in the x row.
 */
#include <stdlib.h>
#include <string.h>

#include "../../include/qldpc.h"
#include "qldpc_graph.h"
#include "qldpc_polar_core.h"

int qldpc_polar_encode_host(int log2_n, int n_frames, const uint32_t *u, uint32_t *x)
{
    if (pl_check_size(log2_n)) { qldpc_set_error("polar_encode_host: log2_n=%d (1 .. %d)", log2_n, PL_MAX_LOG2N); return QLDPC_ESIZE; }
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

/* what a frame's decode works on */
typedef struct pl_frame {
    int n, sl, maxq;
    const uint32_t *frozen;        /* the code's frozen mask, a row */
    const uint32_t *fval;          /* the frame's frozen values, a row, or NULL */
    uint32_t *x;                   /* the re-encoded words of the finished nodes, a row */
    void *B;                       /* beliefs: level l (2^l of them) at pl_off(n, l) */
    void *leaf;                    /* the frame's leaf beliefs or NULL */
    long j;                        /* the leaf block at work */
    uint32_t uw, xw;               /* its decisions and their re-encoded word so far */
} pl_frame;

static size_t pl_off(int n, int l) { return ((size_t)2 << n) - ((size_t)2 << l); }

/* the decoder of one frame for one message type: T the belief type, TIN the input's, LOAD / F / G the core's functions with maxq at hand */
#define PL_HOST_DECODER(SUF, TIN, T, LOAD, F, G)                                                                                          \
    static void pl_block_##SUF(pl_frame *fr, int l, int pos)                                                                              \
    {                                                                                                                                     \
        const int maxq = fr->maxq;                                                                                                        \
        (void)maxq;                                                                                                                       \
        const T *src = (const T *)fr->B + pl_off(fr->n, l);                                                                               \
        if (l == 0) {                                                                                                                     \
            const long i = (fr->j << fr->sl) + pos;                                                                                       \
            const unsigned bit = pl_leaf_bit(src[0] < 0, pl_bit(fr->frozen[i >> 5], pos), fr->fval ? pl_bit(fr->fval[i >> 5], pos) : 0u); \
            if (fr->leaf) ((T *)fr->leaf)[i] = src[0];                                                                                    \
            fr->uw |= bit << (31 - pos);                                                                                                  \
            fr->xw |= bit << (31 - pos);                                                                                                  \
            return;                                                                                                                       \
        }                                                                                                                                 \
        const int h = 1 << (l - 1);                                                                                                       \
        T *dst = (T *)fr->B + pl_off(fr->n, l - 1);                                                                                       \
        for (int k = 0; k < h; k++) dst[k] = F(src[k], src[k + h]);                                                                       \
        pl_block_##SUF(fr, l - 1, pos);                                                                                                   \
        for (int k = 0; k < h; k++) dst[k] = G(src[k], src[k + h], pl_bit(fr->xw, pos + k));                                              \
        pl_block_##SUF(fr, l - 1, pos + h);                                                                                               \
        fr->xw ^= (fr->xw << h) & ((0xffffffffu << (32 - h)) >> pos);                                                                     \
    }                                                                                                                                     \
    static void pl_decode_##SUF(pl_frame *fr, const TIN *llr, uint32_t *u)                                                                \
    {                                                                                                                                     \
        const int n = fr->n, sl = fr->sl, maxq = fr->maxq;                                                                                \
        (void)maxq;                                                                                                                       \
        const long N = 1l << n, blocks = N >> sl;                                                                                         \
        T *B = (T *)fr->B;                                                                                                                \
        for (long k = 0; k < N; k++) B[k] = LOAD(llr[k]);                                                                                 \
        for (long j = 0; j < blocks; j++) {                                                                                               \
            const int top = j == 0 ? n - 1 : pl_ctz(j) + sl;                                                                              \
            for (int l = top; l >= sl; l--) {                                                                                             \
                const T *src = B + pl_off(n, l + 1);                                                                                      \
                T *dst = B + pl_off(n, l);                                                                                                \
                const long h = 1l << l, c0 = (j << sl) - h;      /* g: the node of h leaves that ends where block j begins */             \
                if (j != 0 && l == top)                                                                                                   \
                    for (long k = 0; k < h; k++) dst[k] = G(src[k], src[k + h], pl_bit(fr->x[(c0 + k) >> 5], (int)((c0 + k) & 31)));       \
                else                                                                                                                      \
                    for (long k = 0; k < h; k++) dst[k] = F(src[k], src[k + h]);                                                          \
            }                                                                                                                             \
            fr->j = j; fr->uw = 0u; fr->xw = 0u;                                                                                          \
            pl_block_##SUF(fr, sl, 0);                                                                                                    \
            u[j] = fr->uw;                                                                                                                \
            fr->x[j] = fr->xw;                                   /* = pl_enc_word(uw, sl) */                                              \
            pl_combine_words(fr->x, j, 1);                                                                                                \
        }                                                                                                                                 \
    }

#define PL_I8_LOAD(v) pl_i8_load((int)(v), maxq)
#define PL_I8_G(a, b, c) pl_i8_g((a), (b), (c), maxq)
#define PL_F32_LOAD(v) (v)
PL_HOST_DECODER(i8, int8_t, int, PL_I8_LOAD, pl_i8_f, PL_I8_G)
PL_HOST_DECODER(f32, float, float, PL_F32_LOAD, pl_f32_f, pl_f32_g)

/* the argument checks of a host decode (`who` names it in the messages) and, where they pass, the code's frozen mask: a row the caller frees */
int pl_host_decode_args(const char *who, int log2_n, int n_info, const int *info_pos, int messages, int maxq, int n_frames, const void *llr, uint32_t **frozen_mask)
{
    *frozen_mask = NULL;
    if (pl_check_size(log2_n)) { qldpc_set_error("%s: log2_n=%d (1 .. %d)", who, log2_n, PL_MAX_LOG2N); return QLDPC_ESIZE; }
    if (messages != QLDPC_POLAR_I8 && messages != QLDPC_POLAR_F32) { qldpc_set_error("%s: messages=%d (QLDPC_POLAR_I8 or QLDPC_POLAR_F32)", who, messages); return QLDPC_EINVAL; }
    if (pl_check_maxq(messages, maxq)) {
        qldpc_set_error("%s: maxq=%d (1 .. %d: f is not saturated and gives maxq + 1, which an int8 holds up to 127; use maxq <= %d)", who, maxq, PL_MAX_MAXQ, PL_MAX_MAXQ);
        return QLDPC_ESIZE;
    }
    if (n_frames < 0) { qldpc_set_error("%s: n_frames=%d is negative", who, n_frames); return QLDPC_EINVAL; }
    const long W = pl_words(log2_n);
    uint32_t *mask = (uint32_t *)calloc((size_t)W, sizeof(uint32_t));
    if (!mask) return QLDPC_ENOMEM;
    int rc = pl_mark_info(log2_n, n_info, info_pos, mask);
    if (rc) {
        if (rc == PL_EINVAL) qldpc_set_error("%s: info_pos names a position twice (positions must be distinct)", who);
        else qldpc_set_error("%s: n_info=%d positions, each in 0 .. N - 1, are required (0 <= n_info <= N)", who, n_info);
        free(mask);
        return rc;
    }
    if (n_frames > 0 && !llr) { qldpc_set_error("%s: llr is NULL", who); free(mask); return QLDPC_EINVAL; }
    const uint32_t valid = pl_row_mask(log2_n);
    for (long w = 0; w < W; w++) mask[w] = ~mask[w] & valid;      /* the frozen mask */
    *frozen_mask = mask;
    return QLDPC_OK;
}

int qldpc_polar_decode_host(int log2_n, int n_info, const int *info_pos, int messages, int maxq, int n_frames, const void *llr,
                            const uint32_t *frozen_u, uint32_t *u, uint32_t *info, uint32_t *x, void *leaf)
{
    uint32_t *mask;
    const int rc = pl_host_decode_args("polar_decode_host", log2_n, n_info, info_pos, messages, maxq, n_frames, llr, &mask);
    if (rc) return rc;
    const long N = 1l << log2_n, W = pl_words(log2_n), Wi = (n_info + 31) / 32;
    const size_t esz = messages == QLDPC_POLAR_I8 ? sizeof(int) : sizeof(float), lsz = messages == QLDPC_POLAR_I8 ? 1 : sizeof(float);
    void *B = malloc(esz * 2 * (size_t)N);
    uint32_t *rows = (uint32_t *)malloc(sizeof(uint32_t) * 2 * (size_t)W);
    if (!B || !rows) { free(B); free(rows); free(mask); return QLDPC_ENOMEM; }
    int8_t *leaf8 = NULL;
    int *leaf32 = NULL;                                             /* the I8 mirror works in ints and narrows the leaf beliefs at the end */
    if (leaf && messages == QLDPC_POLAR_I8) {
        leaf32 = (int *)malloc(sizeof(int) * (size_t)N);
        if (!leaf32) { free(B); free(rows); free(mask); return QLDPC_ENOMEM; }
        leaf8 = (int8_t *)leaf;
    }
    pl_frame fr;
    memset(&fr, 0, sizeof(fr));
    fr.n = log2_n; fr.sl = pl_sub_log(log2_n); fr.maxq = maxq; fr.frozen = mask; fr.B = B;
    for (long f = 0; f < n_frames; f++) {
        uint32_t *uf = rows, *xf = rows + W;
        fr.fval = frozen_u ? frozen_u + f * W : NULL;
        fr.x = xf;
        if (messages == QLDPC_POLAR_I8) {
            fr.leaf = leaf32;
            pl_decode_i8(&fr, (const int8_t *)llr + f * N, uf);
            if (leaf8) for (long i = 0; i < N; i++) leaf8[f * N + i] = (int8_t)leaf32[i];
        } else {
            fr.leaf = leaf ? (char *)leaf + lsz * (size_t)(f * N) : NULL;
            pl_decode_f32(&fr, (const float *)llr + f * N, uf);
        }
        if (u) memcpy(u + f * W, uf, sizeof(uint32_t) * (size_t)W);
        if (x) memcpy(x + f * W, xf, sizeof(uint32_t) * (size_t)W);
        if (info) {
            uint32_t *row = info + f * Wi;
            memset(row, 0, sizeof(uint32_t) * (size_t)Wi);
            for (int m = 0; m < n_info; m++) row[m >> 5] |= pl_bit(uf[info_pos[m] >> 5], info_pos[m]) << (31 - (m & 31));
        }
    }
    free(leaf32); free(B); free(rows); free(mask);
    return QLDPC_OK;
}
