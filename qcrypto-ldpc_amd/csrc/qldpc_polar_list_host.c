/*
 * qldpc_polar_list_host.c -- the host mirror of the CRC-aided SC list decoder (qldpc_polar_list_decode_host) and Alice's CRC
 * (qldpc_polar_crc_host): plain C over the functions of qldpc_polar_list_core.h, one frame at a time, leaf by leaf.  The paths of a frame are held
 * as the lanes of qldpc_kernels_polar_list.h hold them -- L slots and a word of slot pointers per level, nothing copied on a fork -- so that the
 * published curve's 25 000 frames take seconds; the numpy restatement of the tests copies whole paths and agrees bit for bit.
 */
#include <stdlib.h>
#include <string.h>

#include "qldpc_polar_int.h"
#include "qldpc_polar_list_core.h"

/* what a frame's decode works on */
typedef struct pll_frame {
    int n, L, maxq;
    long N, W;
    const uint32_t *frozen;        /* the code's frozen mask, a row */
    const uint32_t *fval;          /* the frame's frozen values, a row, or NULL */
    void *in;                      /* level n: the N loaded beliefs */
    void *A;                       /* level l = 1 .. n - 1: L slots of 2^l beliefs at L (2^l - 2) */
    uint32_t *bits;                /* bit level b = 0 .. log2 W: L slots of 2^b words at pll_bit_off(L, b) */
    uint32_t ptr_a[PLL_MAX_LOG2N + 1], ptr_b[PLL_MAX_LOG2N];
    uint32_t xw[PLL_MAX_L];        /* the open leaf block of every path */
} pll_frame;

/* the in-block combines after the leaf at place p: every node that ends there, smallest first */
static uint32_t pll_close_nodes(uint32_t xw, int p)
{
    for (int h = 1; p & h; h <<= 1) xw ^= (xw << h) & ((0xffffffffu << (32 - h)) >> (p + 1 - 2 * h));
    return xw;
}

/* leaf block j is complete in xw[]: the node of 2^t blocks that ends with it goes into slot k of bit level t, built from the left nodes below */
static void pll_close_block(pll_frame *fr, long j, int P)
{
    const int t = pll_done_level(j);
    const long sz = 1l << t;
    for (int k = 0; k < P; k++) {
        uint32_t *dst = fr->bits + pll_bit_off(fr->L, t) + (size_t)k * (size_t)sz;
        dst[sz - 1] = fr->xw[k];
        for (int b = 0; b < t; b++) {
            const long s = 1l << b;
            const uint32_t *left = fr->bits + pll_bit_off(fr->L, b) + (size_t)pll_nib(fr->ptr_b[b], k) * (size_t)s;
            for (long e = 0; e < s; e++) dst[sz - 2 * s + e] = left[e] ^ dst[sz - s + e];
        }
        fr->xw[k] = 0u;
    }
    fr->ptr_b[t] = PLL_IDENT;
}

/* the decoder of one frame for one message type: T the belief type, TIN the input's; the metric's type, the penalty and the select go by the
   suffix (pll_met_, pll_*_pen, pll_select_); returns the live paths */
typedef uint32_t pll_met_i8;
typedef float pll_met_f32;
#define PLL_HOST_DECODER(SUF, TIN, T, LOAD, F, G)                                                                                         \
    static int pll_decode_##SUF(pll_frame *fr, const TIN *llr, pll_met_##SUF *metric)                                                     \
    {                                                                                                                                     \
        const int n = fr->n, L = fr->L, maxq = fr->maxq;                                                                                  \
        (void)maxq;                                                                                                                       \
        const long N = fr->N;                                                                                                             \
        T *in = (T *)fr->in, *A = (T *)fr->A, D[PLL_MAX_L];                                                                               \
        pll_met_##SUF m[PLL_MAX_L], mf[PLL_MAX_L];                                                                                        \
        uint32_t nx[PLL_MAX_L];                                                                                                           \
        int P = 1;                                                                                                                        \
        for (long k = 0; k < N; k++) in[k] = LOAD(llr[k]);                                                                                \
        for (int l = 0; l <= n; l++) fr->ptr_a[l] = PLL_IDENT;                                                                            \
        for (int b = 0; b < PLL_MAX_LOG2N; b++) fr->ptr_b[b] = PLL_IDENT;                                                                 \
        for (int k = 0; k < L; k++) { metric[k] = 0; fr->xw[k] = 0u; D[k] = 0; }                                                          \
        for (long i = 0; i < N; i++) {                                                                                                    \
            const int p = (int)(i & 31);                                                                                                  \
            const long j = i >> 5;                                                                                                        \
            const int top = i == 0 ? n - 1 : pl_ctz(i);                                                                                   \
            for (int l = top; l >= 0; l--) {                         /* level l of every path from its level l + 1 */                     \
                const long h = 1l << l;                                                                                                   \
                const int is_g = i != 0 && l == top;                                                                                      \
                for (int k = 0; k < P; k++) {                                                                                             \
                    const T *src = l + 1 == n ? in : A + (size_t)L * (size_t)(2 * h - 2) + (size_t)pll_nib(fr->ptr_a[l + 1], k) * (size_t)(2 * h); \
                    T *dst = l ? A + (size_t)L * (size_t)(h - 2) + (size_t)k * (size_t)h : &D[k];                                         \
                    if (!is_g) {                                                                                                          \
                        for (long e = 0; e < h; e++) dst[e] = F(src[e], src[e + h]);                                                      \
                    } else if (l >= PL_SUB_LOG) {                    /* the left sibling: a node of h / 32 blocks */                      \
                        const uint32_t *cw = fr->bits + pll_bit_off(L, l - PL_SUB_LOG) + (size_t)pll_nib(fr->ptr_b[l - PL_SUB_LOG], k) * (size_t)(h >> 5); \
                        for (long e = 0; e < h; e++) dst[e] = G(src[e], src[e + h], pl_bit(cw[e >> 5], (int)(e & 31)));                   \
                    } else {                                         /* the left sibling: the h places before p of the open block */     \
                        for (long e = 0; e < h; e++) dst[e] = G(src[e], src[e + h], pl_bit(fr->xw[k], p - (int)h + (int)e));              \
                    }                                                                                                                     \
                }                                                                                                                         \
                if (l) fr->ptr_a[l] = PLL_IDENT;                                                                                          \
            }                                                                                                                             \
            if (pl_bit(fr->frozen[j], p)) {                                                                                               \
                const unsigned bit = fr->fval ? pl_bit(fr->fval[j], p) : 0u;                                                              \
                for (int k = 0; k < P; k++) {                                                                                             \
                    if ((unsigned)(D[k] < 0) != bit) metric[k] += pll_##SUF##_pen(D[k]);                                                  \
                    fr->xw[k] |= bit << (31 - p);                                                                                         \
                }                                                                                                                         \
            } else {                                                                                                                      \
                const int n_new = 2 * P < L ? 2 * P : L;                                                                                  \
                for (int k = 0; k < P; k++) { m[k] = metric[k]; mf[k] = metric[k] + pll_##SUF##_pen(D[k]); }                              \
                const uint32_t sel = pll_select_##SUF(PLL_MAX_L, P, n_new, m, mf);                                                        \
                uint32_t par = 0u;                                                                                                        \
                for (int r = 0; r < n_new; r++) {                                                                                         \
                    const unsigned c = pll_nib(sel, r) & 7u, flip = pll_nib(sel, r) >> 3;                                                 \
                    metric[r] = flip ? mf[c] : m[c];                                                                                      \
                    nx[r] = fr->xw[c] | (((unsigned)(D[c] < 0) ^ flip) << (31 - p));                                                      \
                    par |= (uint32_t)c << (4 * r);                                                                                        \
                }                                                                                                                         \
                for (int r = 0; r < n_new; r++) fr->xw[r] = nx[r];                                                                        \
                for (int l = 1; l < n; l++) fr->ptr_a[l] = pll_perm(fr->ptr_a[l], par, PLL_MAX_L);                                        \
                for (int b = 0; b < PLL_MAX_LOG2N; b++) fr->ptr_b[b] = pll_perm(fr->ptr_b[b], par, PLL_MAX_L);                            \
                P = n_new;                                                                                                                \
            }                                                                                                                             \
            for (int k = 0; k < P; k++) fr->xw[k] = pll_close_nodes(fr->xw[k], p);                                                        \
            if (p == 31 || i == N - 1) pll_close_block(fr, j, P);                                                                         \
        }                                                                                                                                 \
        return P;                                                                                                                         \
    }

PL_HOST_MESSAGES(PLL_HOST_DECODER)

static int pll_crc_args(const char *who, int crc_len, uint32_t crc_poly, int n_info)
{
    const int rc = pll_check_crc(crc_len, crc_poly, n_info);
    if (rc)
        qldpc_set_error("%s: crc_len=%d, crc_poly=0x%x, n_info=%d (crc_len 0 .. 32 and at most n_info; crc_poly holds the low crc_len coefficients, x^crc_len is implied)",
                        who, crc_len, (unsigned)crc_poly, n_info);
    return rc;
}

int qldpc_polar_crc_host(int crc_len, uint32_t crc_poly, int n_bits, int n_frames, const uint32_t *rows, uint32_t *crc)
{
    if (pll_crc_args("polar_crc_host", crc_len, crc_poly, -1)) return QLDPC_ESIZE;
    if (n_bits < 0 || n_frames < 0) { qldpc_set_error("polar_crc_host: n_bits=%d, n_frames=%d: negative", n_bits, n_frames); return QLDPC_EINVAL; }
    if (n_frames > 0 && (!crc || (n_bits > 0 && !rows))) { qldpc_set_error("polar_crc_host: NULL row pointer"); return QLDPC_EINVAL; }
    const long Wb = ((long)n_bits + 31) / 32;
    for (long f = 0; f < n_frames; f++) {
        uint32_t r = 0u;
        for (long m = 0; m < n_bits; m++) r = pll_crc_step(r, pl_bit(rows[f * Wb + (m >> 5)], (int)(m & 31)), crc_len, crc_poly);
        crc[f] = r;
    }
    return QLDPC_OK;
}

int qldpc_polar_list_decode_host(int log2_n, int n_info, const int *info_pos, int messages, int maxq, int list_size, int crc_len, uint32_t crc_poly,
                                 int n_frames, const void *llr, const uint32_t *frozen_u, const uint32_t *crc, uint32_t *u, uint32_t *info,
                                 uint32_t *x, int32_t *pick, void *metric, uint32_t *list_x)
{
    const char *who = "polar_list_decode_host";
    uint32_t *mask;
    int rc = pl_args_scalars(who, log2_n, PLL_MAX_LOG2N, messages, maxq);
    if (rc) return rc;
    if (pll_check_list(list_size)) { qldpc_set_error("%s: list_size=%d (1, 2, 4 or 8)", who, list_size); return QLDPC_ESIZE; }
    if (n_frames < 0) { qldpc_set_error("%s: n_frames=%d is negative", who, n_frames); return QLDPC_EINVAL; }
    rc = pl_args_frozen_mask(who, log2_n, n_info, info_pos, &mask);
    if (rc) return rc;
    if (pll_crc_args(who, crc_len, crc_poly, n_info)) { free(mask); return QLDPC_ESIZE; }
    if (crc && crc_len == 0) { qldpc_set_error("%s: a crc row with crc_len = 0", who); free(mask); return QLDPC_EINVAL; }
    if (n_frames > 0 && !llr) { qldpc_set_error("%s: llr is NULL", who); free(mask); return QLDPC_EINVAL; }
    const long N = 1l << log2_n, W = pl_words(log2_n), Wi = ((long)n_info + 31) / 32;
    const int L = list_size;
    const size_t esz = messages == QLDPC_POLAR_I8 ? sizeof(int) : sizeof(float);
    pll_frame fr;
    memset(&fr, 0, sizeof(fr));
    fr.n = log2_n; fr.L = L; fr.maxq = maxq; fr.N = N; fr.W = W; fr.frozen = mask;
    fr.in = malloc(esz * (size_t)N);
    fr.A = malloc(esz * (size_t)L * (size_t)N);
    fr.bits = (uint32_t *)malloc(sizeof(uint32_t) * pll_bit_words(L, log2_n));
    uint32_t *uk = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)L * (size_t)W);
    if (!fr.in || !fr.A || !fr.bits || !uk) { free(fr.in); free(fr.A); free(fr.bits); free(uk); free(mask); return QLDPC_ENOMEM; }
    const uint32_t *roots = fr.bits + pll_bit_off(L, pll_done_level(W - 1));
    for (long f = 0; f < n_frames; f++) {
        uint32_t mi[PLL_MAX_L];
        float mf[PLL_MAX_L];
        int P;
        fr.fval = frozen_u ? frozen_u + f * W : NULL;
        if (messages == QLDPC_POLAR_I8) P = pll_decode_i8(&fr, (const int8_t *)llr + f * N, mi);
        else P = pll_decode_f32(&fr, (const float *)llr + f * N, mf);
        /* u = encode(x) of every live path; the first whose CRC is the expected one */
        const uint32_t want = crc ? crc[f] : 0u;
        int first = -1;
        for (int k = 0; k < P; k++) {
            qldpc_polar_encode_host(log2_n, 1, roots + (size_t)k * (size_t)W, uk + (size_t)k * (size_t)W);
            uint32_t r = 0u;
            for (int m = 0; m < n_info; m++) r = pll_crc_step(r, pl_bit(uk[(size_t)k * (size_t)W + (size_t)(info_pos[m] >> 5)], info_pos[m]), crc_len, crc_poly);
            if (first < 0 && r == want) first = k;
        }
        const uint32_t *us = uk + (size_t)(first < 0 ? 0 : first) * (size_t)W, *xs = roots + (size_t)(first < 0 ? 0 : first) * (size_t)W;
        if (pick) pick[f] = first;
        if (u) memcpy(u + f * W, us, sizeof(uint32_t) * (size_t)W);
        if (x) memcpy(x + f * W, xs, sizeof(uint32_t) * (size_t)W);
        if (info)
            for (long w = 0; w < Wi; w++) info[f * Wi + w] = pl_info_word(us, 1, info_pos, n_info, (size_t)w);
        if (metric) {
            for (int k = 0; k < L; k++) {
                if (messages == QLDPC_POLAR_I8) ((uint32_t *)metric)[f * L + k] = k < P ? mi[k] : 0xffffffffu;
                else ((float *)metric)[f * L + k] = k < P ? mf[k] : __builtin_inff();
            }
        }
        if (list_x) {
            uint32_t *rows = list_x + (size_t)f * (size_t)L * (size_t)W;
            memset(rows, 0, sizeof(uint32_t) * (size_t)L * (size_t)W);
            memcpy(rows, roots, sizeof(uint32_t) * (size_t)P * (size_t)W);
        }
    }
    free(fr.in); free(fr.A); free(fr.bits); free(uk); free(mask);
    return QLDPC_OK;
}
