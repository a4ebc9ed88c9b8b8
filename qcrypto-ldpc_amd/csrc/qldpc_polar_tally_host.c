/*
 * qldpc_polar_tally_host.c -- the host side of the genie-aided code construction, plain C on the rule of qldpc_polar_tally_core.h:
 * qldpc_polar_tally_host, the mirror of qldpc_polar_tally_dev (the genie decode is qldpc_polar_decode_host of a code with no information
 * position, its frozen row the true row, PLT_CHUNK frames at a time so that no [frames][N] array of leaf beliefs exists), and the two helpers
 * that turn a tally into a code: qldpc_polar_construct_order_host and qldpc_polar_construct_k_host.
 */
#include <stdlib.h>
#include <string.h>

#include "qldpc_polar_int.h"
#include "qldpc_polar_tally_core.h"

#define PLT_CHUNK 64

int qldpc_polar_tally_host(int log2_n, int messages, int maxq, int n_frames, const void *llr, const uint32_t *u_true, uint64_t *tally)
{
    const int rc = pl_args_scalars("polar_tally_host", log2_n, PL_MAX_LOG2N, messages, maxq);
    if (rc) return rc;
    if (n_frames < 0) { qldpc_set_error("polar_tally_host: n_frames=%d is negative", n_frames); return QLDPC_EINVAL; }
    if (n_frames == 0) return QLDPC_OK;
    if (!llr || !u_true || !tally) { qldpc_set_error("polar_tally_host: NULL pointer (llr, u_true and tally are required)"); return QLDPC_EINVAL; }
    const long N = 1l << log2_n, W = pl_words(log2_n), blocks = N >> pl_sub_log(log2_n);
    const int s = 1 << pl_sub_log(log2_n);
    const size_t esz = messages == QLDPC_POLAR_I8 ? 1 : sizeof(float);
    void *leaf = malloc(esz * (size_t)N * PLT_CHUNK);
    if (!leaf) return QLDPC_ENOMEM;
    for (long f0 = 0; f0 < n_frames; f0 += PLT_CHUNK) {
        const int nf = (int)(n_frames - f0 < PLT_CHUNK ? n_frames - f0 : PLT_CHUNK);
        const int rd = qldpc_polar_decode_host(log2_n, 0, NULL, messages, maxq, nf, (const char *)llr + esz * (size_t)(f0 * N), u_true + f0 * W, NULL, NULL, NULL, leaf);
        if (rd) { free(leaf); return rd; }
        for (long f = 0; f < nf; f++)
            for (long j = 0; j < blocks; j++) {
                uint32_t wrong, tie;
                const uint32_t truth = u_true[(f0 + f) * W + j];
                if (messages == QLDPC_POLAR_I8) {
                    int L[32];
                    for (int i = 0; i < s; i++) L[i] = ((const int8_t *)leaf)[f * N + j * s + i];
                    plt_block_words_i8(L, s, truth, &wrong, &tie);
                } else {
                    plt_block_words_f32((const float *)leaf + f * N + j * s, s, truth, &wrong, &tie);
                }
                for (int i = 0; i < s; i++) {
                    tally[j * s + i] += (wrong >> i) & 1u;
                    tally[N + j * s + i] += (tie >> i) & 1u;
                }
            }
    }
    free(leaf);
    return QLDPC_OK;
}

/* a tally's scores into score[N] where no count passes PLT_MAX_COUNT */
static int plt_scores(const char *who, long N, const uint64_t *tally, uint64_t *score)
{
    for (long p = 0; p < N; p++) {
        if (plt_check_count(tally[p], tally[N + p])) {
            qldpc_set_error("%s: a count of position %ld is above 2^40: tally fewer frames", who, p);
            return QLDPC_ESIZE;
        }
        score[p] = plt_score(tally[p], tally[N + p]);
    }
    return QLDPC_OK;
}

/* rank[perm[r]] = r where perm is a permutation of 0 .. N - 1 */
static int plt_rank(const char *who, const char *name, long N, const int *perm, int *rank)
{
    for (long p = 0; p < N; p++) rank[p] = -1;
    for (long r = 0; r < N; r++) {
        const int p = perm[r];
        if (p < 0 || p >= N || rank[p] >= 0) {
            qldpc_set_error("%s: %s is no permutation of 0 .. N - 1 (entry %ld is %d)", who, name, r, p);
            return QLDPC_EINVAL;
        }
        rank[p] = (int)r;
    }
    return QLDPC_OK;
}

/* a stable merge sort of idx[0 .. n) by score descending; tmp holds n entries */
static void plt_sort(int *idx, int *tmp, long n, const uint64_t *score)
{
    for (long w = 1; w < n; w <<= 1) {
        for (long lo = 0; lo < n; lo += 2 * w) {
            const long mid = lo + w < n ? lo + w : n, hi = lo + 2 * w < n ? lo + 2 * w : n;
            long a = lo, b = mid, o = lo;
            while (a < mid && b < hi) tmp[o++] = score[idx[b]] > score[idx[a]] ? idx[b++] : idx[a++];
            while (a < mid) tmp[o++] = idx[a++];
            while (b < hi) tmp[o++] = idx[b++];
        }
        memcpy(idx, tmp, sizeof(int) * (size_t)n);
    }
}

int qldpc_polar_construct_order_host(int log2_n, const uint64_t *tally, const int *prior, int *order)
{
    const char *who = "polar_construct_order_host";
    if (pl_check_size(log2_n, PL_MAX_LOG2N)) { qldpc_set_error("%s: log2_n=%d (1 .. %d)", who, log2_n, PL_MAX_LOG2N); return QLDPC_ESIZE; }
    if (!tally || !order) { qldpc_set_error("%s: NULL pointer (tally and order are required)", who); return QLDPC_EINVAL; }
    const long N = 1l << log2_n;
    uint64_t *score = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)N);
    int *idx = (int *)malloc(sizeof(int) * 2 * (size_t)N);
    int rc = score && idx ? QLDPC_OK : QLDPC_ENOMEM;
    if (!rc) rc = plt_scores(who, N, tally, score);
    if (!rc && prior) rc = plt_rank(who, "prior", N, prior, idx + N);      /* the ranks are only the check */
    if (!rc) {
        for (long r = 0; r < N; r++) idx[r] = prior ? prior[r] : (int)r;  /* in the prior's order, which a stable sort keeps among equal scores */
        plt_sort(idx, idx + N, N, score);
        memcpy(order, idx, sizeof(int) * (size_t)N);
    }
    free(score); free(idx);
    return rc;
}

int qldpc_polar_construct_k_host(int log2_n, const uint64_t *tally, const int *order, uint64_t max_score_sum, int *k)
{
    const char *who = "polar_construct_k_host";
    if (pl_check_size(log2_n, PL_MAX_LOG2N)) { qldpc_set_error("%s: log2_n=%d (1 .. %d)", who, log2_n, PL_MAX_LOG2N); return QLDPC_ESIZE; }
    if (!tally || !order || !k) { qldpc_set_error("%s: NULL pointer (tally, order and k are required)", who); return QLDPC_EINVAL; }
    const long N = 1l << log2_n;
    uint64_t *score = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)N);
    int *rank = (int *)malloc(sizeof(int) * (size_t)N);
    int rc = score && rank ? QLDPC_OK : QLDPC_ENOMEM;
    if (!rc) rc = plt_scores(who, N, tally, score);
    if (!rc) rc = plt_rank(who, "order", N, order, rank);
    if (!rc) {
        uint64_t sum = 0;                                                /* at most 2^20 scores of at most 3 x 2^40 */
        long K = 0;
        while (K < N && sum + score[order[N - 1 - K]] <= max_score_sum) sum += score[order[N - 1 - K++]];
        *k = (int)K;
    }
    free(score); free(rank);
    return rc;
}
