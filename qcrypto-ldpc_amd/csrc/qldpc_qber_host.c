/*
 * qldpc_qber_host.c -- the host side of the syndrome-weight QBER estimate that needs no device: the grid and score tables (built here in double,
 * uploaded by qldpc_qber_create), and the mirrors of the counting and the argmax kernels over the functions of qldpc_qber_core.h.
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/qldpc.h"
#include "qldpc_graph.h"
#include "qldpc_qber_core.h"

int qldpc_qber_table_host(int max_degree, int n_grid, float q_lo, float q_hi, int32_t *L1, int32_t *L0, float *q, float *llr)
{
    if (max_degree < 1 || n_grid < 2 || n_grid > QB_MAX_GRID || !((double)q_lo >= QB_MIN_Q_LO) || !(q_hi > q_lo) || !(q_hi < 0.5f)) {
        qldpc_set_error("qber_table: need max_degree >= 1, 2 <= n_grid <= %d, %g <= q_lo < q_hi < 0.5 (got %d, %d, %g, %g)", QB_MAX_GRID, QB_MIN_Q_LO,
                        max_degree, n_grid, (double)q_lo, (double)q_hi);
        return QLDPC_EINVAL;
    }
    if (max_degree > QB_MAX_DEGREE) { qldpc_set_error("qber_table: check degree %d > %d", max_degree, QB_MAX_DEGREE); return QLDPC_EUNSUPPORTED; }
    for (int k = 0; k < n_grid; k++) {
        const double qk = (double)q_lo * pow((double)q_hi / (double)q_lo, (double)k / (double)(n_grid - 1));
        if (q) q[k] = (float)qk;
        if (llr) llr[k] = qldpc_bsc_llr((float)qk);
        if (L1) L1[k] = 0;
        if (L0) L0[k] = 0;
        for (int d = 1; d <= max_degree; d++) {
            const double p = -0.5 * expm1((double)d * log1p(-2.0 * qk));      /* (1 - (1 - 2 q)^d) / 2 */
            if (L1) L1[(size_t)d * n_grid + k] = (int32_t)llround(log(p) * QB_SCALE);
            if (L0) L0[(size_t)d * n_grid + k] = (int32_t)llround(log1p(-p) * QB_SCALE);
        }
    }
    return QLDPC_OK;
}

/* one frame: counts[D + 1][2] */
int qldpc_qber_counts_host(const qldpc_code *code, const uint32_t *bits, const uint8_t *vn_class, int n_channel, const uint32_t *synd,
                           const uint32_t *erase, const uint32_t *known, const uint32_t *value, uint32_t *counts)
{
    if (!code || !bits || !counts || (known && !value)) return QLDPC_EINVAL;
    const int N = code->N, M = code->M, D = code->max_dc, Wn = (N + 31) / 32;
    uint32_t *rows = (uint32_t *)malloc(sizeof(uint32_t) * 3 * (size_t)Wn);
    if (!rows) return QLDPC_ENOMEM;
    uint32_t *val = rows, *noisy = rows + Wn, *erased = rows + 2 * (size_t)Wn;
    for (int w = 0; w < Wn; w++) {
        uint32_t pi, pu;
        qb_class_word(vn_class, w, N, &pi, &pu);
        qb_collapse_word(bits[w], erase ? erase[w] : 0u, known ? known[w] : 0u, known ? value[w] : 0u, pi, pu, qb_below_word(w, n_channel),
                         &val[w], &noisy[w], &erased[w]);
    }
    memset(counts, 0, sizeof(uint32_t) * 2 * (size_t)(D + 1));
    for (int c = 0; c < M; c++) {
        uint32_t u = synd ? qb_bit(synd, c) : 0u, er = 0;
        int d = 0;
        for (int k = code->cn_ptr[c]; k < code->cn_ptr[c + 1]; k++) {
            const int v = code->cn_var[k];
            u ^= qb_bit(val, v);
            d += (int)qb_bit(noisy, v);
            er |= qb_bit(erased, v);
        }
        if (er) continue;
        counts[2 * d] += 1;
        counts[2 * d + 1] += u;
    }
    free(rows);
    return QLDPC_OK;
}

int qldpc_qber_argmax_host(const uint64_t *counts, int max_degree, int n_grid, const int32_t *L1, const int32_t *L0, int *index)
{
    if (!counts || !L1 || !L0 || !index || max_degree < 1 || max_degree > QB_MAX_DEGREE || n_grid < 2 || n_grid > QB_MAX_GRID) return QLDPC_EINVAL;
    uint64_t total = 0;
    for (int d = 0; d <= max_degree; d++) {
        if (counts[2 * d + 1] > counts[2 * d] || counts[2 * d] >= (1ull << 35)) { qldpc_set_error("qber_argmax: bad counts at degree %d", d); return QLDPC_EINVAL; }
        total += counts[2 * d];
    }
    if (total >= (1ull << 35)) { qldpc_set_error("qber_argmax: 2^35 checks or more, the score could overflow"); return QLDPC_EINVAL; }
    int best_k = -1;
    int64_t best_S = 0;
    if (qb_observations(counts, max_degree))
        for (int k = 0; k < n_grid; k++) {
            const int64_t S = qb_score(counts, max_degree, L1, L0, n_grid, k);
            if (qb_better(S, k, best_S, best_k)) { best_S = S; best_k = k; }
        }
    *index = best_k;
    return QLDPC_OK;
}
