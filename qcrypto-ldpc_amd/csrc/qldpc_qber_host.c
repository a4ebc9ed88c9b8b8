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

/* the transposed check table tab[D][M] of a code, -1 past a check's degree: what the counting kernels walk */
static void check_table(const qldpc_code *code, int *tab)
{
    const int M = code->M, D = code->max_dc;
    for (int c = 0; c < M; c++)
        for (int j = 0; j < D; j++) {
            const int k = code->cn_ptr[c] + j;
            tab[(size_t)j * M + c] = k < code->cn_ptr[c + 1] ? code->cn_var[k] : -1;
        }
}

/*
 * The merged count's view of a code given as its transposed check table tab[D][M]: verifies edge by edge that the parity part is an accumulator chain
 * (qldpc_qber_core.h: QLDPC_EUNSUPPORTED and the reason in the error text if not) and fills the repeat table rep[D][M] (NULL = verify only): for every
 * edge the distance back to the nearest earlier check within QB_MAX_RUN - 1 that holds the same VN, or 0.
 */
int qldpc_qber_repeat_table_host(const int *tab, int N, int M, int D, uint8_t *rep)
{
    if (!tab || N < 1 || M < 1 || D < 1) return QLDPC_EINVAL;
    const int K = N - M;
    if (K < 0) { qldpc_set_error("qber merge: M = %d > N = %d", M, N); return QLDPC_EUNSUPPORTED; }
    int *last = (int *)malloc(sizeof(int) * (size_t)N);      /* the last check so far that holds VN v */
    if (!last) return QLDPC_ENOMEM;
    for (int v = 0; v < N; v++) last[v] = -1;
    int rc = QLDPC_OK;
    for (int c = 0; c < M && !rc; c++) {
        int own = 0, left = 0;      /* VN K + c and VN K + c - 1 seen in this row */
        for (int j = 0; j < D; j++) {
            const int v = tab[(size_t)j * M + c];
            if (v < 0) break;
            if (v >= N) { rc = QLDPC_EINVAL; break; }
            if (v >= K) {
                if (v == K + c && !own) own = 1;
                else if (c > 0 && v == K + c - 1 && !left) left = 1;
                else { qldpc_set_error("qber merge: no accumulator chain, check %d holds parity VN %d", c, v); rc = QLDPC_EUNSUPPORTED; break; }
            }
            const int back = last[v] >= 0 && last[v] < c ? c - last[v] : 0;
            if (rep) rep[(size_t)j * M + c] = (uint8_t)(back < QB_MAX_RUN ? back : 0);
        }
        if (!rc && (!own || (c > 0 && !left))) {
            qldpc_set_error("qber merge: no accumulator chain, check %d lacks parity VN %d", c, own ? K + c - 1 : K + c);
            rc = QLDPC_EUNSUPPORTED;
        }
        for (int j = 0; j < D && !rc; j++) {
            const int v = tab[(size_t)j * M + c];
            if (v < 0) break;
            last[v] = c;
        }
    }
    free(last);
    return rc;
}

/* one frame, merged: counts[QB_MAX_DEGREE + 1][2] */
int qldpc_qber_counts_merged_host(const qldpc_code *code, const uint32_t *bits, const uint8_t *vn_class, int n_channel, const uint32_t *synd,
                                  const uint32_t *erase, const uint32_t *known, const uint32_t *value, uint32_t *counts)
{
    if (!code || !bits || !counts || (known && !value)) return QLDPC_EINVAL;
    const int N = code->N, M = code->M, D = code->max_dc, K = N - M, Wn = (N + 31) / 32;
    uint32_t *rows = (uint32_t *)malloc(sizeof(uint32_t) * 3 * (size_t)Wn);
    int *tab = (int *)malloc(sizeof(int) * (size_t)D * (size_t)M);
    uint8_t *rep = (uint8_t *)malloc((size_t)D * (size_t)M);
    if (!rows || !tab || !rep) { free(rows); free(tab); free(rep); return QLDPC_ENOMEM; }
    check_table(code, tab);
    const int rc = qldpc_qber_repeat_table_host(tab, N, M, D, rep);
    if (rc) { free(rows); free(tab); free(rep); return rc; }
    uint32_t *val = rows, *noisy = rows + Wn, *erased = rows + 2 * (size_t)Wn;
    for (int w = 0; w < Wn; w++) {
        uint32_t pi, pu;
        qb_class_word(vn_class, w, N, &pi, &pu);
        qb_collapse_word(bits[w], erase ? erase[w] : 0u, known ? known[w] : 0u, known ? value[w] : 0u, pi, pu, qb_below_word(w, n_channel),
                         &val[w], &noisy[w], &erased[w]);
    }
    memset(counts, 0, sizeof(uint32_t) * 2 * (QB_MAX_DEGREE + 1));
    for (int h = 0; h < M; h++) {
        if (h > 0 && qb_bit(erased, K + h - 1)) continue;      /* no head */
        const int w0 = (K + h) >> 5;
        const int len = qb_run_checks(erased[w0], w0 + 1 < Wn ? erased[w0 + 1] : 0u, K, h, M), t = h + len - 1;
        if (len > QB_MAX_RUN) continue;
        uint32_t u = 0, er = 0;
        int d = 0;
        for (int c = h; c <= t; c++) {
            if (synd) u ^= qb_bit(synd, c);
            for (int j = 0; j < D; j++) {
                const int v = tab[(size_t)j * M + c];
                if (v < 0) break;
                if (qb_is_link(v, K, h, t)) continue;
                u ^= qb_bit(val, v);
                er |= qb_bit(erased, v);
                if (qb_bit(noisy, v)) d += (qb_earlier_in_run(tab, rep, M, D, rep[(size_t)j * M + c], c, v, h) & 1) ? -1 : 1;
            }
        }
        if (er || d > QB_MAX_DEGREE) continue;
        counts[2 * d] += 1;
        counts[2 * d + 1] += u;
    }
    free(rows); free(tab); free(rep);
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
