/*
 * qldpc_mc_host.c -- host mirror of the Monte-Carlo frame, channel and pattern definitions (qldpc_mc_philox_host, qldpc_mc_frames_host,
 * qldpc_mc_llr_host, qldpc_mc_pattern_host): the functions of qldpc_mc_core.h that the kernels of qldpc_mc.hip run per lane, here in a loop
 * over frames and words, or over candidates; the table builder of the quantised AWGN channel (qldpc_mc_awgn_table); and the deal of one
 * round of the QBER sweep (qldpc_mc_sweep_deal_host), the function qldpc_mc_sweep itself calls per round.  Plain C, no device.
 */
#include <math.h>
#include <stdlib.h>

#include "../../include/qldpc.h"
#include "qldpc_graph.h"
#include "qldpc_mc_core.h"

int qldpc_mc_philox_host(const uint32_t counter[4], const uint32_t key[2], uint32_t out[4])
{
    if (!counter || !key || !out) return QLDPC_EINVAL;
    mc_philox(counter[0], counter[1], counter[2], counter[3], key[0], key[1], out);
    return QLDPC_OK;
}

int qldpc_mc_frames_host(int K, int N, const int *info_bits_pos, const uint8_t *vn_class, uint64_t seed, double qber, double parity_ber,
                         uint64_t first_frame, int n_frames, uint32_t *info_words, uint32_t *flip_words)
{
    if (K < 1 || N < 1 || K > N) { qldpc_set_error("mc_frames_host: K=%d N=%d", K, N); return QLDPC_ESIZE; }
    if (!(qber >= 0.0 && qber < 1.0) || !(parity_ber >= 0.0 && parity_ber < 1.0)) {
        qldpc_set_error("mc_frames_host: qber=%g parity_ber=%g, both in [0, 1)", qber, parity_ber);
        return QLDPC_ESIZE;
    }
    if (n_frames < 0 || (!info_words && !flip_words)) return QLDPC_EINVAL;
    if (n_frames == 0) return QLDPC_OK;
    const int Wk = (K + 31) / 32, Wn = (N + 31) / 32;
    if (info_words)
        for (int f = 0; f < n_frames; f++)
            for (int j = 0; j < Wk; j++) info_words[(size_t)f * Wk + j] = mc_info_word(seed, first_frame + (uint64_t)f, (uint32_t)j, K);
    if (!flip_words) return QLDPC_OK;
    uint8_t *cls = (uint8_t *)malloc(32 * (size_t)Wn);
    uint32_t *cls4 = (uint32_t *)malloc(4 * 8 * (size_t)Wn);
    int rc = QLDPC_OK;
    if (!cls || !cls4) rc = QLDPC_ENOMEM;
    else if (mc_classes(K, N, info_bits_pos, vn_class, cls, NULL)) {
        qldpc_set_error("mc_frames_host: info_bits_pos outside [0, %d) or repeated, or a VN class above 2", N);
        rc = QLDPC_EINVAL;
    } else {
        mc_pack_classes(cls, Wn, cls4);
        const uint32_t tc = mc_threshold(qber), tp = mc_threshold(parity_ber);
        for (int f = 0; f < n_frames; f++)
            for (int w = 0; w < Wn; w++)
                flip_words[(size_t)f * Wn + w] = mc_flip_word(seed, first_frame + (uint64_t)f, (uint32_t)w, cls4 + 8 * (size_t)w, tc, tp);
    }
    free(cls); free(cls4);
    return rc;
}

int qldpc_mc_awgn_table(double sigma, double rmax, int maxq, uint64_t *cum0, uint64_t *cum1, float *value)
{
    if (!(sigma > 0.0 && sigma < INFINITY) || !(rmax > 0.0 && rmax < INFINITY) || maxq < 1 || 2 * maxq + 2 > MC_SOFT_MAX_LEVELS) {
        qldpc_set_error("mc_awgn_table: sigma=%g rmax=%g (positive, finite), maxq=%d (1 .. %d)", sigma, rmax, maxq, MC_SOFT_MAX_LEVELS / 2 - 1);
        return QLDPC_ESIZE;
    }
    if (!cum0 || !cum1 || !value) return QLDPC_EINVAL;
    const int Q = 2 * maxq + 2;
    uint64_t *cum[2] = {cum0, cum1};
    for (int b = 0; b < 2; b++)
        for (int k = 0; k < Q - 1; k++) {
            const double boundary = (double)(k - maxq) * rmax / (double)maxq, x = (boundary - (double)(1 - 2 * b)) / sigma;
            cum[b][k] = (uint64_t)floor(4294967296.0 * (0.5 * erfc(-x / sqrt(2.0))));
        }
    for (int l = 0; l < Q; l++) value[l] = (float)(l - maxq - 1);
    return QLDPC_OK;
}

int qldpc_mc_llr_host(int K, int N, const int *info_bits_pos, const uint8_t *vn_class, uint64_t seed, double parity_ber, const qldpc_mc_channel *table,
                      const uint32_t *cw_words, uint64_t first_frame, int n_frames, float *llr, uint32_t *flip_words)
{
    if (K < 1 || N < 1 || K > N) { qldpc_set_error("mc_llr_host: K=%d N=%d", K, N); return QLDPC_ESIZE; }
    if (!(parity_ber >= 0.0 && parity_ber < 1.0)) { qldpc_set_error("mc_llr_host: parity_ber=%g outside [0, 1)", parity_ber); return QLDPC_ESIZE; }
    if (!table || n_frames < 0 || (!llr && !flip_words)) return QLDPC_EINVAL;
    if (table->reserved[0] || table->reserved[1]) { qldpc_set_error("mc_llr_host: reserved words of the table must be zero"); return QLDPC_EINVAL; }
    const int Wn = (N + 31) / 32;
    mc_soft_table *t = (mc_soft_table *)malloc(sizeof(*t));
    uint8_t *cls = (uint8_t *)malloc(32 * (size_t)Wn);
    uint32_t *cls4 = (uint32_t *)malloc(4 * 8 * (size_t)Wn);
    int rc = QLDPC_OK;
    if (!t || !cls || !cls4) rc = QLDPC_ENOMEM;
    else if ((rc = mc_soft_table_build(table->levels, table->cum[0], table->cum[1], table->value, t))) {
        qldpc_set_error("mc_llr_host: levels=%d outside 2 .. %d, or a row that decreases or passes 2^32", table->levels, MC_SOFT_MAX_LEVELS);
        rc = rc == -1 ? QLDPC_ESIZE : QLDPC_EINVAL;
    } else if (mc_classes(K, N, info_bits_pos, vn_class, cls, NULL)) {
        qldpc_set_error("mc_llr_host: info_bits_pos outside [0, %d) or repeated, or a VN class above 2", N);
        rc = QLDPC_EINVAL;
    } else {
        mc_pack_classes(cls, Wn, cls4);
        const uint32_t tp = mc_threshold(parity_ber);
        for (int f = 0; f < n_frames; f++)
            for (int w = 0; w < Wn; w++) {
                const uint32_t c = cw_words ? cw_words[(size_t)f * Wn + w] : 0u;
                uint32_t flips = 0;
                for (uint32_t g = 0; g < 8; g++) {
                    float l[4];
                    flips |= mc_soft_quad(seed, first_frame + (uint64_t)f, 8u * (uint32_t)w + g, cls4[8 * (size_t)w + g], (c >> (28u - 4u * g)) & 0xfu, t->thr[0],
                                          t->live[0], t->thr[1], t->live[1], t->value, tp, l) << (28u - 4u * g);
                    for (int b = 0; b < 4 && llr; b++) {
                        const int v = 32 * w + 4 * (int)g + b;
                        if (v < N) llr[(size_t)f * N + v] = l[b];
                    }
                }
                if (flip_words) flip_words[(size_t)f * Wn + w] = flips;
            }
    }
    free(t); free(cls); free(cls4);
    return rc;
}

/* the radix select of qldpc_mc_core.h in a loop over the candidates: per digit one pass that recomputes the keys, then the final pass in index
 * order.  idx = the chosen candidate indices (into the candidate list), ascending. */
int qldpc_mc_pattern_host(uint64_t seed, uint64_t pattern, int n_cand, int n_punct, int key_bits, int *idx)
{
    if (n_cand < 0 || n_punct < 0 || n_punct > n_cand) { qldpc_set_error("mc_pattern_host: n_punct=%d outside [0, n_cand=%d]", n_punct, n_cand); return QLDPC_ESIZE; }
    if (key_bits < 0 || key_bits > 32) { qldpc_set_error("mc_pattern_host: key_bits=%d outside 0 .. 32", key_bits); return QLDPC_ESIZE; }
    if (n_punct == 0) return QLDPC_OK;
    if (!idx) return QLDPC_EINVAL;
    const int kb = mc_key_bits(key_bits);
    const uint32_t blocks = ((uint32_t)n_cand + 3u) / 4u;
    uint32_t prefix = 0, mask = 0, k = (uint32_t)n_punct, u[4];
    for (int shift = mc_select_top_shift(kb); shift >= 0; shift -= MC_SEL_BITS) {
        uint32_t hist[MC_SEL_BINS] = {0};
        for (uint32_t q = 0; q < blocks; q++) {
            mc_pattern_keys(seed, pattern, q, kb, u);
            for (uint32_t b = 0; b < 4 && 4 * q + b < (uint32_t)n_cand; b++)
                if ((u[b] & mask) == prefix) hist[(u[b] >> shift) & (MC_SEL_BINS - 1)]++;
        }
        prefix |= mc_select_digit(hist, &k) << shift;
        mask |= (uint32_t)(MC_SEL_BINS - 1) << shift;
    }
    uint32_t equal = 0;
    int out = 0;      /* reaches n_punct exactly: the candidates below T plus the first k at T */
    for (uint32_t q = 0; q < blocks; q++) {
        mc_pattern_keys(seed, pattern, q, kb, u);
        for (uint32_t b = 0; b < 4 && 4 * q + b < (uint32_t)n_cand; b++) {
            if (out < n_punct && mc_pattern_takes(u[b], prefix, k, equal)) idx[out++] = (int)(4 * q + b);
            equal += u[b] == prefix;
        }
    }
    return QLDPC_OK;
}

int qldpc_mc_sweep_deal_host(int n_points, int chunk, int slots, uint64_t max_frames, uint64_t max_frame_errors, const uint64_t *done,
                             const uint64_t *frame_errors, int *give)
{
    if (n_points < 1 || n_points > MC_SWEEP_MAX_POINTS || chunk < 1 || slots < 1 || max_frames == 0) {
        qldpc_set_error("mc_sweep_deal_host: n_points=%d (1 .. %d), chunk=%d, slots=%d (at least 1), max_frames=%llu (at least 1)", n_points, MC_SWEEP_MAX_POINTS,
                        chunk, slots, (unsigned long long)max_frames);
        return QLDPC_ESIZE;
    }
    if (!done || !frame_errors || !give) return QLDPC_EINVAL;
    return mc_sweep_deal(n_points, chunk, slots, max_frames, max_frame_errors, done, frame_errors, give);
}
