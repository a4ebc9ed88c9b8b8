/*
 * qldpc_mc_host.c -- host mirror of the Monte-Carlo frame, channel and pattern definitions (qldpc_mc_philox_host, qldpc_mc_frames_host,
 * qldpc_mc_llr_host, qldpc_mc_pattern_host, qldpc_mc_weight_frames_host): the functions of qldpc_mc_core.h that the kernels of qldpc_mc.hip
 * run per lane, here in a loop over frames and words, or over candidates; the table builder of the quantised AWGN channel
 * (qldpc_mc_awgn_table); the deal of one round of the QBER sweep (qldpc_mc_sweep_deal_host), the function qldpc_mc_sweep itself calls per
 * round; the argument checks of the sweep over table channels (qldpc_mc_sweep_tables_check_host), which qldpc_mc_sweep_tables runs first; the FER estimate over fixed-weight strata (qldpc_mc_strata_fer_host); and the schedule of the blind reconciliation rounds
 * (qldpc_mc_blind_next_host, the function qldpc_mc_blind itself calls per launch) with the efficiency they end at
 * (qldpc_mc_blind_efficiency_host); and the schedule of the guessing rounds (qldpc_mc_guess_next_host, the function qldpc_mc_guess itself calls per
 * launch).  Plain C, no device.
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

/* *out = the padded class map of (K, N, info_bits_pos, vn_class) in the four-per-word form of mc_flip_word: 8 ceil(N / 32) words that the caller
 * frees; *channel_vns (optional) grows by the number of QLDPC_VN_CHANNEL VNs.  On an error *out = NULL and the text goes under the caller's name */
static int mc_class_words(const char *who, int K, int N, const int *info_bits_pos, const uint8_t *vn_class, uint32_t **out, int *channel_vns)
{
    const int Wn = (N + 31) / 32;
    uint8_t *cls = (uint8_t *)malloc(32 * (size_t)Wn);
    uint32_t *cls4 = (uint32_t *)malloc(4 * 8 * (size_t)Wn);
    int rc = QLDPC_OK;
    if (!cls || !cls4) rc = QLDPC_ENOMEM;
    else if (mc_classes(K, N, info_bits_pos, vn_class, cls, NULL)) {
        qldpc_set_error("%s: info_bits_pos outside [0, %d) or repeated, or a VN class above 2", who, N);
        rc = QLDPC_EINVAL;
    } else {
        mc_pack_classes(cls, Wn, cls4);
        for (int v = 0; v < N && channel_vns; v++) *channel_vns += cls[v] == 0;
    }
    free(cls);
    if (rc) { free(cls4); cls4 = NULL; }
    *out = cls4;
    return rc;
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
    uint32_t *cls4;
    const int rc = mc_class_words("mc_frames_host", K, N, info_bits_pos, vn_class, &cls4, NULL);
    if (rc) return rc;
    const uint32_t tc = mc_threshold(qber), tp = mc_threshold(parity_ber);
    for (int f = 0; f < n_frames; f++)
        for (int w = 0; w < Wn; w++)
            flip_words[(size_t)f * Wn + w] = mc_flip_word(seed, first_frame + (uint64_t)f, (uint32_t)w, cls4 + 8 * (size_t)w, tc, tp);
    free(cls4);
    return QLDPC_OK;
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
    uint32_t *cls4 = NULL;
    int rc = QLDPC_OK;
    if (!t) rc = QLDPC_ENOMEM;
    else if ((rc = mc_soft_table_build(table->levels, table->cum[0], table->cum[1], table->value, t))) {
        qldpc_set_error("mc_llr_host: levels=%d outside 2 .. %d, or a row that decreases or passes 2^32", table->levels, MC_SOFT_MAX_LEVELS);
        rc = rc == -1 ? QLDPC_ESIZE : QLDPC_EINVAL;
    } else if (!(rc = mc_class_words("mc_llr_host", K, N, info_bits_pos, vn_class, &cls4, NULL))) {
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
    free(t); free(cls4);
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

/* every argument check of qldpc_mc_sweep_tables, which runs it first: the codes of qldpc_mc_sweep in its order, per table those of
 * qldpc_mc_set_channel (every table is built once into a scratch table, as qldpc_mc_set_channel builds its own) */
int qldpc_mc_sweep_tables_check_host(int N, int batch, const qldpc_mc_sweep_tables_cfg *cfg)
{
    const char *who = "mc_sweep_tables";
    if (!cfg) return QLDPC_EINVAL;
    if (N < 1 || batch < 1) { qldpc_set_error("%s: N=%d batch=%d", who, N, batch); return QLDPC_ESIZE; }
    if (cfg->reserved[0] || cfg->reserved[1]) { qldpc_set_error("%s: reserved fields %d, %d must be zero", who, cfg->reserved[0], cfg->reserved[1]); return QLDPC_EINVAL; }
    if (cfg->n_points < 1 || cfg->n_points > MC_SWEEP_MAX_POINTS) { qldpc_set_error("%s: n_points=%d outside 1 .. %d", who, cfg->n_points, MC_SWEEP_MAX_POINTS); return QLDPC_ESIZE; }
    if (cfg->chunk < 0 || cfg->chunk > batch) { qldpc_set_error("%s: chunk=%d outside [0, batch=%d]", who, cfg->chunk, batch); return QLDPC_ESIZE; }
    if (cfg->max_frames == 0) { qldpc_set_error("%s: max_frames=0", who); return QLDPC_ESIZE; }
    if ((uint64_t)batch * 8u * (uint64_t)((N + 31) / 32) >= (1ull << 31)) { qldpc_set_error("%s: %d frames of N = %d pass 2^31 lanes of four VNs", who, batch, N); return QLDPC_ESIZE; }
    if (!cfg->points || cfg->n_order < 0 || (cfg->n_order > 0 && !cfg->punct_order)) { qldpc_set_error("%s: a missing array (points, or punct_order with n_order=%d)", who, cfg->n_order); return QLDPC_EINVAL; }
    uint8_t *seen = (uint8_t *)calloc((size_t)N, 1);
    mc_soft_table *t = (mc_soft_table *)malloc(sizeof(*t));
    int rc = seen && t ? QLDPC_OK : QLDPC_ENOMEM;
    const int bad = rc ? -1 : mc_punct_order_check(cfg->punct_order, cfg->n_order, N, seen);
    if (bad >= 0) { qldpc_set_error("%s: punct_order[%d] = %d is repeated or outside [0, %d)", who, bad, cfg->punct_order[bad], N); rc = QLDPC_EINVAL; }
    for (int q = 0; q < cfg->n_points && !rc; q++) {
        const qldpc_mc_table_point *pt = &cfg->points[q];
        const int dirty = pt->reserved || pt->table.reserved[0] || pt->table.reserved[1];
        const int built = dirty ? 0 : mc_soft_table_build(pt->table.levels, pt->table.cum[0], pt->table.cum[1], pt->table.value, t);
        if (dirty) { qldpc_set_error("%s: reserved fields of point %d or of its table must be zero", who, q); rc = QLDPC_EINVAL; }
        else if (built == -1) { qldpc_set_error("%s: levels=%d of point %d outside 2 .. %d", who, pt->table.levels, q, MC_SOFT_MAX_LEVELS); rc = QLDPC_ESIZE; }
        else if (built) { qldpc_set_error("%s: the table of point %d has a missing array, a row that decreases or an entry above 2^32", who, q); rc = QLDPC_EINVAL; }
        else if (pt->n_punct < 0 || pt->n_punct > cfg->n_order) { qldpc_set_error("%s: n_punct=%d of point %d outside [0, n_order=%d]", who, pt->n_punct, q, cfg->n_order); rc = QLDPC_ESIZE; }
    }
    free(seen); free(t);
    return rc;
}

/* the radix select of a fixed-weight frame (qldpc_mc_core.h) in a loop over the quads: per digit one pass that recomputes the keys of the
 * channel VNs, then the final pass word by word with the running count of equal keys that the kernel forms by a prefix over its lanes */
int qldpc_mc_weight_frames_host(int K, int N, const int *info_bits_pos, const uint8_t *vn_class, uint64_t seed, double parity_ber, uint64_t first_frame,
                                int n_frames, const int *weights, int key_bits, uint32_t *info_words, uint32_t *flip_words)
{
    if (K < 1 || N < 1 || K > N) { qldpc_set_error("mc_weight_frames_host: K=%d N=%d", K, N); return QLDPC_ESIZE; }
    if (!(parity_ber >= 0.0 && parity_ber < 1.0)) { qldpc_set_error("mc_weight_frames_host: parity_ber=%g outside [0, 1)", parity_ber); return QLDPC_ESIZE; }
    if (key_bits < 0 || key_bits > 32) { qldpc_set_error("mc_weight_frames_host: key_bits=%d outside 0 .. 32", key_bits); return QLDPC_ESIZE; }
    if (n_frames < 0 || (!info_words && !flip_words) || (n_frames > 0 && flip_words && !weights)) return QLDPC_EINVAL;
    if (n_frames == 0) return QLDPC_OK;
    const int Wk = (K + 31) / 32, Wn = (N + 31) / 32, kb = mc_key_bits(key_bits);
    uint32_t *cls4;
    int channel_vns = 0, rc = mc_class_words("mc_weight_frames_host", K, N, info_bits_pos, vn_class, &cls4, &channel_vns);
    for (int f = 0; f < n_frames && flip_words && !rc; f++)
        if (weights[f] < 0 || weights[f] > channel_vns) {
            qldpc_set_error("mc_weight_frames_host: weights[%d]=%d outside [0, %d channel VNs]", f, weights[f], channel_vns);
            rc = QLDPC_ESIZE;
        }
    if (rc) { free(cls4); return rc; }      /* nothing is written by a refused call */
    if (info_words)
        for (int f = 0; f < n_frames; f++)
            for (int j = 0; j < Wk; j++) info_words[(size_t)f * Wk + j] = mc_info_word(seed, first_frame + (uint64_t)f, (uint32_t)j, K);
    const uint32_t tp = mc_threshold(parity_ber);
    for (int f = 0; f < n_frames && flip_words; f++) {
        const uint64_t frame = first_frame + (uint64_t)f;
        uint32_t prefix = 0, mask = 0, k = (uint32_t)weights[f], u[4];
        for (int shift = mc_select_top_shift(kb); shift >= 0 && weights[f] > 0; shift -= MC_SEL_BITS) {
            uint32_t hist[MC_SEL_BINS] = {0};
            for (uint32_t g = 0; g < 8u * (uint32_t)Wn; g++) {
                const uint32_t m = mc_weight_quad(seed, frame, g, cls4[g], 0u, u);
                for (uint32_t b = 0; b < 4; b++) {
                    const uint32_t key = u[b] >> (32 - kb);
                    if (((m >> b) & 1u) && (key & mask) == prefix) hist[(key >> shift) & (MC_SEL_BINS - 1)]++;
                }
            }
            prefix |= mc_select_digit(hist, &k) << shift;
            mask |= (uint32_t)(MC_SEL_BINS - 1) << shift;
        }
        uint32_t equal = 0;      /* T = prefix, r = k (weight 0: both 0) */
        for (int w = 0; w < Wn; w++) {
            uint32_t less, eq, pin;
            mc_weight_masks(seed, frame, (uint32_t)w, cls4 + 8 * (size_t)w, kb, prefix, tp, &less, &eq, &pin);
            flip_words[(size_t)f * Wn + w] = mc_weight_take(less, eq, prefix, k, equal) | pin;
            equal += (uint32_t)__builtin_popcount(eq);
        }
    }
    free(cls4);
    return QLDPC_OK;
}

/* Binom(n, q)(w) in double by lgamma */
static double mc_binom_pmf(int n, int w, double lq, double l1q)
{
    return exp(lgamma((double)n + 1.0) - lgamma((double)w + 1.0) - lgamma((double)(n - w) + 1.0) + (double)w * lq + (double)(n - w) * l1q);
}

int qldpc_mc_strata_fer_host(int n_channel, int n_strata, const int *weights, const uint64_t *frames, const uint64_t *frame_errors, double qber, double out[4])
{
    if (n_channel < 1 || n_strata < 1 || n_strata > MC_SWEEP_MAX_POINTS || !(qber > 0.0 && qber < 1.0)) {
        qldpc_set_error("mc_strata_fer_host: n_channel=%d (at least 1), n_strata=%d (1 .. %d), qber=%g (inside (0, 1))", n_channel, n_strata, MC_SWEEP_MAX_POINTS, qber);
        return QLDPC_ESIZE;
    }
    if (!weights || !frames || !frame_errors || !out) return QLDPC_EINVAL;
    for (int s = 0; s < n_strata; s++) {
        if (weights[s] < 0 || weights[s] > n_channel) { qldpc_set_error("mc_strata_fer_host: weights[%d]=%d outside [0, %d]", s, weights[s], n_channel); return QLDPC_ESIZE; }
        if (s > 0 && weights[s] <= weights[s - 1]) { qldpc_set_error("mc_strata_fer_host: weights[%d]=%d is not above weights[%d]=%d", s, weights[s], s - 1, weights[s - 1]); return QLDPC_EINVAL; }
        if (frames[s] == 0 || frame_errors[s] > frames[s]) {
            qldpc_set_error("mc_strata_fer_host: stratum %d has %llu frames and %llu frame errors", s, (unsigned long long)frames[s], (unsigned long long)frame_errors[s]);
            return QLDPC_ESIZE;
        }
    }
    const double lq = log(qber), l1q = log1p(-qber);
    double fer = 0.0, var = 0.0, below = 0.0, above = 0.0;
    for (int w = 0; w < weights[0]; w++) below += mc_binom_pmf(n_channel, w, lq, l1q);
    for (int w = weights[n_strata - 1] + 1; w <= n_channel; w++) above += mc_binom_pmf(n_channel, w, lq, l1q);
    for (int s = 0; s < n_strata; s++) {      /* c_s: the stratum's own weight, and its share of the weights between it and both neighbours */
        double c = mc_binom_pmf(n_channel, weights[s], lq, l1q);
        if (s > 0)
            for (int w = weights[s - 1] + 1; w < weights[s]; w++)
                c += mc_binom_pmf(n_channel, w, lq, l1q) * ((double)(w - weights[s - 1]) / (double)(weights[s] - weights[s - 1]));
        if (s + 1 < n_strata)
            for (int w = weights[s] + 1; w < weights[s + 1]; w++)
                c += mc_binom_pmf(n_channel, w, lq, l1q) * ((double)(weights[s + 1] - w) / (double)(weights[s + 1] - weights[s]));
        const double p = (double)frame_errors[s] / (double)frames[s];
        fer += c * p;
        var += c * c * p * (1.0 - p) / (double)frames[s];
    }
    out[0] = fer; out[1] = below; out[2] = above; out[3] = sqrt(var);
    return QLDPC_OK;
}

int qldpc_mc_blind_next_host(int max_rounds, int batch, const uint64_t *pool, uint64_t input_left, int *level, int *n)
{
    if (max_rounds < 0 || max_rounds > MC_BLIND_MAX_ROUNDS || batch < 1) {
        qldpc_set_error("mc_blind_next_host: max_rounds=%d (0 .. %d), batch=%d (at least 1)", max_rounds, MC_BLIND_MAX_ROUNDS, batch);
        return QLDPC_ESIZE;
    }
    if (!pool || !level || !n) return QLDPC_EINVAL;
    return mc_blind_next(max_rounds, batch, pool, input_left, level, n);
}

int qldpc_mc_guess_next_host(int guess_bits, int batch, uint64_t pool, uint64_t input_left, int *kind, int *n)
{
    if (guess_bits < 0 || guess_bits > MC_GUESS_MAX_BITS || batch < 1 || (1 << guess_bits) > batch) {
        qldpc_set_error("mc_guess_next_host: guess_bits=%d (0 .. %d), batch=%d (at least 1 and at least 2^guess_bits)", guess_bits, MC_GUESS_MAX_BITS, batch);
        return QLDPC_ESIZE;
    }
    if (!kind || !n) return QLDPC_EINVAL;
    return mc_guess_next(guess_bits, batch, pool, input_left, kind, n);
}

int qldpc_mc_blind_efficiency_host(int n_channel, int n_disclosed_parity, uint64_t frames, uint64_t disclosed, double qber, double *f)
{
    if (n_channel < 1 || n_disclosed_parity < 0 || frames == 0 || !(qber > 0.0 && qber < 0.5)) {
        qldpc_set_error("mc_blind_efficiency_host: n_channel=%d (at least 1), n_disclosed_parity=%d (not negative), frames=%llu (at least 1), qber=%g (inside (0, 0.5))",
                        n_channel, n_disclosed_parity, (unsigned long long)frames, qber);
        return QLDPC_ESIZE;
    }
    if (!f) return QLDPC_EINVAL;
    const double h2 = -qber * log2(qber) - (1.0 - qber) * log2(1.0 - qber);
    *f = ((double)n_disclosed_parity + (double)disclosed / (double)frames) / ((double)n_channel * h2);
    return QLDPC_OK;
}
