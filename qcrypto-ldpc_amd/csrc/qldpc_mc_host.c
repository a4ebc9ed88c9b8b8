/*
 * qldpc_mc_host.c -- host mirror of the Monte-Carlo frame and pattern definitions (qldpc_mc_philox_host, qldpc_mc_frames_host,
 * qldpc_mc_pattern_host): the functions of qldpc_mc_core.h that the kernels of qldpc_mc.hip run per lane, here in a loop over frames and
 * words, or over candidates.  Plain C, no device.
 */
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
