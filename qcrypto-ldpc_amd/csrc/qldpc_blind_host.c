/*
 * qldpc_blind_host.c -- the host side of blind reconciliation that needs no device: the mirror of the weakest-VN select
 * (qldpc_weakest_core.h, the functions the lanes of qk_weakest run), Alice's answer to a request for key bits, and the mirror of the give-up rule
 * of the early-exit run (qldpc_giveup_core.h, the functions the lanes of qk_status_count run).
 */
#include <stdlib.h>

#include "../../include/qldpc.h"
#include "qldpc_weakest_core.h"
#include "qldpc_giveup_core.h"

int qldpc_weakest_host(const float *post, int N, const uint32_t *cand_bits, int d, uint32_t *weak_bits, int *n_taken)
{
    if (!post || !weak_bits || N <= 0 || d < 0) return QLDPC_EINVAL;
    const int W = (N + 31) / 32;
    uint32_t hist[WK_BINS];
    uint32_t T = 0, rem = 0, total = 0;
    for (int p = 0; p < WK_DIGITS; p++) {
        memset(hist, 0, sizeof hist);
        for (int w = 0; w < W; w++) {
            const uint32_t c = wk_cand_word(cand_bits, w, N);
            for (int b = 0; b < 32 && c; b++) {
                if (!((c >> (31 - b)) & 1u)) continue;
                uint32_t bits;
                memcpy(&bits, &post[w * 32 + b], sizeof bits);
                const uint32_t key = wk_key_of_bits(bits);
                if (wk_agrees(key, T, p)) hist[wk_digit(key, p)]++;
            }
        }
        if (p == 0) {
            for (int b = 0; b < WK_BINS; b++) total += hist[b];
            rem = (uint32_t)d < total ? (uint32_t)d : total;
            if (rem == 0) break;
        }
        uint32_t in_bin;
        T |= wk_pick(hist, 1, &rem, &in_bin) << (24 - 8 * p);
    }
    if (rem == 0) T = 0;
    uint32_t run = 0;
    int taken = 0;
    for (int w = 0; w < W; w++) {
        const uint32_t c = wk_cand_word(cand_bits, w, N);
        uint32_t out = 0;
        for (int b = 0; b < 32 && c; b++) {
            if (!((c >> (31 - b)) & 1u)) continue;
            uint32_t bits;
            memcpy(&bits, &post[w * 32 + b], sizeof bits);
            if (wk_taken(wk_key_of_bits(bits), T, rem, &run)) { out |= 0x80000000u >> b; taken++; }
        }
        weak_bits[w] = out;
    }
    if (n_taken) *n_taken = taken;
    return QLDPC_OK;
}

/* Alice: bit[i] = bit pos[i] of her key, MSB-first */
int qldpc_recon_disclose_host(const uint32_t *key_words, int key_bits, const int *pos, int n, uint8_t *bit)
{
    if (!key_words || key_bits <= 0 || n < 0 || (n && (!pos || !bit))) return QLDPC_EINVAL;
    for (int i = 0; i < n; i++)
        if (pos[i] < 0 || pos[i] >= key_bits) return QLDPC_EINVAL;
    for (int i = 0; i < n; i++) bit[i] = (uint8_t)((key_words[pos[i] >> 5] >> (31 - (pos[i] & 31))) & 1u);
    return QLDPC_OK;
}

/* one frame: weights[t] = its syndrome weight at test t + 1 of a run that never stops it */
int qldpc_giveup_host(const int *weights, int n_tests, int syndrome_depth, int patience, int *stop_test, int *outcome)
{
    if (!weights || n_tests < 1 || syndrome_depth < 1 || patience < 0) return QLDPC_EINVAL;
    for (int t = 0; t < n_tests; t++) if (weights[t] < 0) return QLDPC_EINVAL;
    int best, since, depth = 0, stop = 0, what = GU_RAN_OUT;
    gu_reset(&best, &since);
    for (int t = 0; t < n_tests && !stop; t++) {
        const int now = gu_converges(&depth, weights[t] == 0, syndrome_depth);
        gu_observe(&best, &since, weights[t]);
        if (now) { stop = t + 1; what = GU_CONVERGED; }
        else if (patience > 0 && gu_gives_up(weights[t], since, patience, now)) { stop = t + 1; what = GU_GAVE_UP; }
    }
    if (stop_test) *stop_test = stop;
    if (outcome) *outcome = what;
    return QLDPC_OK;
}
