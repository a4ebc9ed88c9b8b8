/*
 * qldpc_blind_host.c -- the host side of blind reconciliation that needs no device: the mirror of the weakest-VN select
 * (qldpc_weakest_core.h, the functions the lanes of qk_weakest run) and Alice's answer to a request for key bits.
 */
#include <stdlib.h>

#include "../../include/qldpc.h"
#include "qldpc_weakest_core.h"

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
