/* Sanitizer pass over the host side of the fixed-weight error strata (qldpc_mc_weight_frames_host and qldpc_mc_strata_fer_host in
 * qldpc_mc_host.c over qldpc_mc_core.h, no HIP): the two mirrors over edge shapes -- weight 0, weight = every channel VN, N = 33 (one VN in
 * the last word), N % 4 != 0, key_bits = 1, the three classes interleaved, a frame index across 2^32 -- into arrays of exactly the documented
 * sizes; per row the popcount over the channel VNs, nothing past N, nested sets; refused arguments write nothing.
 * Built with -fsanitize=address,undefined by tests/test_mc_strata.py */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "qldpc.h"
#include "qldpc_mc_core.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

static int popcount_masked(const uint32_t *row, const uint8_t *cls, int N, int want_class)
{
    int n = 0;
    for (int v = 0; v < N; v++) n += ((row[v >> 5] >> (31 - (v & 31))) & 1u) && cls[v] == want_class;
    return n;
}

/* every weight of `ws` over `n` frames of one shape; cls[N] = the class map (NULL: channel at 0 .. K-1, pinned elsewhere) */
static int shape(int K, int N, const uint8_t *cls_in, uint64_t first, int n, int key_bits, double parity_ber)
{
    const int Wn = (N + 31) / 32, Wk = (K + 31) / 32;
    uint8_t *cls = malloc((size_t)N);
    int channel = 0;
    for (int v = 0; v < N; v++) { cls[v] = cls_in ? cls_in[v] : (v < K ? 0 : 1); channel += cls[v] == 0; }
    uint32_t *info = malloc(sizeof(uint32_t) * (size_t)n * (size_t)Wk), *flips = malloc(sizeof(uint32_t) * (size_t)n * (size_t)Wn);
    uint32_t *prev = calloc((size_t)n * (size_t)Wn, sizeof(uint32_t));
    int *weights = malloc(sizeof(int) * (size_t)n);
    const int ws[] = {0, 1, channel / 2, channel - 1, channel};
    int last = -1;
    for (unsigned i = 0; i < sizeof(ws) / sizeof(ws[0]); i++) {
        if (ws[i] < 0 || ws[i] <= last) continue;
        for (int f = 0; f < n; f++) weights[f] = ws[i];
        CHECK(qldpc_mc_weight_frames_host(K, N, NULL, cls_in, 0x1234567ull, parity_ber, first, n, weights, key_bits, info, flips) == QLDPC_OK);
        for (int f = 0; f < n; f++) {
            const uint32_t *row = flips + (size_t)f * Wn;
            CHECK(popcount_masked(row, cls, N, 0) == ws[i]);
            CHECK(popcount_masked(row, cls, N, 2) == 0);
            if (parity_ber == 0.0) CHECK(popcount_masked(row, cls, N, 1) == 0);
            if (N & 31) CHECK((row[Wn - 1] & ~mc_tail_mask(N)) == 0);      /* nothing past N */
            for (int w = 0; w < Wn; w++) CHECK((prev[(size_t)f * Wn + w] & ~row[w]) == 0);      /* nested in the weight */
        }
        memcpy(prev, flips, sizeof(uint32_t) * (size_t)n * (size_t)Wn);
        last = ws[i];
    }
    /* info words alone, flip words alone */
    CHECK(qldpc_mc_weight_frames_host(K, N, NULL, cls_in, 0x1234567ull, parity_ber, first, n, NULL, key_bits, info, NULL) == QLDPC_OK);
    CHECK(qldpc_mc_weight_frames_host(K, N, NULL, cls_in, 0x1234567ull, parity_ber, first, n, weights, key_bits, NULL, flips) == QLDPC_OK);
    CHECK(memcmp(prev, flips, sizeof(uint32_t) * (size_t)n * (size_t)Wn) == 0);
    free(cls); free(info); free(flips); free(prev); free(weights);
    return 0;
}

int main(void)
{
    int cases = 0;
    uint8_t mixed[131];
    for (int v = 0; v < 131; v++) mixed[v] = (uint8_t)((v * 7 + v / 5) % 3);
    const int kbs[] = {0, 32, 9, 8, 4, 1};
    for (unsigned i = 0; i < sizeof(kbs) / sizeof(kbs[0]); i++, cases += 6) {
        if (shape(20, 33, NULL, 0, 3, kbs[i], 0.0) || shape(33, 33, NULL, 4294967294ull, 4, kbs[i], 0.0) || shape(1, 1, NULL, 0, 2, kbs[i], 0.0)) return 1;
        if (shape(40, 131, mixed, 4294967295ull, 3, kbs[i], 0.25) || shape(64, 64, NULL, 7, 2, kbs[i], 0.0) || shape(5, 1030, NULL, 0, 2, kbs[i], 0.5)) return 1;
    }
    /* refused arguments: nothing is written */
    uint32_t info[2] = {0xA5A5A5A5u, 0xA5A5A5A5u}, flips[4] = {0xA5A5A5A5u, 0xA5A5A5A5u, 0xA5A5A5A5u, 0xA5A5A5A5u};
    int w2[2] = {3, 21};
    CHECK(qldpc_mc_weight_frames_host(20, 33, NULL, NULL, 1, 0.0, 0, 2, w2, 0, info, flips) == QLDPC_ESIZE);
    CHECK(strstr(qldpc_last_error(), "weights[1]=21") != NULL);
    w2[1] = -1;
    CHECK(qldpc_mc_weight_frames_host(20, 33, NULL, NULL, 1, 0.0, 0, 2, w2, 0, info, flips) == QLDPC_ESIZE);
    w2[1] = 20;
    CHECK(qldpc_mc_weight_frames_host(20, 33, NULL, NULL, 1, 0.0, 0, 2, w2, 33, info, flips) == QLDPC_ESIZE);
    CHECK(qldpc_mc_weight_frames_host(20, 33, NULL, NULL, 1, 0.0, 0, 2, w2, -1, info, flips) == QLDPC_ESIZE);
    CHECK(qldpc_mc_weight_frames_host(20, 33, NULL, NULL, 1, 1.0, 0, 2, w2, 0, info, flips) == QLDPC_ESIZE);
    CHECK(qldpc_mc_weight_frames_host(34, 33, NULL, NULL, 1, 0.0, 0, 2, w2, 0, info, flips) == QLDPC_ESIZE);
    CHECK(qldpc_mc_weight_frames_host(20, 33, NULL, NULL, 1, 0.0, 0, 2, NULL, 0, info, flips) == QLDPC_EINVAL);
    CHECK(qldpc_mc_weight_frames_host(20, 33, NULL, NULL, 1, 0.0, 0, -1, w2, 0, info, flips) == QLDPC_EINVAL);
    CHECK(qldpc_mc_weight_frames_host(20, 33, NULL, NULL, 1, 0.0, 0, 2, w2, 0, NULL, NULL) == QLDPC_EINVAL);
    const int bad_pos[2] = {5, 5};
    CHECK(qldpc_mc_weight_frames_host(2, 33, bad_pos, NULL, 1, 0.0, 0, 2, w2, 0, info, flips) == QLDPC_EINVAL);
    CHECK(info[0] == 0xA5A5A5A5u && info[1] == 0xA5A5A5A5u && flips[0] == 0xA5A5A5A5u && flips[3] == 0xA5A5A5A5u);
    CHECK(qldpc_mc_weight_frames_host(20, 33, NULL, NULL, 1, 0.0, 0, 0, NULL, 0, info, flips) == QLDPC_OK);      /* no frames */
    cases += 12;

    /* the estimate: arrays of exactly n_strata entries */
    double out[4];
    for (int n = 1; n <= 600; n += 37, cases++) {
        int *w = malloc(sizeof(int) * (size_t)(n + 1));
        uint64_t *fr = malloc(sizeof(uint64_t) * (size_t)(n + 1)), *fe = malloc(sizeof(uint64_t) * (size_t)(n + 1));
        for (int s = 0; s <= n; s++) { w[s] = s; fr[s] = 7; fe[s] = 7; }
        CHECK(qldpc_mc_strata_fer_host(n, n + 1, w, fr, fe, 0.11, out) == QLDPC_OK);
        CHECK(fabs(out[0] - 1.0) < 1e-12 && out[1] == 0.0 && out[2] == 0.0 && out[3] == 0.0);
        CHECK(qldpc_mc_strata_fer_host(n, 1, w + n / 2, fr, fe, 0.11, out) == QLDPC_OK);      /* a single stratum: the rest is in the tails */
        CHECK(fabs(out[0] + out[1] + out[2] - 1.0) < 1e-12);
        int strided = 0;
        for (int s = 0; s <= n; s += 5) { w[strided] = s; fe[strided] = (uint64_t)(s % 8); strided++; }
        CHECK(qldpc_mc_strata_fer_host(n, strided, w, fr, fe, 0.4, out) == QLDPC_OK);
        CHECK(out[0] >= 0.0 && out[0] <= 1.0 && out[1] == 0.0 && out[2] >= 0.0 && out[3] >= 0.0);
        free(w); free(fr); free(fe);
    }
    const int w3[3] = {3, 5, 9}, w3_eq[3] = {3, 3, 9}, w3_hi[3] = {3, 5, 101};
    const uint64_t f3[3] = {10, 10, 10}, e3[3] = {0, 5, 10}, f3_zero[3] = {10, 0, 10}, e3_over[3] = {0, 11, 10};
    out[0] = -7.0;
    CHECK(qldpc_mc_strata_fer_host(100, 3, w3_hi, f3, e3, 0.05, out) == QLDPC_ESIZE);
    CHECK(qldpc_mc_strata_fer_host(100, 0, w3, f3, e3, 0.05, out) == QLDPC_ESIZE);
    CHECK(qldpc_mc_strata_fer_host(100, QLDPC_MC_SWEEP_MAX_POINTS + 1, w3, f3, e3, 0.05, out) == QLDPC_ESIZE);
    CHECK(qldpc_mc_strata_fer_host(0, 3, w3, f3, e3, 0.05, out) == QLDPC_ESIZE);
    CHECK(qldpc_mc_strata_fer_host(100, 3, w3, f3_zero, e3, 0.05, out) == QLDPC_ESIZE);
    CHECK(qldpc_mc_strata_fer_host(100, 3, w3, f3, e3_over, 0.05, out) == QLDPC_ESIZE);
    CHECK(qldpc_mc_strata_fer_host(100, 3, w3, f3, e3, 0.0, out) == QLDPC_ESIZE);
    CHECK(qldpc_mc_strata_fer_host(100, 3, w3, f3, e3, 1.0, out) == QLDPC_ESIZE);
    CHECK(qldpc_mc_strata_fer_host(100, 3, w3_eq, f3, e3, 0.05, out) == QLDPC_EINVAL);
    CHECK(qldpc_mc_strata_fer_host(100, 3, NULL, f3, e3, 0.05, out) == QLDPC_EINVAL);
    CHECK(qldpc_mc_strata_fer_host(100, 3, w3, NULL, e3, 0.05, out) == QLDPC_EINVAL);
    CHECK(qldpc_mc_strata_fer_host(100, 3, w3, f3, NULL, 0.05, out) == QLDPC_EINVAL);
    CHECK(qldpc_mc_strata_fer_host(100, 3, w3, f3, e3, 0.05, NULL) == QLDPC_EINVAL);
    CHECK(out[0] == -7.0);
    CHECK(qldpc_mc_strata_fer_host(100, 3, w3, f3, e3, 0.05, out) == QLDPC_OK && out[0] > 0.0 && out[3] > 0.0);
    cases += 14;
    printf("sanitizer pass ok: %d cases\n", cases);
    return 0;
}
