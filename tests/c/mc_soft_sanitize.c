/* Sanitizer pass over the host side of the quantised soft-output channel (qldpc_mc_llr_host and qldpc_mc_awgn_table of qldpc_mc_host.c over
 * qldpc_mc_core.h, no HIP): the mirror at the edge sizes into buffers of exactly the size the call may write, the table shapes at their limits
 * (Q = 2, Q = 256, rows of zeros and of 2^32), ranges against their parts, and every argument check.
 * Built with -fsanitize=address,undefined by tests/test_mc_soft.py */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "qldpc.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)
#define TWO32 4294967296ull

int main(void)
{
    /* the table builder: exact sizes (Q - 1, Q - 1, Q), monotone rows inside [0, 2^32] */
    static const struct { double sigma, rmax; int maxq; } awgn[] = {{0.8414, 3.0, 31}, {1.0, 3.0, 31}, {0.05, 3.0, 127}, {5.0, 0.5, 1}, {1e-3, 3.0, 4}, {1e6, 3.0, 4}};
    for (size_t a = 0; a < sizeof(awgn) / sizeof(*awgn); a++) {
        const int Q = 2 * awgn[a].maxq + 2;
        uint64_t *c0 = malloc(sizeof(uint64_t) * (size_t)(Q - 1)), *c1 = malloc(sizeof(uint64_t) * (size_t)(Q - 1));
        float *val = malloc(sizeof(float) * (size_t)Q);
        CHECK(qldpc_mc_awgn_table(awgn[a].sigma, awgn[a].rmax, awgn[a].maxq, c0, c1, val) == QLDPC_OK);
        for (int k = 0; k < Q - 1; k++) {
            CHECK(c0[k] <= TWO32 && c1[k] <= TWO32 && c0[k] <= c1[k]);
            if (k) CHECK(c0[k] >= c0[k - 1] && c1[k] >= c1[k - 1]);
        }
        for (int l = 0; l < Q; l++) CHECK(val[l] == (float)(l - awgn[a].maxq - 1));
        free(c0); free(c1); free(val);
    }
    {
        uint64_t c[3]; float v[4];
        CHECK(qldpc_mc_awgn_table(0.0, 3.0, 1, c, c, v) == QLDPC_ESIZE && qldpc_mc_awgn_table(NAN, 3.0, 1, c, c, v) == QLDPC_ESIZE);
        CHECK(qldpc_mc_awgn_table(INFINITY, 3.0, 1, c, c, v) == QLDPC_ESIZE && qldpc_mc_awgn_table(1.0, -3.0, 1, c, c, v) == QLDPC_ESIZE);
        CHECK(qldpc_mc_awgn_table(1.0, 3.0, 0, c, c, v) == QLDPC_ESIZE && qldpc_mc_awgn_table(1.0, 3.0, 128, c, c, v) == QLDPC_ESIZE);
        CHECK(qldpc_mc_awgn_table(1.0, 3.0, 1, NULL, c, v) == QLDPC_EINVAL && qldpc_mc_awgn_table(1.0, 3.0, 1, c, c, NULL) == QLDPC_EINVAL);
    }

    static const int sizes[][2] = {{1, 1}, {1, 3}, {2, 4}, {3, 5}, {31, 33}, {32, 64}, {33, 65}, {504, 1008}, {1776, 1998}};
    static const uint64_t firsts[] = {0, 4294967196ull /* 2^32 - 100 */, 18446744073709551615ull /* wraps */};
    static const int levels[] = {2, 3, 64, 256};
    int cases = 0;
    for (size_t s = 0; s < sizeof(sizes) / sizeof(*sizes); s++)
        for (size_t a = 0; a < sizeof(firsts) / sizeof(*firsts); a++)
            for (size_t q = 0; q < sizeof(levels) / sizeof(*levels); q++) {
                const int K = sizes[s][0], N = sizes[s][1], Wn = (N + 31) / 32, n = 5, Q = levels[q];
                const uint64_t first = firsts[a];
                uint64_t *c0 = malloc(sizeof(uint64_t) * (size_t)(Q - 1)), *c1 = malloc(sizeof(uint64_t) * (size_t)(Q - 1));
                float *val = malloc(sizeof(float) * (size_t)Q);
                for (int k = 0; k < Q - 1; k++) {      /* a row that starts with zeros, repeats entries and ends with 2^32 */
                    c0[k] = k < 2 && Q > 4 ? 0 : (k >= Q - 3 && Q > 4 ? TWO32 : (uint64_t)((k / 2 * 2 + 1)) * (TWO32 / (uint64_t)Q));
                    c1[k] = c0[k] / 2 + (c0[k] == TWO32 ? TWO32 / 2 : 0);
                }
                for (int l = 0; l < Q; l++) val[l] = (float)(l - Q / 2);
                const qldpc_mc_channel t = {Q, {c0, c1}, val, {0, 0}};
                uint8_t *cls = malloc((size_t)N);
                for (int v = 0; v < N; v++) cls[v] = (uint8_t)(v % 3);
                uint32_t *cw = malloc(4 * (size_t)n * Wn), *flips = malloc(4 * (size_t)n * Wn), *part_f = malloc(4 * (size_t)n * Wn);
                float *llr = malloc(sizeof(float) * (size_t)n * N), *part_l = malloc(sizeof(float) * (size_t)n * N);
                for (int i = 0; i < n * Wn; i++) cw[i] = 0x9e3779b9u * (uint32_t)(i + 1);
                CHECK(qldpc_mc_llr_host(K, N, NULL, NULL, 7, 0.0, &t, cw, first, n, llr, flips) == QLDPC_OK);
                /* a range equals its parts, and either output alone */
                CHECK(qldpc_mc_llr_host(K, N, NULL, NULL, 7, 0.0, &t, cw, first, 2, part_l, part_f) == QLDPC_OK);
                CHECK(qldpc_mc_llr_host(K, N, NULL, NULL, 7, 0.0, &t, cw + 2 * Wn, first + 2, 3, part_l + 2 * N, NULL) == QLDPC_OK);
                CHECK(qldpc_mc_llr_host(K, N, NULL, NULL, 7, 0.0, &t, cw + 2 * Wn, first + 2, 3, NULL, part_f + 2 * Wn) == QLDPC_OK);
                CHECK(!memcmp(llr, part_l, sizeof(float) * (size_t)n * N) && !memcmp(flips, part_f, 4 * (size_t)n * Wn));
                for (int f = 0; f < n; f++) {
                    if (N % 32) CHECK((flips[(size_t)f * Wn + Wn - 1] & ((1u << (32 - N % 32)) - 1u)) == 0);
                    for (int v = 0; v < N; v++) {
                        const float l = llr[(size_t)f * N + v];
                        const int b = (cw[(size_t)f * Wn + v / 32] >> (31 - v % 32)) & 1, fl = (flips[(size_t)f * Wn + v / 32] >> (31 - v % 32)) & 1;
                        if (v < K) CHECK(l >= (float)(-Q / 2) && l <= (float)(Q - 1 - Q / 2) && l == floorf(l));
                        else CHECK(l == (b ? -QLDPC_CONFIRMED_BIT_LLR : QLDPC_CONFIRMED_BIT_LLR));      /* pinned, parity_ber = 0 */
                        CHECK(fl == (b ? l > 0.0f : l < 0.0f));
                        if (v < K && Q > 4) CHECK(l >= (float)(2 - Q / 2) && l <= (float)(Q - 3 - Q / 2));      /* the levels nothing reaches */
                    }
                }
                /* a class map of its own with dirty parity, the all-zero codeword, n = 0 */
                CHECK(qldpc_mc_llr_host(K, N, NULL, cls, 7, 0.2, &t, NULL, first, n, llr, flips) == QLDPC_OK);
                for (int f = 0; f < n; f++)
                    for (int v = 2; v < N; v += 3) CHECK(llr[(size_t)f * N + v] == 0.0f && !(flips[(size_t)f * Wn + v / 32] & (0x80000000u >> (v % 32))));
                CHECK(qldpc_mc_llr_host(K, N, NULL, cls, 7, 0.2, &t, cw, first, 0, llr, flips) == QLDPC_OK);
                /* argument checks: nothing is written */
                memset(llr, 0x5a, sizeof(float) * (size_t)n * N);
                memcpy(part_l, llr, sizeof(float) * (size_t)n * N);
                qldpc_mc_channel bad = t;
                bad.levels = 1;
                CHECK(qldpc_mc_llr_host(K, N, NULL, NULL, 7, 0.0, &bad, cw, first, n, llr, flips) == QLDPC_ESIZE);
                bad.levels = 257;
                CHECK(qldpc_mc_llr_host(K, N, NULL, NULL, 7, 0.0, &bad, cw, first, n, llr, flips) == QLDPC_ESIZE);
                bad = t; bad.reserved[0] = 1;
                CHECK(qldpc_mc_llr_host(K, N, NULL, NULL, 7, 0.0, &bad, cw, first, n, llr, flips) == QLDPC_EINVAL);
                bad = t; bad.value = NULL;
                CHECK(qldpc_mc_llr_host(K, N, NULL, NULL, 7, 0.0, &bad, cw, first, n, llr, flips) == QLDPC_EINVAL);
                bad = t; bad.cum[1] = NULL;
                CHECK(qldpc_mc_llr_host(K, N, NULL, NULL, 7, 0.0, &bad, cw, first, n, llr, flips) == QLDPC_EINVAL);
                const uint64_t keep = c1[Q - 2];
                c1[Q - 2] = TWO32 + 1;
                CHECK(qldpc_mc_llr_host(K, N, NULL, NULL, 7, 0.0, &t, cw, first, n, llr, flips) == QLDPC_EINVAL);
                c1[Q - 2] = keep;
                if (Q > 2) {
                    const uint64_t k0 = c0[0];
                    c0[0] = c0[1] + 1;
                    CHECK(qldpc_mc_llr_host(K, N, NULL, NULL, 7, 0.0, &t, cw, first, n, llr, flips) == QLDPC_EINVAL);
                    c0[0] = k0;
                }
                CHECK(qldpc_mc_llr_host(K, N, NULL, NULL, 7, 1.0, &t, cw, first, n, llr, flips) == QLDPC_ESIZE);
                CHECK(qldpc_mc_llr_host(N + 1, N, NULL, NULL, 7, 0.0, &t, cw, first, n, llr, flips) == QLDPC_ESIZE);
                CHECK(qldpc_mc_llr_host(K, N, NULL, NULL, 7, 0.0, NULL, cw, first, n, llr, flips) == QLDPC_EINVAL);
                CHECK(qldpc_mc_llr_host(K, N, NULL, NULL, 7, 0.0, &t, cw, first, -1, llr, flips) == QLDPC_EINVAL);
                CHECK(qldpc_mc_llr_host(K, N, NULL, NULL, 7, 0.0, &t, cw, first, n, NULL, NULL) == QLDPC_EINVAL);
                cls[N - 1] = 3;
                CHECK(qldpc_mc_llr_host(K, N, NULL, cls, 7, 0.0, &t, cw, first, n, llr, flips) == QLDPC_EINVAL);
                CHECK(!memcmp(llr, part_l, sizeof(float) * (size_t)n * N));
                free(c0); free(c1); free(val); free(cls); free(cw); free(flips); free(part_f); free(llr); free(part_l);
                cases++;
            }
    printf("sanitizer pass ok: %d cases\n", cases);
    return 0;
}
