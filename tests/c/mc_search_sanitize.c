/* Sanitizer pass over the host side of the puncture-pattern definition (qldpc_mc_pattern_host in qldpc_mc_host.c over qldpc_mc_core.h, no
 * HIP): the radix select at the edge sizes into buffers of exactly n_punct entries, checked against a plain selection by repeated minimum,
 * the argument checks, and the list validation that qldpc_mc_set_candidates / qldpc_mc_set_puncture run before they touch the device.
 * Built with -fsanitize=address,undefined by tests/test_mc_search.py */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "qldpc.h"
#include "qldpc_mc_core.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

/* the definition, literally: take n_punct times the smallest (u', c) not taken yet */
static void by_minimum(uint64_t seed, uint64_t p, int n_cand, int n_punct, int key_bits, char *taken)
{
    uint32_t *u = malloc(sizeof(uint32_t) * (size_t)(n_cand + 4));
    for (int q = 0; 4 * q < n_cand; q++) mc_pattern_keys(seed, p, (uint32_t)q, key_bits, u + 4 * q);
    memset(taken, 0, (size_t)n_cand);
    for (int i = 0; i < n_punct; i++) {
        int best = -1;
        for (int c = 0; c < n_cand; c++)
            if (!taken[c] && (best < 0 || u[c] < u[best])) best = c;
        taken[best] = 1;
    }
    free(u);
}

int main(void)
{
    static const int n_cands[] = {1, 3, 4, 5, 63, 64, 65, 255, 257, 410, 1000};
    static const uint64_t patterns[] = {0, 1, 4294967295ull, 4294967296ull, 9223372036854775813ull /* 2^63 + 5 */};
    static const int key_bits[] = {32, 8, 3, 1};
    int cases = 0;
    for (size_t a = 0; a < sizeof(n_cands) / sizeof(*n_cands); a++)
        for (size_t b = 0; b < sizeof(patterns) / sizeof(*patterns); b++)
            for (size_t c = 0; c < sizeof(key_bits) / sizeof(*key_bits); c++) {
                const int n_cand = n_cands[a], punct[5] = {0, 1, n_cand / 3, n_cand - 1, n_cand};
                char *taken = malloc((size_t)n_cand);
                for (int k = 0; k < 5; k++) {
                    const int n_punct = punct[k];
                    int *idx = malloc(sizeof(int) * (size_t)(n_punct ? n_punct : 1));      /* exactly n_punct entries may be written */
                    CHECK(qldpc_mc_pattern_host(7, patterns[b], n_cand, n_punct, key_bits[c], n_punct ? idx : NULL) == QLDPC_OK);
                    by_minimum(7, patterns[b], n_cand, n_punct, key_bits[c], taken);
                    for (int i = 0; i < n_punct; i++) {
                        CHECK(idx[i] >= 0 && idx[i] < n_cand && (i == 0 || idx[i] > idx[i - 1]) && taken[idx[i]]);
                        taken[idx[i]] = 0;
                    }
                    for (int v = 0; v < n_cand; v++) CHECK(!taken[v]);
                    free(idx);
                    cases++;
                }
                free(taken);
            }
    /* argument checks: nothing is written */
    int idx[4] = {-7, -7, -7, -7};
    CHECK(qldpc_mc_pattern_host(7, 0, 4, 5, 32, idx) == QLDPC_ESIZE);
    CHECK(qldpc_mc_pattern_host(7, 0, 4, -1, 32, idx) == QLDPC_ESIZE);
    CHECK(qldpc_mc_pattern_host(7, 0, -1, 0, 32, idx) == QLDPC_ESIZE);
    CHECK(qldpc_mc_pattern_host(7, 0, 4, 2, 33, idx) == QLDPC_ESIZE);
    CHECK(qldpc_mc_pattern_host(7, 0, 4, 2, -1, idx) == QLDPC_ESIZE);
    CHECK(qldpc_mc_pattern_host(7, 0, 4, 2, 32, NULL) == QLDPC_EINVAL);
    CHECK(idx[0] == -7 && idx[1] == -7 && idx[2] == -7 && idx[3] == -7);
    CHECK(qldpc_mc_pattern_host(7, 0, 0, 0, 0, NULL) == QLDPC_OK);
    CHECK(strstr(qldpc_last_error(), "key_bits=-1") != NULL);

    /* the list validation of candidates and puncture sets, and the packed row of a good list */
    static const int Ns[] = {1, 31, 32, 33, 1008, 2000};
    for (size_t a = 0; a < sizeof(Ns) / sizeof(*Ns); a++) {
        const int N = Ns[a], Wn = (N + 31) / 32, n = (N + 2) / 3;
        int *vn = malloc(sizeof(int) * (size_t)n);
        uint32_t *row = malloc(4 * (size_t)Wn);
        for (int i = 0; i < n; i++) vn[i] = 3 * i;
        vn[n - 1] = N - 1;                                                        /* the last VN: the row's tail word */
        CHECK(mc_vn_list_check(vn, n, N) == -1 && mc_vn_list_check(NULL, 0, N) == -1);
        mc_vn_list_row(vn, n, N, row);
        int bits = 0;
        for (int w = 0; w < Wn; w++) bits += __builtin_popcount(row[w]);
        CHECK(bits == n && (row[(N - 1) >> 5] & (0x80000000u >> ((N - 1) & 31))) && (row[Wn - 1] & ~mc_tail_mask(N)) == 0);
        vn[n - 1] = N;
        CHECK(mc_vn_list_check(vn, n, N) == n - 1);
        vn[n - 1] = N - 1;
        vn[0] = -1;
        CHECK(mc_vn_list_check(vn, n, N) == 0);
        vn[0] = 0;
        if (n > 2) {
            vn[1] = vn[0];                                                        /* repeated */
            CHECK(mc_vn_list_check(vn, n, N) == 1);
            vn[1] = vn[2] + 1;                                                    /* descending */
            CHECK(mc_vn_list_check(vn, n, N) == 2);
        }
        free(vn); free(row);
        cases++;
    }
    printf("sanitizer pass ok: %d cases\n", cases);
    return 0;
}
