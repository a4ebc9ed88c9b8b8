/* Sanitizer pass over the host side of the genie-aided polar code construction (qldpc_polar_tally_host.c on qldpc_polar_tally_core.h, no HIP):
 * the tally's mirror at every size up to 2^11 in both message types with every array malloc'ed at its stated size, against the leaf beliefs of a
 * K = 0 qldpc_polar_decode_host, a second call adding up, and the two helpers with and without a prior, with all scores equal and with their
 * refusals.  Built with -fsanitize=address,undefined by tests/test_polar_construct.py */
#include "qldpc.h"
#include "qldpc_polar_tally_core.h"

#include "polar_sanitize_common.h"

static int run(int n, int f32, int maxq, int F)
{
    const long N = 1l << n, W = pl_words(n);
    const size_t esz = f32 ? sizeof(float) : 1, beliefs = esz * (size_t)(F * N);
    const int kind = f32 ? QLDPC_POLAR_F32 : QLDPC_POLAR_I8;
    void *llr = malloc(beliefs), *leaf = malloc(beliefs);
    uint32_t *u = (uint32_t *)malloc(4 * (size_t)(F * W));
    uint64_t *tally = (uint64_t *)calloc(2 * (size_t)N, 8), *want = (uint64_t *)calloc(2 * (size_t)N, 8);
    int *order = (int *)malloc(sizeof(int) * (size_t)N), *order2 = (int *)malloc(sizeof(int) * (size_t)N), *prior = draw_info_pos(N, (int)N);
    fill_llr(llr, F * N, f32, 3, 1.0f);                           /* small integers: ties everywhere */
    for (long i = 0; i < F * W; i++) u[i] = (uint32_t)rnd() & pl_row_mask(n);
    CHECK(qldpc_polar_decode_host(n, 0, NULL, kind, maxq, F, llr, u, NULL, NULL, NULL, leaf) == QLDPC_OK);
    for (long f = 0; f < F; f++)
        for (long p = 0; p < N; p++) {
            const double L = f32 ? (double)((float *)leaf)[f * N + p] : (double)((int8_t *)leaf)[f * N + p];
            want[p] += L != 0.0 && (L < 0.0) != get(u + f * W, p);
            want[N + p] += L == 0.0;
        }
    CHECK(qldpc_polar_tally_host(n, kind, maxq, F, llr, u, tally) == QLDPC_OK);
    CHECK(!memcmp(tally, want, 16 * (size_t)N));
    /* two calls add up: the first F / 2 frames, then the rest, on top of the whole */
    const long h = F / 2;
    CHECK(qldpc_polar_tally_host(n, kind, maxq, (int)h, llr, u, tally) == QLDPC_OK);
    CHECK(qldpc_polar_tally_host(n, kind, maxq, (int)(F - h), (char *)llr + esz * (size_t)(h * N), u + h * W, tally) == QLDPC_OK);
    for (long i = 0; i < 2 * N; i++) CHECK(tally[i] == 2 * want[i]);
    CHECK(qldpc_polar_tally_host(n, kind, maxq, 0, NULL, NULL, NULL) == QLDPC_OK);
    /* the order: a permutation, scores descending, ties by the prior's rank; the K of a bound */
    int *rank = (int *)malloc(sizeof(int) * (size_t)N);
    for (long r = 0; r < N; r++) rank[prior[r]] = (int)r;
    CHECK(qldpc_polar_construct_order_host(n, want, prior, order) == QLDPC_OK);
    CHECK(qldpc_polar_construct_order_host(n, want, NULL, order2) == QLDPC_OK);
    uint64_t total = 0;
    for (long r = 0; r < N; r++) total += plt_score(want[order[r]], want[N + order[r]]);
    for (long r = 0; r + 1 < N; r++) {
        const uint64_t a = plt_score(want[order[r]], want[N + order[r]]), b = plt_score(want[order[r + 1]], want[N + order[r + 1]]);
        const uint64_t a2 = plt_score(want[order2[r]], want[N + order2[r]]), b2 = plt_score(want[order2[r + 1]], want[N + order2[r + 1]]);
        CHECK(a > b || (a == b && rank[order[r]] < rank[order[r + 1]]));
        CHECK(a2 > b2 || (a2 == b2 && order2[r] < order2[r + 1]));
    }
    int k = -1;
    CHECK(qldpc_polar_construct_k_host(n, want, order, total, &k) == QLDPC_OK && k == N);
    CHECK(qldpc_polar_construct_k_host(n, want, order, 0, &k) == QLDPC_OK && k >= 0 && k <= N);
    for (long r = N - k; r < N; r++) CHECK(plt_score(want[order[r]], want[N + order[r]]) == 0);
    CHECK(k == N || plt_score(want[order[N - 1 - k]], want[N + order[N - 1 - k]]) > 0);
    /* all scores equal: the prior itself */
    for (long i = 0; i < 2 * N; i++) want[i] = 7;
    CHECK(qldpc_polar_construct_order_host(n, want, prior, order) == QLDPC_OK && !memcmp(order, prior, sizeof(int) * (size_t)N));
    CHECK(qldpc_polar_construct_k_host(n, want, order, 21 * 3 + 20, &k) == QLDPC_OK && k == (N < 3 ? N : 3));
    free(llr); free(leaf); free(u); free(tally); free(want); free(order); free(order2); free(prior); free(rank);
    return 0;
}

int main(void)
{
    for (int n = 1; n <= 11; n++) {
        if (run(n, 0, 1, 70) || run(n, 0, 31, 5) || run(n, 1, 0, 67)) return 1;
    }
    /* refusals */
    int8_t z[128] = {0};
    uint32_t row[4] = {0};
    uint64_t t[256] = {0};
    int order[128], k = 0;
    for (int i = 0; i < 128; i++) order[i] = i;
    CHECK(qldpc_polar_tally_host(0, 0, 31, 1, z, row, t) == QLDPC_ESIZE);
    CHECK(qldpc_polar_tally_host(21, 0, 31, 1, z, row, t) == QLDPC_ESIZE);
    CHECK(qldpc_polar_tally_host(7, 0, 127, 1, z, row, t) == QLDPC_ESIZE && strstr(msg, "polar_tally_host"));
    CHECK(qldpc_polar_tally_host(7, 2, 31, 1, z, row, t) == QLDPC_EINVAL);
    CHECK(qldpc_polar_tally_host(7, 0, 31, -1, z, row, t) == QLDPC_EINVAL);
    CHECK(qldpc_polar_tally_host(7, 0, 31, 1, NULL, row, t) == QLDPC_EINVAL);
    CHECK(qldpc_polar_tally_host(7, 0, 31, 1, z, NULL, t) == QLDPC_EINVAL);
    CHECK(qldpc_polar_tally_host(7, 0, 31, 1, z, row, NULL) == QLDPC_EINVAL);
    CHECK(qldpc_polar_construct_order_host(0, t, NULL, order) == QLDPC_ESIZE && qldpc_polar_construct_order_host(21, t, NULL, order) == QLDPC_ESIZE);
    CHECK(qldpc_polar_construct_order_host(7, NULL, NULL, order) == QLDPC_EINVAL && qldpc_polar_construct_order_host(7, t, NULL, NULL) == QLDPC_EINVAL);
    CHECK(qldpc_polar_construct_k_host(0, t, order, 0, &k) == QLDPC_ESIZE);
    CHECK(qldpc_polar_construct_k_host(7, t, order, 0, NULL) == QLDPC_EINVAL && qldpc_polar_construct_k_host(7, t, NULL, 0, &k) == QLDPC_EINVAL);
    CHECK(qldpc_polar_construct_k_host(7, t, order, 0, &k) == QLDPC_OK && k == 128);
    order[5] = 6;                                                  /* 6 twice */
    CHECK(qldpc_polar_construct_order_host(7, t, order, order) == QLDPC_EINVAL && strstr(msg, "prior"));
    CHECK(qldpc_polar_construct_k_host(7, t, order, 0, &k) == QLDPC_EINVAL && strstr(msg, "order"));
    order[5] = 128;
    CHECK(qldpc_polar_construct_order_host(7, t, order, order) == QLDPC_EINVAL);
    order[5] = -1;
    CHECK(qldpc_polar_construct_k_host(7, t, order, 0, &k) == QLDPC_EINVAL);
    order[5] = 5;
    t[3] = PLT_MAX_COUNT;
    CHECK(qldpc_polar_construct_order_host(7, t, NULL, order) == QLDPC_OK);
    for (int i = 0; i < 128; i++) order[i] = i;
    t[128 + 9] = PLT_MAX_COUNT + 1;
    CHECK(qldpc_polar_construct_order_host(7, t, NULL, order) == QLDPC_ESIZE && strstr(msg, "2^40"));
    CHECK(qldpc_polar_construct_k_host(7, t, order, ~0ull, &k) == QLDPC_ESIZE);
    printf("polar tally: sanitizer pass ok\n");
    return 0;
}
