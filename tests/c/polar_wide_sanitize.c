/* Sanitizer pass over the host walk of the wide form's memory plan (qldpc_polar_wide_core.h, qldpc_polar_wide_host.c, no HIP): every size up to
 * 2^13 in both message types, every row malloc'ed at its exact size, each output asked for alone and all together, against the host mirror
 * (qldpc_polar_host.c) bit for bit.  The walk itself allocates the scratch, the LDS stand-in and the windows at exactly the sizes the core
 * header states, so an index outside the plan is an error here.  Built with -fsanitize=address,undefined by tests/test_polar_wide_host.py */
#include "qldpc.h"
#include "qldpc_polar_wide_core.h"

#include "polar_sanitize_common.h"

static int run(int n, int f32, int maxq, int n_info, int with_fval)
{
    const long N = 1l << n, W = pl_words(n), Wi = (n_info + 31) / 32;
    const int F = 3;
    int *pos = draw_info_pos(N, n_info);
    const size_t esz = f32 ? sizeof(float) : 1, rows = 4 * (size_t)(F * W), irow = 4 * (size_t)(Wi ? F * Wi : 1), beliefs = esz * (size_t)(F * N);
    void *llr = malloc(beliefs), *leaf = malloc(beliefs), *leaf_m = malloc(beliefs), *leaf1 = malloc(beliefs);
    uint32_t *fv = (uint32_t *)calloc((size_t)(F * W), 4), *u = (uint32_t *)malloc(rows), *x = (uint32_t *)malloc(rows), *info = (uint32_t *)malloc(irow),
             *u_m = (uint32_t *)malloc(rows), *x_m = (uint32_t *)malloc(rows), *info_m = (uint32_t *)malloc(irow), *u1 = (uint32_t *)malloc(rows),
             *x1 = (uint32_t *)malloc(rows), *info1 = (uint32_t *)malloc(irow);
    fill_llr(llr, F * N, f32, 1000, 64.0f);
    if (with_fval) for (long i = 0; i < F * W; i++) fv[i] = (uint32_t)rnd();
    const uint32_t *fz = with_fval ? fv : NULL;
    const int kind = f32 ? QLDPC_POLAR_F32 : QLDPC_POLAR_I8;
    CHECK(qldpc_polar_decode_host(n, n_info, pos, kind, maxq, F, llr, fz, u_m, info_m, x_m, leaf_m) == QLDPC_OK);
    /* all together */
    CHECK(qldpc_polar_decode_wide_host(n, n_info, pos, kind, maxq, F, llr, fz, u, info, x, leaf) == QLDPC_OK);
    CHECK(!memcmp(u, u_m, rows) && !memcmp(x, x_m, rows) && !memcmp(leaf, leaf_m, beliefs) && (!Wi || !memcmp(info, info_m, 4 * (size_t)(F * Wi))));
    /* each output alone, and none */
    CHECK(qldpc_polar_decode_wide_host(n, n_info, pos, kind, maxq, F, llr, fz, u1, NULL, NULL, NULL) == QLDPC_OK && !memcmp(u1, u_m, rows));
    CHECK(qldpc_polar_decode_wide_host(n, n_info, pos, kind, maxq, F, llr, fz, NULL, info1, NULL, NULL) == QLDPC_OK && (!Wi || !memcmp(info1, info_m, 4 * (size_t)(F * Wi))));
    CHECK(qldpc_polar_decode_wide_host(n, n_info, pos, kind, maxq, F, llr, fz, NULL, NULL, x1, NULL) == QLDPC_OK && !memcmp(x1, x_m, rows));
    CHECK(qldpc_polar_decode_wide_host(n, n_info, pos, kind, maxq, F, llr, fz, NULL, NULL, NULL, leaf1) == QLDPC_OK && !memcmp(leaf1, leaf_m, beliefs));
    CHECK(qldpc_polar_decode_wide_host(n, n_info, pos, kind, maxq, F, llr, fz, NULL, NULL, NULL, NULL) == QLDPC_OK);
    free(pos); free(llr); free(leaf); free(leaf_m); free(leaf1); free(fv); free(u); free(x); free(info); free(u_m); free(x_m); free(info_m);
    free(u1); free(x1); free(info1);
    return 0;
}

int main(void)
{
    for (int n = 1; n <= 13; n++) {
        const long N = 1l << n;
        const int ks[4] = {0, (int)N, (int)(N / 2), (int)(rnd() % (uint64_t)(N + 1))};
        for (int k = 0; k < 4; k++)
            for (int with = 0; with < 2; with++) {
                if (run(n, 0, n % 3 == 0 ? 1 : (n % 3 == 1 ? 31 : 126), ks[k], with)) return 1;
                if (run(n, 1, 0, ks[k], with)) return 1;
            }
    }
    /* the plan: a frame's scratch is below N elements, and the LDS levels and the four windows are inside the 160 KiB of a workgroup */
    for (int c = PLW_CHIP_MIN; c <= PLW_CHIP_MAX; c++)
        for (int n = PL_SUB_LOG + 1; n <= PL_MAX_LOG2N; n++) {
            CHECK(plw_scratch_elems(n, c) < ((size_t)1 << n));
            CHECK(sizeof(float) * plw_lds_elems(n, c) + 4 * sizeof(uint32_t) * PLW_WIN <= 160u * 1024u);
        }
    /* refusals: the mirror's */
    int8_t z[128] = {0};
    uint32_t row[4] = {0};
    int p2[2] = {1, 1}, p128[1] = {128};
    CHECK(qldpc_polar_decode_wide_host(0, 0, NULL, 0, 31, 1, z, NULL, row, NULL, NULL, NULL) == QLDPC_ESIZE);
    CHECK(qldpc_polar_decode_wide_host(21, 0, NULL, 0, 31, 1, z, NULL, row, NULL, NULL, NULL) == QLDPC_ESIZE);
    CHECK(qldpc_polar_decode_wide_host(7, 0, NULL, 0, 127, 1, z, NULL, row, NULL, NULL, NULL) == QLDPC_ESIZE && strstr(msg, "int8") && strstr(msg, "wide_host"));
    CHECK(qldpc_polar_decode_wide_host(7, 0, NULL, 2, 31, 1, z, NULL, row, NULL, NULL, NULL) == QLDPC_EINVAL);
    CHECK(qldpc_polar_decode_wide_host(7, 2, p2, 0, 31, 1, z, NULL, row, NULL, NULL, NULL) == QLDPC_EINVAL);
    CHECK(qldpc_polar_decode_wide_host(7, 1, p128, 0, 31, 1, z, NULL, row, NULL, NULL, NULL) == QLDPC_ESIZE);
    CHECK(qldpc_polar_decode_wide_host(7, 1, NULL, 0, 31, 1, z, NULL, row, NULL, NULL, NULL) == QLDPC_ESIZE);
    CHECK(qldpc_polar_decode_wide_host(7, 0, NULL, 0, 31, -1, z, NULL, row, NULL, NULL, NULL) == QLDPC_EINVAL);
    CHECK(qldpc_polar_decode_wide_host(7, 0, NULL, 0, 31, 1, NULL, NULL, row, NULL, NULL, NULL) == QLDPC_EINVAL);
    CHECK(qldpc_polar_decode_wide_host(7, 0, NULL, 0, 31, 0, NULL, NULL, NULL, NULL, NULL, NULL) == QLDPC_OK);
    printf("polar wide: sanitizer pass ok\n");
    return 0;
}
