/* Sanitizer pass over the host side of the Monte-Carlo loop around the polar decoders (qldpc_polar_mc_host.c over qldpc_polar_mc_core.h, no HIP):
 * the mirror of its frames at sizes 2 .. 2^11 in both message types, with and without a CRC, both frozen and both source modes, tables of 2, 3, 64
 * and 256 levels, every array malloc'ed at its stated size, each output asked for alone and all together (which must agree), a range in one call
 * against the same range in two; the table builder in both roundings at the largest maxq of each; and the refusals.  Built with
 * -fsanitize=address,undefined by tests/test_polar_mc.py */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "qldpc.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd(void)
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}

/* a table of `levels` levels at exactly levels - 1 and levels entries: ascending rows with a run of equal thresholds, zeros in front and 2^32 at the
 * end where there is room; integer values */
static void make_table(int levels, uint64_t **c0, uint64_t **c1, float **v)
{
    uint64_t *c[2];
    for (int b = 0; b < 2; b++) {
        c[b] = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)(levels - 1));
        uint64_t at = 0;
        for (int k = 0; k < levels - 1; k++) {
            if (k >= 2 && k % 5 != 0) at += (4294967296ull - at) / (uint64_t)(levels - k) / 2u + (rnd() & 0xffu);
            c[b][k] = k >= levels - 3 && levels > 8 ? 4294967296ull : at;
        }
    }
    *v = (float *)malloc(sizeof(float) * (size_t)levels);
    for (int l = 0; l < levels; l++) (*v)[l] = (float)((int)(rnd() % 256u) - 128);
    *c0 = c[0]; *c1 = c[1];
}

static int run(int n, int f32, int n_info, int crc_len, uint32_t crc_poly, int frozen, int source, int levels)
{
    const long N = 1l << n, W = N <= 32 ? 1 : N / 32, Wi = (n_info + 31) / 32;
    const int F = 5, kind = f32 ? QLDPC_POLAR_F32 : QLDPC_POLAR_I8;
    const uint64_t seed = rnd(), first = (rnd() & 1u) ? 0xfffffffdull : rnd();
    int *pos = (int *)malloc(sizeof(int) * (size_t)(n_info ? n_info : 1)), *perm = (int *)malloc(sizeof(int) * (size_t)N);
    for (long i = 0; i < N; i++) perm[i] = (int)i;
    for (long i = N - 1; i > 0; i--) { const long j = (long)(rnd() % (uint64_t)(i + 1)); const int t = perm[i]; perm[i] = perm[j]; perm[j] = t; }
    for (int m = 0; m < n_info; m++) pos[m] = perm[m];
    free(perm);
    uint64_t *c0, *c1;
    float *v;
    make_table(levels, &c0, &c1, &v);
    const size_t esz = f32 ? sizeof(float) : 1, b_info = 4 * (size_t)(Wi ? F * Wi : 1), b_row = 4 * (size_t)(F * W), b_llr = esz * (size_t)(F * N), b_fl = 4 * (size_t)F;
    uint32_t *info = (uint32_t *)malloc(b_info), *u = (uint32_t *)malloc(b_row), *x = (uint32_t *)malloc(b_row), *fl = (uint32_t *)malloc(b_fl);
    uint32_t *info1 = (uint32_t *)malloc(b_info), *u1 = (uint32_t *)malloc(b_row), *x1 = (uint32_t *)malloc(b_row), *fl1 = (uint32_t *)malloc(b_fl);
    void *llr = malloc(b_llr), *llr1 = malloc(b_llr);
#define FRAMES(FIRST, COUNT, I, U, X, L, FL) \
    qldpc_polar_mc_frames_host(n, n_info, n_info ? pos : NULL, kind, crc_len, crc_poly, frozen, source, seed, levels, c0, c1, v, FIRST, COUNT, I, U, X, L, FL)
    CHECK(FRAMES(first, F, info, u, x, llr, fl) == QLDPC_OK);
    /* each output alone */
    CHECK(FRAMES(first, F, info1, NULL, NULL, NULL, NULL) == QLDPC_OK && (!Wi || !memcmp(info1, info, 4 * (size_t)(F * Wi))));
    CHECK(FRAMES(first, F, NULL, u1, NULL, NULL, NULL) == QLDPC_OK && !memcmp(u1, u, b_row));
    CHECK(FRAMES(first, F, NULL, NULL, x1, NULL, NULL) == QLDPC_OK && !memcmp(x1, x, b_row));
    CHECK(FRAMES(first, F, NULL, NULL, NULL, llr1, NULL) == QLDPC_OK && !memcmp(llr1, llr, b_llr));
    CHECK(FRAMES(first, F, NULL, NULL, NULL, NULL, fl1) == QLDPC_OK && !memcmp(fl1, fl, b_fl));
    CHECK(FRAMES(first, F, NULL, NULL, NULL, NULL, NULL) == QLDPC_OK);
    /* the range in two calls */
    CHECK(FRAMES(first, 2, info1, u1, x1, llr1, fl1) == QLDPC_OK);
    CHECK(FRAMES(first + 2, F - 2, info1 + 2 * Wi, u1 + 2 * W, x1 + 2 * W, (char *)llr1 + esz * (size_t)(2 * N), fl1 + 2) == QLDPC_OK);
    CHECK((!Wi || !memcmp(info1, info, 4 * (size_t)(F * Wi))) && !memcmp(u1, u, b_row) && !memcmp(x1, x, b_row) && !memcmp(llr1, llr, b_llr) && !memcmp(fl1, fl, b_fl));
    /* without a table: the rows, and neither llr nor flips */
    CHECK(qldpc_polar_mc_frames_host(n, n_info, n_info ? pos : NULL, kind, crc_len, crc_poly, frozen, source, seed, 0, NULL, NULL, NULL, first, F, NULL, u1, x1, NULL, NULL) == QLDPC_OK);
    CHECK(!memcmp(u1, u, b_row) && !memcmp(x1, x, b_row));
    CHECK(qldpc_polar_mc_frames_host(n, n_info, n_info ? pos : NULL, kind, crc_len, crc_poly, frozen, source, seed, 0, NULL, NULL, NULL, first, F, NULL, NULL, NULL, llr1, NULL) == QLDPC_ESTATE);
#undef FRAMES
    /* the frozen positions of u are zero in the zero mode, and the bits past N of a short row */
    if (frozen == QLDPC_POLAR_MC_FROZEN_ZERO && n_info == 0)
        for (long i = 0; i < F * W; i++) CHECK(u[i] == 0u && x[i] == 0u);
    if (N < 32)
        for (long i = 0; i < F; i++) CHECK(!(u[i] & (0xffffffffu >> N)) && !(x[i] & (0xffffffffu >> N)));
    free(pos); free(c0); free(c1); free(v); free(info); free(u); free(x); free(fl); free(info1); free(u1); free(x1); free(fl1); free(llr); free(llr1);
    return 0;
}

int main(void)
{
    static const int levels[4] = {2, 3, 64, 256};
    int t = 0;
    for (int n = 1; n <= 11; n++) {
        const long N = 1l << n;
        const int ks[5] = {0, (int)N, (int)(N / 2 + 1 > N ? N : N / 2 + 1), 16, 40};
        for (int k = 0; k < 5; k++) {
            if (ks[k] > N) continue;
            for (int c = 0; c < 3; c++) {
                const int crc_len = c == 0 ? 0 : (c == 1 ? 11 : 32);
                if (crc_len > ks[k]) continue;
                for (int f32 = 0; f32 < 2; f32++, t++)
                    if (run(n, f32, ks[k], crc_len, c == 1 ? 0x621u : (c == 2 ? 0x04C11DB7u : 0u), t & 1, (t >> 1) % 3 == 0, levels[t % 4])) return 1;
            }
        }
    }
    /* the table builder: both roundings at their largest maxq, arrays at exactly the level count */
    {
        uint64_t *c0 = (uint64_t *)malloc(sizeof(uint64_t) * 255), *c1 = (uint64_t *)malloc(sizeof(uint64_t) * 255), *d0 = (uint64_t *)malloc(sizeof(uint64_t) * 255),
                 *d1 = (uint64_t *)malloc(sizeof(uint64_t) * 255);
        float *v = (float *)malloc(sizeof(float) * 256), *w = (float *)malloc(sizeof(float) * 256);
        CHECK(qldpc_polar_mc_awgn_table(0.8, 4.0, 127, 0, c0, c1, v) == 256);
        CHECK(qldpc_mc_awgn_table(0.8, 4.0, 127, d0, d1, w) == QLDPC_OK && !memcmp(c0, d0, 8 * 255) && !memcmp(c1, d1, 8 * 255) && !memcmp(v, w, 4 * 256));
        CHECK(qldpc_polar_mc_awgn_table(0.8, 4.0, 127, 1, c0, c1, v) == 255 && v[0] == -127.0f && v[254] == 127.0f);
        for (int k = 1; k < 254; k++) CHECK(c0[k] >= c0[k - 1] && c1[k] >= c1[k - 1] && c1[k] >= c0[k]);
        CHECK(qldpc_polar_mc_awgn_table(0.8, 4.0, 128, 1, c0, c1, v) == QLDPC_ESIZE);
        CHECK(qldpc_polar_mc_awgn_table(0.8, 4.0, 128, 0, c0, c1, v) == QLDPC_ESIZE);
        CHECK(qldpc_polar_mc_awgn_table(0.0, 4.0, 31, 1, c0, c1, v) == QLDPC_ESIZE);
        CHECK(qldpc_polar_mc_awgn_table(0.8, 4.0, 31, 2, c0, c1, v) == QLDPC_EINVAL);
        CHECK(qldpc_polar_mc_awgn_table(0.8, 4.0, 31, 1, NULL, c1, v) == QLDPC_EINVAL);
        free(c0); free(c1); free(d0); free(d1); free(v); free(w);
    }
    /* refusals of the mirror */
    {
        const uint64_t c0[1] = {1u << 31}, c1[1] = {1u << 30}, bad[2] = {5, 4}, big[1] = {4294967297ull};
        const float v[3] = {3.0f, -3.0f, 0.5f}, out_of_range[2] = {128.0f, 0.0f};
        int p2[2] = {1, 1}, p1[1] = {3};
        uint32_t row[4];
        int8_t l8[8];
        CHECK(qldpc_polar_mc_frames_host(0, 0, NULL, 0, 0, 0, 0, 0, 1, 2, c0, c1, v, 0, 1, row, NULL, NULL, NULL, NULL) == QLDPC_ESIZE);
        CHECK(qldpc_polar_mc_frames_host(21, 0, NULL, 0, 0, 0, 0, 0, 1, 2, c0, c1, v, 0, 1, row, NULL, NULL, NULL, NULL) == QLDPC_ESIZE);
        CHECK(qldpc_polar_mc_frames_host(3, 0, NULL, 2, 0, 0, 0, 0, 1, 2, c0, c1, v, 0, 1, row, NULL, NULL, NULL, NULL) == QLDPC_EINVAL);
        CHECK(qldpc_polar_mc_frames_host(3, 0, NULL, 0, 0, 0, 2, 0, 1, 2, c0, c1, v, 0, 1, row, NULL, NULL, NULL, NULL) == QLDPC_EINVAL);
        CHECK(qldpc_polar_mc_frames_host(3, 0, NULL, 0, 0, 0, 0, 2, 1, 2, c0, c1, v, 0, 1, row, NULL, NULL, NULL, NULL) == QLDPC_EINVAL);
        CHECK(qldpc_polar_mc_frames_host(3, 0, NULL, 0, 0, 0, 0, 0, 1, 2, c0, c1, v, 0, -1, row, NULL, NULL, NULL, NULL) == QLDPC_EINVAL);
        CHECK(qldpc_polar_mc_frames_host(3, 2, p2, 0, 0, 0, 0, 0, 1, 2, c0, c1, v, 0, 1, row, NULL, NULL, NULL, NULL) == QLDPC_EINVAL);
        CHECK(qldpc_polar_mc_frames_host(3, 1, NULL, 0, 0, 0, 0, 0, 1, 2, c0, c1, v, 0, 1, row, NULL, NULL, NULL, NULL) == QLDPC_ESIZE);
        CHECK(qldpc_polar_mc_frames_host(3, 1, p1, 0, 2, 1, 0, 0, 1, 2, c0, c1, v, 0, 1, row, NULL, NULL, NULL, NULL) == QLDPC_ESIZE);      /* crc_len > n_info */
        CHECK(qldpc_polar_mc_frames_host(3, 1, p1, 0, 1, 2, 0, 0, 1, 2, c0, c1, v, 0, 1, row, NULL, NULL, NULL, NULL) == QLDPC_ESIZE);      /* a coefficient past crc_len */
        CHECK(qldpc_polar_mc_frames_host(3, 1, p1, 0, 0, 0, 0, 0, 1, 1, c0, c1, v, 0, 1, NULL, NULL, NULL, l8, NULL) == QLDPC_ESIZE);
        CHECK(qldpc_polar_mc_frames_host(3, 1, p1, 0, 0, 0, 0, 0, 1, 257, c0, c1, v, 0, 1, NULL, NULL, NULL, l8, NULL) == QLDPC_ESIZE);
        CHECK(qldpc_polar_mc_frames_host(3, 1, p1, 0, 0, 0, 0, 0, 1, 2, NULL, c1, v, 0, 1, NULL, NULL, NULL, l8, NULL) == QLDPC_EINVAL);
        CHECK(qldpc_polar_mc_frames_host(3, 1, p1, 0, 0, 0, 0, 0, 1, 3, bad, bad, v, 0, 1, NULL, NULL, NULL, l8, NULL) == QLDPC_EINVAL);
        CHECK(qldpc_polar_mc_frames_host(3, 1, p1, 0, 0, 0, 0, 0, 1, 2, big, c1, v, 0, 1, NULL, NULL, NULL, l8, NULL) == QLDPC_EINVAL);
        CHECK(qldpc_polar_mc_frames_host(3, 1, p1, 0, 0, 0, 0, 0, 1, 2, c0, c1, v + 1, 0, 1, NULL, NULL, NULL, l8, NULL) == QLDPC_EINVAL);   /* 0.5 is no int8 */
        CHECK(qldpc_polar_mc_frames_host(3, 1, p1, 0, 0, 0, 0, 0, 1, 2, c0, c1, out_of_range, 0, 1, NULL, NULL, NULL, l8, NULL) == QLDPC_EINVAL);
        CHECK(qldpc_polar_mc_frames_host(3, 1, p1, 0, 0, 0, 0, 0, 1, 2, c0, c1, v, 0, 1, NULL, NULL, NULL, l8, NULL) == QLDPC_OK);
        CHECK(qldpc_polar_mc_frames_host(3, 1, p1, 0, 0, 0, 0, 0, 1, 2, c0, c1, v, 0, 0, NULL, NULL, NULL, NULL, NULL) == QLDPC_OK);
        CHECK(strlen(qldpc_last_error()) > 0);
    }
    printf("polar mc: sanitizer pass ok\n");
    return 0;
}
