/* Sanitizer pass over the polar list decoder on the host (qldpc_polar_list_core.h and the mirror of qldpc_polar_list_host.c, no HIP): every size up
 * to 2^9, every list size and both message types, every row malloc'ed at its exact size, each output asked for alone and all together, the picked
 * path against the list (x is its row, u = encode(x), info its bits, its CRC the expected one), list size 1 against the SC mirror, the CRC call
 * against the bit loop of its definition, and every refusal.
 * Built with -fsanitize=address,undefined by tests/test_polar_list_host.py */
#include <math.h>

#include "qldpc.h"
#include "qldpc_polar_list_core.h"

#include "polar_sanitize_common.h"


/* the CRC by its definition, a bit at a time over a row of unpacked bits */
static uint32_t crc_def(const unsigned char *bits, int n_bits, int crc_len, uint32_t poly)
{
    uint64_t r = 0;
    for (int m = 0; m < n_bits && crc_len; m++) {
        const unsigned top = (unsigned)((r >> (crc_len - 1)) & 1u) ^ bits[m];
        r = (r << 1) & ((1ull << crc_len) - 1ull);
        if (top) r ^= poly;
    }
    return (uint32_t)r;
}

static int run(int n, int f32, int maxq, int L, int n_info, int crc_len, uint32_t poly, int with_rows)
{
    const long N = 1l << n, W = pl_words(n), Wi = (n_info + 31) / 32;
    const int F = 3, kind = f32 ? QLDPC_POLAR_F32 : QLDPC_POLAR_I8;
    int *pos = draw_info_pos(N, n_info);
    const size_t esz = f32 ? sizeof(float) : 1, row = 4 * (size_t)(F * W);
    void *llr = malloc(esz * (size_t)(F * N));
    uint32_t *fv = (uint32_t *)malloc(row), *crc = (uint32_t *)malloc(4 * (size_t)F), *u = (uint32_t *)malloc(row), *x = (uint32_t *)malloc(row),
             *info = (uint32_t *)malloc(4 * (size_t)(Wi ? F * Wi : 1)), *lx = (uint32_t *)malloc(row * (size_t)L), *metric = (uint32_t *)malloc(4 * (size_t)(F * L)),
             *u1 = (uint32_t *)malloc(row), *x1 = (uint32_t *)malloc(row), *info1 = (uint32_t *)malloc(4 * (size_t)(Wi ? F * Wi : 1)),
             *lx1 = (uint32_t *)malloc(row * (size_t)L), *metric1 = (uint32_t *)malloc(4 * (size_t)(F * L)), *enc = (uint32_t *)malloc(row);
    int32_t *pick = (int32_t *)malloc(4 * (size_t)F), *pick1 = (int32_t *)malloc(4 * (size_t)F);
    unsigned char *ib = (unsigned char *)malloc((size_t)(n_info ? n_info : 1));
    fill_llr(llr, F * N, f32, 8, 4.0f);                           /* few float values: ties in the metrics */
    for (long i = 0; i < F * W; i++) fv[i] = (uint32_t)rnd();
    for (int f = 0; f < F; f++) crc[f] = (uint32_t)rnd() & pll_crc_mask(crc_len);
    const uint32_t *fvp = with_rows ? fv : NULL, *crcp = with_rows && crc_len ? crc : NULL;
#define DECODE(U, I, X, P, M, LX) qldpc_polar_list_decode_host(n, n_info, pos, kind, maxq, L, crc_len, poly, F, llr, fvp, crcp, U, I, X, P, M, LX)
    CHECK(DECODE(u, info, x, pick, metric, lx) == QLDPC_OK);
    /* each output alone, and none */
    CHECK(DECODE(u1, NULL, NULL, NULL, NULL, NULL) == QLDPC_OK && !memcmp(u, u1, row));
    CHECK(DECODE(NULL, info1, NULL, NULL, NULL, NULL) == QLDPC_OK && !memcmp(info, info1, 4 * (size_t)(F * Wi)));
    CHECK(DECODE(NULL, NULL, x1, NULL, NULL, NULL) == QLDPC_OK && !memcmp(x, x1, row));
    CHECK(DECODE(NULL, NULL, NULL, pick1, NULL, NULL) == QLDPC_OK && !memcmp(pick, pick1, 4 * (size_t)F));
    CHECK(DECODE(NULL, NULL, NULL, NULL, metric1, NULL) == QLDPC_OK && !memcmp(metric, metric1, 4 * (size_t)(F * L)));
    CHECK(DECODE(NULL, NULL, NULL, NULL, NULL, lx1) == QLDPC_OK && !memcmp(lx, lx1, row * (size_t)L));
    CHECK(DECODE(NULL, NULL, NULL, NULL, NULL, NULL) == QLDPC_OK);
    const int P = pll_final_paths(L, n_info);
    CHECK(qldpc_polar_encode_host(n, F, x, enc) == QLDPC_OK && !memcmp(enc, u, row));
    for (int f = 0; f < F; f++) {
        const int k = pick[f] < 0 ? 0 : pick[f];
        CHECK(pick[f] >= -1 && pick[f] < P);
        CHECK(!memcmp(x + f * W, lx + ((size_t)f * (size_t)L + (size_t)k) * (size_t)W, 4 * (size_t)W));
        for (int m = 0; m < n_info; m++) { ib[m] = (unsigned char)get(u + f * W, pos[m]); CHECK(get(info + f * Wi, m) == ib[m]); }
        const uint32_t want = crcp ? crc[f] : 0u;
        CHECK((crc_def(ib, n_info, crc_len, poly) == want) == (pick[f] >= 0));
        if (crc_len == 0) CHECK(pick[f] == 0);
        for (int s = 0; s < L; s++) {
            const uint32_t *r = lx + ((size_t)f * (size_t)L + (size_t)s) * (size_t)W;
            int any = 0;
            for (long w = 0; w < W; w++) any |= r[w] != 0u;
            if (s >= P) CHECK(!any && (f32 ? isinf(((float *)metric)[f * L + s]) : metric[f * L + s] == 0xffffffffu));
            else CHECK(f32 ? ((float *)metric)[f * L + s] >= 0.0f && !isinf(((float *)metric)[f * L + s]) : metric[f * L + s] <= (uint32_t)(N * (maxq + 1)));
        }
    }
    if (L == 1 && crc_len == 0) {                                 /* the SC decoder, bit for bit */
        CHECK(qldpc_polar_decode_host(n, n_info, pos, kind, maxq, F, llr, fvp, u1, info1, x1, NULL) == QLDPC_OK);
        CHECK(!memcmp(u, u1, row) && !memcmp(x, x1, row) && !memcmp(info, info1, 4 * (size_t)(F * Wi)));
    }
    /* Alice's call on the information rows: the remainder the pick looked for */
    if (n_info > 0) {
        CHECK(qldpc_polar_crc_host(crc_len, poly, n_info, F, info, crc) == QLDPC_OK);
        for (int f = 0; f < F; f++) {
            for (int m = 0; m < n_info; m++) ib[m] = (unsigned char)get(info + f * Wi, m);
            CHECK(crc[f] == crc_def(ib, n_info, crc_len, poly));
        }
    }
    free(pos); free(llr); free(fv); free(crc); free(u); free(x); free(info); free(lx); free(metric); free(u1); free(x1); free(info1); free(lx1);
    free(metric1); free(enc); free(pick); free(pick1); free(ib);
    return 0;
}

int main(void)
{
    static const int lists[4] = {1, 2, 4, 8};
    for (int n = 1; n <= 9; n++) {
        const long N = 1l << n;
        const int ks[5] = {0, (int)N, (int)(N / 2), (int)(rnd() % (uint64_t)(N + 1)), 1};
        for (int li = 0; li < 4; li++)
            for (int k = 0; k < 5; k++)
                for (int with = 0; with < 2; with++) {
                    const int K = ks[k], crc_len = with ? (K < 11 ? K : (k == 1 && K >= 32 ? 32 : 11)) : 0;
                    const uint32_t poly = crc_len == 11 ? 0x621u : (crc_len == 32 ? 0x04C11DB7u : (uint32_t)rnd() & pll_crc_mask(crc_len));
                    if (run(n, 0, n % 3 == 0 ? 1 : (n % 3 == 1 ? 31 : 126), lists[li], K, crc_len, poly, with)) return 1;
                    if (run(n, 1, 0, lists[li], K, crc_len, poly, with)) return 1;
                }
    }
    /* refusals */
    int8_t z[8] = {0};
    uint32_t row[4] = {0}, one[1] = {0};
    int32_t pk[1];
    int p2[2] = {1, 1}, p3[3] = {1, 2, 3}, p8[1] = {8};
#define REFUSE(n, ni, pos, kind, maxq, L, cl, cp, F, llr, crc) qldpc_polar_list_decode_host(n, ni, pos, kind, maxq, L, cl, cp, F, llr, NULL, crc, row, NULL, NULL, pk, NULL, NULL)
    CHECK(REFUSE(0, 0, NULL, 0, 31, 4, 0, 0, 1, z, NULL) == QLDPC_ESIZE);
    CHECK(REFUSE(17, 0, NULL, 0, 31, 4, 0, 0, 1, z, NULL) == QLDPC_ESIZE);
    CHECK(REFUSE(3, 0, NULL, 0, 127, 4, 0, 0, 1, z, NULL) == QLDPC_ESIZE && strstr(msg, "int8"));
    CHECK(REFUSE(3, 0, NULL, 0, 0, 4, 0, 0, 1, z, NULL) == QLDPC_ESIZE);
    CHECK(REFUSE(3, 0, NULL, 2, 31, 4, 0, 0, 1, z, NULL) == QLDPC_EINVAL);
    CHECK(REFUSE(3, 0, NULL, 0, 31, 0, 0, 0, 1, z, NULL) == QLDPC_ESIZE);
    CHECK(REFUSE(3, 0, NULL, 0, 31, 3, 0, 0, 1, z, NULL) == QLDPC_ESIZE);
    CHECK(REFUSE(3, 0, NULL, 0, 31, 16, 0, 0, 1, z, NULL) == QLDPC_ESIZE);
    CHECK(REFUSE(3, 2, p2, 0, 31, 4, 0, 0, 1, z, NULL) == QLDPC_EINVAL);
    CHECK(REFUSE(3, 1, p8, 0, 31, 4, 0, 0, 1, z, NULL) == QLDPC_ESIZE);
    CHECK(REFUSE(3, 9, p8, 0, 31, 4, 0, 0, 1, z, NULL) == QLDPC_ESIZE);
    CHECK(REFUSE(3, 1, NULL, 0, 31, 4, 0, 0, 1, z, NULL) == QLDPC_ESIZE);
    CHECK(REFUSE(3, 3, p3, 0, 31, 4, -1, 0, 1, z, NULL) == QLDPC_ESIZE);
    CHECK(REFUSE(3, 3, p3, 0, 31, 4, 33, 0, 1, z, NULL) == QLDPC_ESIZE);
    CHECK(REFUSE(3, 3, p3, 0, 31, 4, 4, 1, 1, z, NULL) == QLDPC_ESIZE);                  /* a CRC longer than the information word */
    CHECK(REFUSE(3, 3, p3, 0, 31, 4, 3, 8, 1, z, NULL) == QLDPC_ESIZE);                  /* x^crc_len is implied */
    CHECK(REFUSE(3, 3, p3, 0, 31, 4, 0, 1, 1, z, NULL) == QLDPC_ESIZE);
    CHECK(REFUSE(3, 3, p3, 0, 31, 4, 0, 0, 1, z, one) == QLDPC_EINVAL);                  /* an expected remainder without a CRC */
    CHECK(REFUSE(3, 3, p3, 0, 31, 4, 3, 3, -1, z, NULL) == QLDPC_EINVAL);
    CHECK(REFUSE(3, 3, p3, 0, 31, 4, 3, 3, 1, NULL, NULL) == QLDPC_EINVAL);
    CHECK(REFUSE(3, 3, p3, 0, 31, 4, 3, 3, 0, NULL, NULL) == QLDPC_OK);
    CHECK(REFUSE(3, 3, p3, 0, 31, 4, 3, 3, 1, z, one) == QLDPC_OK);
    CHECK(qldpc_polar_crc_host(33, 0, 3, 1, row, one) == QLDPC_ESIZE && qldpc_polar_crc_host(-1, 0, 3, 1, row, one) == QLDPC_ESIZE);
    CHECK(qldpc_polar_crc_host(4, 16, 3, 1, row, one) == QLDPC_ESIZE && qldpc_polar_crc_host(4, 3, -1, 1, row, one) == QLDPC_EINVAL);
    CHECK(qldpc_polar_crc_host(4, 3, 3, -1, row, one) == QLDPC_EINVAL && qldpc_polar_crc_host(4, 3, 3, 1, NULL, one) == QLDPC_EINVAL);
    CHECK(qldpc_polar_crc_host(4, 3, 3, 1, row, NULL) == QLDPC_EINVAL && qldpc_polar_crc_host(4, 3, 3, 0, NULL, NULL) == QLDPC_OK);
    CHECK(qldpc_polar_crc_host(4, 3, 0, 1, NULL, one) == QLDPC_OK && one[0] == 0u);
    printf("polar list: sanitizer pass ok\n");
    return 0;
}
