/* Sanitizer pass over the polar reconciliation sessions on the host (qldpc_polar_recon_core.h and the mirrors of qldpc_polar_recon_host.c, no HIP):
 * every size up to 2^9, both message types and every host decoder, every row malloc'ed at its exact size: the tables against the frozen mask read a
 * bit at a time, Alice's syndrome and crc against u = encode(masked key) read a bit at a time, Bob's prior and frozen row against the rule, a
 * block that Bob holds without an error through the decode mirror (OK, nothing corrected, the key with a clean pad), a block with a key_bits out of
 * range, the verdict on rows of exact size with and without pick, and every refusal.
 * Built with -fsanitize=address,undefined by tests/test_polar_recon_host.py */
#include "qldpc.h"
#include "qldpc_polar_recon_core.h"

#include "polar_sanitize_common.h"

static int run(int n, int f32, int maxq, int K, int crc_len, uint32_t poly, int form, int rule, int list_size)
{
    const long N = 1l << n, W = pl_words(n), Nf = N - K, Wf = (Nf + 31) / 32, Wi = (K + 31) / 32;
    const int B = 5, kind = f32 ? QLDPC_POLAR_F32 : QLDPC_POLAR_I8;
    const double prior = 1.0, pin = f32 ? 16777216.0 : (double)maxq;
    int *pos = draw_info_pos(N, K);
    const size_t esz = f32 ? sizeof(float) : 1, row = 4 * (size_t)(B * W);
    uint32_t *mask = (uint32_t *)malloc(4 * (size_t)W), *ka = (uint32_t *)malloc(row), *kb = (uint32_t *)malloc(row), *u = (uint32_t *)malloc(row),
             *syn = (uint32_t *)malloc(4 * (size_t)(Wf ? B * Wf : 1)), *crc = (uint32_t *)malloc(4 * (size_t)B), *frozen = (uint32_t *)malloc(row),
             *info = (uint32_t *)malloc(4 * (size_t)(Wi ? B * Wi : 1));
    int *prefix = (int *)malloc(sizeof(int) * (size_t)W), *fpos = (int *)malloc(sizeof(int) * (size_t)(Nf ? Nf : 1)), *bits = (int *)malloc(sizeof(int) * (size_t)B),
        *status = (int *)malloc(sizeof(int) * (size_t)B), *corrected = (int *)malloc(sizeof(int) * (size_t)B);
    int32_t *pick = (int32_t *)malloc(4 * (size_t)B);
    void *llr = malloc(esz * (size_t)(B * N));
    /* the tables */
    CHECK(qldpc_polar_recon_tables_host(n, K, pos, mask, prefix, fpos) == QLDPC_OK);
    long r = 0;
    for (long i = 0; i < N; i++) {
        if ((i & 31) == 0) CHECK(prefix[i >> 5] == r);
        if (get(mask, i)) { CHECK(fpos[r] == i); r++; }
    }
    CHECK(r == Nf);
    for (int m = 0; m < K; m++) CHECK(!get(mask, pos[m]));
    CHECK(qldpc_polar_recon_tables_host(n, K, pos, NULL, NULL, NULL) == QLDPC_OK);
    /* the blocks: key lengths N, N - 1, 1, a random one, and one out of range; junk past every key */
    const int lens[5] = {(int)N, (int)(N > 1 ? N - 1 : 1), 1, (int)(1 + rnd() % (uint64_t)N), (int)(N + 1)};
    for (int f = 0; f < B; f++) bits[f] = lens[f];
    for (long i = 0; i < B * W; i++) ka[i] = (uint32_t)rnd();
    /* Alice */
    CHECK(qldpc_polar_recon_encode_host(n, K, pos, crc_len, poly, B, ka, bits, Nf ? syn : NULL, crc) == QLDPC_OK);
    for (int f = 0; f < B; f++) {
        const int k = prc_key_bits(bits[f], n);
        for (long w = 0; w < W; w++) u[f * W + w] = ka[f * W + w] & prc_key_mask(k, (uint32_t)w);
        for (long i = 0; i < N; i++) CHECK(get(u + f * W, i) == (i < k ? get(ka + f * W, i) : 0));
    }
    memcpy(kb, u, row);                                           /* Bob holds Alice's keys with a clean pad .. */
    CHECK(qldpc_polar_encode_host(n, B, u, u) == QLDPC_OK);
    for (int f = 0; f < B; f++) {
        for (long j = 0; j < Nf; j++) CHECK(get(syn + f * Wf, j) == get(u + f * W, fpos[j]));
        for (long j = Nf; j < 32 * Wf; j++) CHECK(!get(syn + f * Wf, j));
        uint32_t reg = 0u;
        for (int m = 0; m < K; m++) reg = pll_crc_step(reg, (unsigned)get(u + f * W, pos[m]), crc_len, poly);
        CHECK(reg == crc[f]);
    }
    /* Bob's prior */
    CHECK(qldpc_polar_recon_prior_host(n, K, pos, kind, maxq, prior, pin, B, kb, bits, Nf ? syn : NULL, llr, frozen) == QLDPC_OK);
    for (int f = 0; f < B; f++) {
        const int k = prc_key_bits(bits[f], n);
        for (long i = 0; i < N; i++) {
            const double l = f32 ? (double)((float *)llr)[f * N + i] : (double)((int8_t *)llr)[f * N + i];
            CHECK(l == (i < k ? (get(kb + f * W, i) ? -prior : prior) : pin));
            CHECK(get(frozen + f * W, i) == (get(mask, i) ? get(u + f * W, i) : 0));
        }
    }
    /* the session's decode: nothing to correct, so every block of a valid length is OK and its key stays; .. and junk in the pad goes */
    for (int f = 0; f < B; f++)
        for (long w = 0; w < W; w++) kb[f * W + w] |= (uint32_t)rnd() & ~prc_key_mask(prc_key_bits(bits[f], n), (uint32_t)w) & pl_row_mask(n);
    uint32_t *before = (uint32_t *)malloc(row);
    memcpy(before, kb, row);
    CHECK(qldpc_polar_recon_decode_host(n, K, pos, kind, maxq, form, rule, list_size, crc_len, poly, prior, pin, B, kb, bits, Nf ? syn : NULL, crc, status, corrected,
                                        list_size ? pick : NULL) == QLDPC_OK);
    for (int f = 0; f < B; f++) {
        if (!prc_key_bits_ok(bits[f], n)) {
            CHECK(status[f] == QLDPC_ESIZE && corrected[f] == -1 && !memcmp(kb + f * W, before + f * W, 4 * (size_t)W));
            continue;
        }
        CHECK(status[f] == QLDPC_OK && corrected[f] == 0);
        if (list_size) CHECK(pick[f] >= 0);
        for (long w = 0; w < W; w++) CHECK(kb[f * W + w] == (before[f * W + w] & prc_key_mask(bits[f], (uint32_t)w)));
    }
    /* the verdict on rows of exact size: a wrong remainder, and a pick of -1 */
    for (int f = 0; f < B; f++)
        for (long j = 0; j < Wi; j++) info[f * Wi + j] = (uint32_t)rnd();
    CHECK(qldpc_polar_crc_host(crc_len, poly, K, B, info, crc) == QLDPC_OK);
    crc[1] ^= 1u;
    for (int f = 0; f < B; f++) pick[f] = f == 2 ? -1 : f;
    memcpy(before, kb, row);
    CHECK(qldpc_polar_recon_verdict_host(n, K, crc_len, poly, B, info, u, NULL, kb, NULL, crc, status, NULL) == QLDPC_OK);
    for (int f = 0; f < B; f++) CHECK(status[f] == (f == 1 ? QLDPC_EDECODE : QLDPC_OK));
    memcpy(kb, before, row);
    CHECK(qldpc_polar_recon_verdict_host(n, K, 0, 0, B, NULL, u, pick, kb, NULL, NULL, status, corrected) == QLDPC_OK);
    for (int f = 0; f < B; f++) CHECK(status[f] == (f == 2 ? QLDPC_EDECODE : QLDPC_OK) && (f == 2) == (corrected[f] == -1));
    free(pos); free(mask); free(ka); free(kb); free(u); free(syn); free(crc); free(frozen); free(info); free(prefix); free(fpos); free(bits); free(status);
    free(corrected); free(pick); free(llr); free(before);
    return 0;
}

int main(void)
{
    for (int n = 1; n <= 9; n++) {
        const long N = 1l << n;
        const int ks[4] = {(int)N, (int)(N / 2), (int)(1 + rnd() % (uint64_t)N), 1};
        for (int k = 0; k < 4; k++)
            for (int d = 0; d < 5; d++) {                         /* SC, SSC, wide, list 1, list 4 */
                const int K = ks[k], crc_len = K >= 32 && k == 0 ? 32 : (K >= 11 ? 11 : K);
                const uint32_t poly = crc_len == 11 ? 0x621u : (crc_len == 32 ? 0x04C11DB7u : (uint32_t)rnd() & pll_crc_mask(crc_len));
                const int form = d == 2 ? QLDPC_POLAR_WIDE : QLDPC_POLAR_LANES, rule = d == 1 ? QLDPC_POLAR_SSC : QLDPC_POLAR_SC, L = d == 3 ? 1 : (d == 4 ? 4 : 0);
                if (run(n, 0, n % 3 == 0 ? 1 : (n % 3 == 1 ? 31 : 126), K, crc_len, poly, form, rule, L)) return 1;
                if (run(n, 1, 0, K, crc_len, poly, form, rule, L)) return 1;
            }
    }
    /* refusals */
    uint32_t w[4] = {0}, c1[1] = {0};
    int8_t z[8] = {0};
    int st[1], p2[2] = {1, 1}, p3[3] = {1, 2, 3}, p8[1] = {8};
    int32_t pk[1];
    CHECK(qldpc_polar_recon_encode_host(0, 0, NULL, 1, 1, 1, w, NULL, w, c1) == QLDPC_ESIZE);
    CHECK(qldpc_polar_recon_encode_host(21, 0, NULL, 1, 1, 1, w, NULL, w, c1) == QLDPC_ESIZE);
    CHECK(qldpc_polar_recon_encode_host(3, 2, p2, 1, 1, 1, w, NULL, w, c1) == QLDPC_EINVAL);
    CHECK(qldpc_polar_recon_encode_host(3, 1, p8, 1, 1, 1, w, NULL, w, c1) == QLDPC_ESIZE);
    CHECK(qldpc_polar_recon_encode_host(3, 3, p3, 0, 0, 1, w, NULL, w, c1) == QLDPC_ESIZE && strstr(msg, "crc_len"));
    CHECK(qldpc_polar_recon_encode_host(3, 3, p3, 4, 1, 1, w, NULL, w, c1) == QLDPC_ESIZE);
    CHECK(qldpc_polar_recon_encode_host(3, 3, p3, 3, 8, 1, w, NULL, w, c1) == QLDPC_ESIZE);
    CHECK(qldpc_polar_recon_encode_host(3, 3, p3, 33, 0, 1, w, NULL, w, c1) == QLDPC_ESIZE);
    CHECK(qldpc_polar_recon_encode_host(3, 3, p3, 3, 3, -1, w, NULL, w, c1) == QLDPC_EINVAL);
    CHECK(qldpc_polar_recon_encode_host(3, 3, p3, 3, 3, 1, NULL, NULL, w, c1) == QLDPC_EINVAL);
    CHECK(qldpc_polar_recon_encode_host(3, 3, p3, 3, 3, 1, w, NULL, NULL, c1) == QLDPC_EINVAL);
    CHECK(qldpc_polar_recon_encode_host(3, 3, p3, 3, 3, 1, w, NULL, w, NULL) == QLDPC_EINVAL);
    CHECK(qldpc_polar_recon_encode_host(3, 3, p3, 3, 3, 0, NULL, NULL, NULL, NULL) == QLDPC_OK);
    CHECK(qldpc_polar_recon_prior_host(3, 3, p3, 0, 31, 0.0, 31.0, 1, w, NULL, w, z, w) == QLDPC_EINVAL && strstr(msg, "prior"));
    CHECK(qldpc_polar_recon_prior_host(3, 3, p3, 0, 31, 1.0, 32.0, 1, w, NULL, w, z, w) == QLDPC_EINVAL);
    CHECK(qldpc_polar_recon_prior_host(3, 3, p3, 0, 31, 1.5, 31.0, 1, w, NULL, w, z, w) == QLDPC_EINVAL);
    CHECK(qldpc_polar_recon_prior_host(3, 3, p3, 0, 31, 1e300, 1e301, 1, w, NULL, w, z, w) == QLDPC_EINVAL);
    CHECK(qldpc_polar_recon_prior_host(3, 3, p3, 1, 0, 1e300, 1e301, 1, w, NULL, w, z, w) == QLDPC_EINVAL);
    CHECK(qldpc_polar_recon_prior_host(3, 3, p3, 1, 0, 1e-300, 1.0, 1, w, NULL, w, z, w) == QLDPC_EINVAL);
    CHECK(qldpc_polar_recon_prior_host(3, 3, p3, 1, 0, 2.0, 1.0, 1, w, NULL, w, z, w) == QLDPC_EINVAL);
    CHECK(qldpc_polar_recon_prior_host(3, 3, p3, 0, 127, 1.0, 31.0, 1, w, NULL, w, z, w) == QLDPC_ESIZE);
    CHECK(qldpc_polar_recon_prior_host(3, 3, p3, 2, 31, 1.0, 31.0, 1, w, NULL, w, z, w) == QLDPC_EINVAL);
    CHECK(qldpc_polar_recon_prior_host(3, 3, p3, 0, 31, 1.0, 31.0, -1, w, NULL, w, z, w) == QLDPC_EINVAL);
    CHECK(qldpc_polar_recon_prior_host(3, 3, p3, 0, 31, 1.0, 31.0, 1, w, NULL, NULL, z, w) == QLDPC_EINVAL);
    CHECK(qldpc_polar_recon_prior_host(3, 3, p3, 0, 31, 1.0, 31.0, 1, w, NULL, w, NULL, w) == QLDPC_EINVAL);
    CHECK(qldpc_polar_recon_prior_host(3, 3, p3, 0, 31, 1.0, 31.0, 1, w, NULL, w, z, NULL) == QLDPC_EINVAL);
    CHECK(qldpc_polar_recon_prior_host(3, 3, p3, 0, 31, 1.0, 31.0, 0, NULL, NULL, NULL, NULL, NULL) == QLDPC_OK);
    CHECK(qldpc_polar_recon_verdict_host(3, 9, 1, 1, 1, w, w, NULL, w, NULL, c1, st, NULL) == QLDPC_ESIZE);
    CHECK(qldpc_polar_recon_verdict_host(3, 3, 0, 0, 1, w, w, NULL, w, NULL, c1, st, NULL) == QLDPC_ESIZE);
    CHECK(qldpc_polar_recon_verdict_host(3, 3, 1, 1, 1, NULL, w, NULL, w, NULL, c1, st, NULL) == QLDPC_EINVAL);
    CHECK(qldpc_polar_recon_verdict_host(3, 3, 1, 1, 1, w, w, NULL, w, NULL, NULL, st, NULL) == QLDPC_EINVAL);
    CHECK(qldpc_polar_recon_verdict_host(3, 3, 1, 1, 1, w, w, NULL, w, NULL, c1, NULL, NULL) == QLDPC_EINVAL);
    CHECK(qldpc_polar_recon_verdict_host(3, 3, 1, 1, -1, w, w, NULL, w, NULL, c1, st, NULL) == QLDPC_EINVAL);
#define DECODE(form, rule, L, cl, B, keys, pick) qldpc_polar_recon_decode_host(3, 3, p3, 0, 31, form, rule, L, cl, 1, 1.0, 31.0, B, keys, NULL, w, c1, st, NULL, pick)
    CHECK(DECODE(0, 0, 3, 1, 1, w, NULL) == QLDPC_ESIZE);
    CHECK(DECODE(2, 0, 0, 1, 1, w, NULL) == QLDPC_EINVAL);
    CHECK(DECODE(0, 2, 0, 1, 1, w, NULL) == QLDPC_EINVAL);
    CHECK(DECODE(1, 0, 4, 1, 1, w, NULL) == QLDPC_EINVAL);
    CHECK(DECODE(0, 0, 0, 1, 1, w, pk) == QLDPC_EINVAL && strstr(msg, "pick"));
    CHECK(DECODE(0, 0, 0, 0, 1, w, NULL) == QLDPC_ESIZE);
    CHECK(DECODE(0, 0, 0, 1, -1, w, NULL) == QLDPC_EINVAL);
    CHECK(DECODE(0, 0, 0, 1, 1, NULL, NULL) == QLDPC_EINVAL);
    CHECK(DECODE(0, 0, 0, 1, 0, NULL, NULL) == QLDPC_OK);
    CHECK(DECODE(0, 0, 4, 1, 1, w, pk) == QLDPC_OK);
    CHECK(qldpc_polar_recon_decode_host(6, 3, p3, 0, 31, QLDPC_POLAR_WIDE, QLDPC_POLAR_SSC, 0, 1, 1, 1.0, 31.0, 1, w, NULL, w, c1, st, NULL, NULL) == QLDPC_EUNSUPPORTED);
    CHECK(qldpc_polar_recon_decode_host(17, 3, p3, 0, 31, 0, 0, 4, 1, 1, 1.0, 31.0, 1, w, NULL, w, c1, st, NULL, NULL) == QLDPC_ESIZE);
    CHECK(qldpc_polar_recon_tables_host(0, 0, NULL, w, NULL, NULL) == QLDPC_ESIZE && qldpc_polar_recon_tables_host(3, 2, p2, w, NULL, NULL) == QLDPC_EINVAL);
    printf("polar recon: sanitizer pass ok\n");
    return 0;
}
