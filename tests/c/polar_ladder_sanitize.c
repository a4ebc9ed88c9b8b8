/* Sanitizer pass over incremental freezing on the host (qldpc_polar_ladder_core.h, the mirrors of qldpc_polar_ladder_host.c and the rows form of the SC
 * mirror in qldpc_polar_host.c, no HIP): every size up to 2^9, both message types, every row malloc'ed at its exact size: the rows decode with
 * all-zero rows against the plain mirror and with all-one rows against its frozen values, Alice's extra row against u read a bit at a time, Bob's
 * rounds on blocks he holds without an error (OK in round 0, nothing disclosed), on blocks he holds wrong with every information bit disclosed (OK,
 * Alice's key), on a block with a key_bits and one with a count out of range, the rounds from zero on noisy blocks with the bookkeeping of counts,
 * decodes and open_per_round checked against each other, and every refusal.
 * Built with -fsanitize=address,undefined by tests/test_polar_ladder_host.py */
#include "qldpc.h"
#include "qldpc_polar_ladder_core.h"

#include "polar_sanitize_common.h"

static int run(int n, int f32, int maxq, int K, int E, int crc_len, uint32_t poly)
{
    const long N = 1l << n, W = pl_words(n), Nf = N - K, Wf = (Nf + 31) / 32, Wi = (K + 31) / 32, We = (E + 31) / 32;
    const int B = 6, F = 3, kind = f32 ? QLDPC_POLAR_F32 : QLDPC_POLAR_I8, rounds = 3, step = 2;
    const double prior = 1.0, pin = f32 ? 16777216.0 : (double)maxq;
    const size_t esz = f32 ? sizeof(float) : 1, row = 4 * (size_t)(B * W);
    int *pos = draw_info_pos(N, K), *xp = (int *)malloc(sizeof(int) * (size_t)(E ? E : 1));
    for (int m = 0; m < E; m++) xp[m] = pos[K - 1 - m];          /* the ladder: the tail of info_pos, backwards */
    /* the rows decode */
    {
        void *llr = malloc(esz * (size_t)(F * N)), *leaf = malloc(esz * (size_t)(F * N)), *leaf2 = malloc(esz * (size_t)(F * N));
        uint32_t *fz = (uint32_t *)malloc(4 * (size_t)(F * W)), *rows = (uint32_t *)malloc(4 * (size_t)(F * W)), *u = (uint32_t *)malloc(4 * (size_t)(F * W)),
                 *x = (uint32_t *)malloc(4 * (size_t)(F * W)), *info = (uint32_t *)malloc(4 * (size_t)(Wi ? F * Wi : 1)), *u2 = (uint32_t *)malloc(4 * (size_t)(F * W)),
                 *x2 = (uint32_t *)malloc(4 * (size_t)(F * W)), *info2 = (uint32_t *)malloc(4 * (size_t)(Wi ? F * Wi : 1));
        fill_llr(llr, F * N, f32, 40, 4.0f);
        for (long i = 0; i < F * W; i++) { fz[i] = (uint32_t)rnd(); rows[i] = 0u; }
        CHECK(qldpc_polar_decode_rows_host(n, K, pos, kind, maxq, F, llr, fz, rows, u, info, x, leaf) == QLDPC_OK);
        CHECK(qldpc_polar_decode_host(n, K, pos, kind, maxq, F, llr, fz, u2, info2, x2, leaf2) == QLDPC_OK);
        CHECK(!memcmp(u, u2, 4 * (size_t)(F * W)) && !memcmp(x, x2, 4 * (size_t)(F * W)) && !memcmp(info, info2, 4 * (size_t)(F * Wi)) && !memcmp(leaf, leaf2, esz * (size_t)(F * N)));
        for (long i = 0; i < F * W; i++) rows[i] = 0xffffffffu;
        CHECK(qldpc_polar_decode_rows_host(n, K, pos, kind, maxq, F, llr, fz, rows, u, NULL, NULL, NULL) == QLDPC_OK);
        for (int f = 0; f < F; f++)
            for (long i = 0; i < N; i++) CHECK(get(u + f * W, i) == get(fz + f * W, i));
        CHECK(qldpc_polar_decode_rows_host(n, K, pos, kind, maxq, F, llr, NULL, rows, NULL, NULL, x, NULL) == QLDPC_OK);      /* everything frozen to 0 */
        for (long i = 0; i < F * W; i++) CHECK(x[i] == 0u);
        for (long i = 0; i < F * W; i++) rows[i] = (uint32_t)rnd();
        CHECK(qldpc_polar_decode_rows_host(n, K, pos, kind, maxq, F, llr, fz, rows, u, info, x, leaf) == QLDPC_OK);
        for (int f = 0; f < F; f++)
            for (long i = 0; i < N; i++)
                if (get(rows + f * W, i)) CHECK(get(u + f * W, i) == get(fz + f * W, i));
        free(llr); free(leaf); free(leaf2); free(fz); free(rows); free(u); free(x); free(info); free(u2); free(x2); free(info2);
    }
    /* the ladder */
    uint32_t *ka = (uint32_t *)malloc(row), *kb = (uint32_t *)malloc(row), *u = (uint32_t *)malloc(row), *before = (uint32_t *)malloc(row),
             *syn = (uint32_t *)malloc(4 * (size_t)(Wf ? B * Wf : 1)), *crc = (uint32_t *)malloc(4 * (size_t)B), *xb = (uint32_t *)malloc(4 * (size_t)(We ? B * We : 1));
    int *bits = (int *)malloc(sizeof(int) * (size_t)B), *extra = (int *)malloc(sizeof(int) * (size_t)B), *status = (int *)malloc(sizeof(int) * (size_t)B),
        *corrected = (int *)malloc(sizeof(int) * (size_t)B), *decodes = (int *)malloc(sizeof(int) * (size_t)B), *per_round = (int *)malloc(sizeof(int) * (size_t)rounds);
    const int lens[6] = {(int)N, (int)(N > 1 ? N - 1 : 1), 1, (int)(1 + rnd() % (uint64_t)N), (int)(N + 1), (int)N};
    for (int f = 0; f < B; f++) bits[f] = lens[f];
    for (long i = 0; i < B * W; i++) ka[i] = (uint32_t)rnd();
    CHECK(qldpc_polar_recon_encode_ladder_host(n, K, pos, crc_len, poly, E, xp, B, ka, bits, Nf ? syn : NULL, crc, E ? xb : NULL) == QLDPC_OK);
    for (int f = 0; f < B; f++) {
        const int k = prc_key_bits(bits[f], n);
        for (long w = 0; w < W; w++) u[f * W + w] = ka[f * W + w] & prc_key_mask(k, (uint32_t)w);
    }
    memcpy(kb, u, row);                                           /* Bob holds Alice's keys with a clean pad */
    CHECK(qldpc_polar_encode_host(n, B, u, u) == QLDPC_OK);
    for (int f = 0; f < B; f++) {
        for (int m = 0; m < E; m++) CHECK(get(xb + f * We, m) == get(u + f * W, xp[m]));
        for (long m = E; m < 32 * We; m++) CHECK(!get(xb + f * We, m));
    }
    /* nothing to correct: OK in round 0 at the count given, one decode; block 4 has no valid length, block 5 no valid count */
    for (int f = 0; f < B; f++) extra[f] = f == 5 ? E + 1 : (int)(rnd() % (uint64_t)(E + 1));
    memcpy(before, kb, row);
    CHECK(qldpc_polar_recon_decode_rounds_host(n, K, pos, kind, maxq, crc_len, poly, prior, pin, E, xp, B, kb, bits, Nf ? syn : NULL, crc, E ? xb : NULL, extra, step, rounds, 0,
                                               status, corrected, decodes, per_round) == QLDPC_OK);
    for (int f = 0; f < B; f++) {
        if (f >= 4) { CHECK(status[f] == QLDPC_ESIZE && corrected[f] == -1 && decodes[f] == 0 && !memcmp(kb + f * W, before + f * W, 4 * (size_t)W)); continue; }
        CHECK(status[f] == QLDPC_OK && corrected[f] == 0 && decodes[f] == 1 && !memcmp(kb + f * W, before + f * W, 4 * (size_t)W));
    }
    CHECK(extra[5] == E + 1 && per_round[0] == 4 && per_round[1] == 0 && per_round[2] == 0);
    /* Bob holds junk: rounds from zero, every output optional left out once; the bookkeeping */
    for (long i = 0; i < B * W; i++) kb[i] = (uint32_t)rnd() & pl_row_mask(n);
    for (int f = 0; f < B; f++) extra[f] = 0;
    CHECK(qldpc_polar_recon_decode_rounds_host(n, K, pos, kind, maxq, crc_len, poly, prior, pin, E, xp, B, kb, bits, Nf ? syn : NULL, crc, E ? xb : NULL, extra, step, rounds, 0,
                                               status, NULL, decodes, per_round) == QLDPC_OK);
    int total = 0;
    for (int f = 0; f < B; f++) {
        if (f == 4) { CHECK(status[f] == QLDPC_ESIZE && decodes[f] == 0); continue; }
        CHECK(decodes[f] >= 1 && decodes[f] <= rounds && (status[f] == QLDPC_OK || status[f] == QLDPC_EDECODE));
        CHECK(extra[f] == ((decodes[f] - 1) * step < E ? (decodes[f] - 1) * step : E));
        total += decodes[f];
    }
    CHECK(per_round[0] + per_round[1] + per_round[2] == total && per_round[0] == B - 1 && per_round[1] >= per_round[2]);
    /* resume with one round, every information bit disclosed where the ladder is the whole set: OK, and the key is Alice's */
    for (int f = 0; f < B; f++) { extra[f] = E; status[f] = f == 1 ? QLDPC_OK : QLDPC_EDECODE; }
    memcpy(before, kb, row);
    CHECK(qldpc_polar_recon_decode_rounds_host(n, K, pos, kind, maxq, crc_len, poly, prior, pin, E, xp, B, kb, bits, Nf ? syn : NULL, crc, E ? xb : NULL, extra, 1, 1, 1, status,
                                               corrected, NULL, NULL) == QLDPC_OK);
    CHECK(status[1] == QLDPC_OK && !memcmp(kb + W, before + W, 4 * (size_t)W) && status[4] == QLDPC_ESIZE);
    if (E == K)
        for (int f = 0; f < B; f++)
            if (f != 1 && f != 4) {
                CHECK(status[f] == QLDPC_OK && corrected[f] >= 0);
                for (long w = 0; w < W; w++) CHECK(kb[f * W + w] == (ka[f * W + w] & prc_key_mask(bits[f], (uint32_t)w)));
            }
    free(pos); free(xp); free(ka); free(kb); free(u); free(before); free(syn); free(crc); free(xb); free(bits); free(extra); free(status); free(corrected);
    free(decodes); free(per_round);
    return 0;
}

int main(void)
{
    for (int n = 1; n <= 9; n++) {
        const long N = 1l << n;
        const int ks[4] = {(int)N, (int)(N / 2), (int)(1 + rnd() % (uint64_t)N), 1};
        for (int k = 0; k < 4; k++)
            for (int e = 0; e < 4; e++) {                         /* E = K, 0, 1, 33 (at most K) */
                const int K = ks[k], crc_len = K >= 32 && k == 0 ? 32 : (K >= 11 ? 11 : K), Es[4] = {K, 0, 1, K < 33 ? K : 33};
                const uint32_t poly = crc_len == 11 ? 0x621u : (crc_len == 32 ? 0x04C11DB7u : (uint32_t)rnd() & pll_crc_mask(crc_len));
                if (run(n, 0, n % 3 == 0 ? 1 : (n % 3 == 1 ? 31 : 126), K, Es[e], crc_len, poly)) return 1;
                if (run(n, 1, 0, K, Es[e], crc_len, poly)) return 1;
            }
    }
    /* the ladder rule on its own */
    CHECK(pld_next_extra(0, 10, 3) == 3 && pld_next_extra(8, 10, 3) == 10 && pld_next_extra(9, 10, 0x7fffffff) == 10);
    CHECK(pld_stays_open(3, 10, 0, 2) && !pld_stays_open(10, 10, 0, 2) && !pld_stays_open(3, 10, 1, 2));
    CHECK(pld_entry(0, 5, 8, 3, 0, 0) == PLD_OPEN && pld_entry(0, 0, 9, 3, 0, 0) == PLD_REFUSE && pld_entry(0, 0, 8, 3, 1, 0) == PLD_REFUSE);
    CHECK(pld_entry(1, PRC_OK, 9, 3, -1, 0) == PLD_KEEP && pld_entry(1, PRC_EDECODE, 8, 3, 0, 0) == PLD_OPEN && pld_entry(1, PRC_EDECODE, 0, 3, 0, 0) == PLD_REFUSE);
    /* refusals */
    uint32_t w[4] = {0}, c1[1] = {0};
    int8_t z[8] = {0};
    int st[1], ex[1] = {0}, p2[2] = {1, 1}, p3[3] = {1, 2, 3}, x1[1] = {2}, x0[1] = {0}, x4[4] = {1, 2, 3, 4};
    CHECK(qldpc_polar_decode_rows_host(3, 3, p3, 0, 31, 1, z, NULL, NULL, w, NULL, NULL, NULL) == QLDPC_EINVAL && strstr(msg, "frozen_rows"));
    CHECK(qldpc_polar_decode_rows_host(3, 3, p3, 0, 31, 1, NULL, NULL, w, w, NULL, NULL, NULL) == QLDPC_EINVAL);
    CHECK(qldpc_polar_decode_rows_host(0, 0, NULL, 0, 31, 1, z, NULL, w, w, NULL, NULL, NULL) == QLDPC_ESIZE);
    CHECK(qldpc_polar_decode_rows_host(3, 2, p2, 0, 31, 1, z, NULL, w, w, NULL, NULL, NULL) == QLDPC_EINVAL);
    CHECK(qldpc_polar_decode_rows_host(3, 3, p3, 0, 31, -1, z, NULL, w, w, NULL, NULL, NULL) == QLDPC_EINVAL);
    CHECK(qldpc_polar_decode_rows_host(3, 3, p3, 0, 31, 0, NULL, NULL, NULL, NULL, NULL, NULL, NULL) == QLDPC_OK);
    CHECK(qldpc_polar_decode_rows_host(3, 3, p3, 0, 31, 1, z, NULL, w, NULL, NULL, NULL, NULL) == QLDPC_OK);
#define ENC(E, xp, B, keys, syn, crc, xb) qldpc_polar_recon_encode_ladder_host(3, 3, p3, 3, 3, E, xp, B, keys, NULL, syn, crc, xb)
    CHECK(ENC(4, x4, 1, w, w, c1, w) == QLDPC_ESIZE && strstr(msg, "n_extra"));
    CHECK(ENC(-1, x1, 1, w, w, c1, w) == QLDPC_ESIZE);
    CHECK(ENC(2, p2, 1, w, w, c1, w) == QLDPC_EINVAL && strstr(msg, "extra_pos"));
    CHECK(ENC(1, x0, 1, w, w, c1, w) == QLDPC_EINVAL);
    CHECK(ENC(1, NULL, 1, w, w, c1, w) == QLDPC_EINVAL);
    CHECK(ENC(1, x1, 1, w, w, c1, NULL) == QLDPC_EINVAL);
    CHECK(ENC(1, x1, 1, NULL, w, c1, w) == QLDPC_EINVAL);
    CHECK(ENC(1, x1, 1, w, NULL, c1, w) == QLDPC_EINVAL);
    CHECK(ENC(1, x1, 1, w, w, NULL, w) == QLDPC_EINVAL);
    CHECK(ENC(1, x1, -1, w, w, c1, w) == QLDPC_EINVAL);
    CHECK(ENC(1, x1, 0, NULL, NULL, NULL, NULL) == QLDPC_OK);
    CHECK(ENC(0, NULL, 1, w, w, c1, NULL) == QLDPC_OK);
    CHECK(qldpc_polar_recon_encode_ladder_host(0, 0, NULL, 1, 1, 0, NULL, 1, w, NULL, w, c1, NULL) == QLDPC_ESIZE);
    CHECK(qldpc_polar_recon_encode_ladder_host(3, 3, p3, 0, 0, 1, x1, 1, w, NULL, w, c1, w) == QLDPC_ESIZE && strstr(msg, "crc_len"));
#define ROUNDS(E, xp, B, keys, xb, extra, step, rounds, resume, status) \
    qldpc_polar_recon_decode_rounds_host(3, 3, p3, 0, 31, 3, 3, 1.0, 31.0, E, xp, B, keys, NULL, w, c1, xb, extra, step, rounds, resume, status, NULL, NULL, NULL)
    CHECK(ROUNDS(1, x1, 1, w, w, ex, 0, 1, 0, st) == QLDPC_EINVAL && strstr(msg, "step"));
    CHECK(ROUNDS(1, x1, 1, w, w, ex, 1, 0, 0, st) == QLDPC_EINVAL);
    CHECK(ROUNDS(1, x1, 1, w, w, ex, 1, 1, 2, st) == QLDPC_EINVAL);
    CHECK(ROUNDS(1, x1, 1, w, w, ex, 1, 1, -1, st) == QLDPC_EINVAL);
    CHECK(ROUNDS(4, x4, 1, w, w, ex, 1, 1, 0, st) == QLDPC_ESIZE);
    CHECK(ROUNDS(2, p2, 1, w, w, ex, 1, 1, 0, st) == QLDPC_EINVAL);
    CHECK(ROUNDS(1, x0, 1, w, w, ex, 1, 1, 0, st) == QLDPC_EINVAL);
    CHECK(ROUNDS(1, x1, 1, NULL, w, ex, 1, 1, 0, st) == QLDPC_EINVAL && strstr(msg, "keys"));
    CHECK(ROUNDS(1, x1, 1, w, NULL, ex, 1, 1, 0, st) == QLDPC_EINVAL && strstr(msg, "extra_bits"));
    CHECK(ROUNDS(1, x1, 1, w, w, NULL, 1, 1, 0, st) == QLDPC_EINVAL);
    CHECK(ROUNDS(1, x1, 1, w, w, ex, 1, 1, 0, NULL) == QLDPC_EINVAL);
    CHECK(ROUNDS(1, x1, -1, w, w, ex, 1, 1, 0, st) == QLDPC_EINVAL);
    CHECK(ROUNDS(1, x1, 0, NULL, NULL, NULL, 1, 1, 0, NULL) == QLDPC_OK);
    CHECK(ROUNDS(0, NULL, 1, w, NULL, ex, 1, 1, 0, st) == QLDPC_OK);
    CHECK(qldpc_polar_recon_decode_rounds_host(3, 3, p3, 0, 31, 3, 3, 0.0, 31.0, 1, x1, 1, w, NULL, w, c1, w, ex, 1, 1, 0, st, NULL, NULL, NULL) == QLDPC_EINVAL && strstr(msg, "prior"));
    CHECK(qldpc_polar_recon_decode_rounds_host(3, 3, p3, 2, 31, 3, 3, 1.0, 31.0, 1, x1, 1, w, NULL, w, c1, w, ex, 1, 1, 0, st, NULL, NULL, NULL) == QLDPC_EINVAL);
    CHECK(qldpc_polar_recon_decode_rounds_host(3, 3, p3, 0, 31, 4, 3, 1.0, 31.0, 1, x1, 1, w, NULL, w, c1, w, ex, 1, 1, 0, st, NULL, NULL, NULL) == QLDPC_ESIZE);
    CHECK(qldpc_polar_recon_decode_rounds_host(3, 3, p3, 0, 31, 3, 3, 1.0, 31.0, 1, x1, 1, w, NULL, NULL, c1, w, ex, 1, 1, 0, st, NULL, NULL, NULL) == QLDPC_EINVAL);
    CHECK(qldpc_polar_recon_decode_rounds_host(3, 3, p3, 0, 31, 3, 3, 1.0, 31.0, 1, x1, 1, w, NULL, w, NULL, w, ex, 1, 1, 0, st, NULL, NULL, NULL) == QLDPC_EINVAL);
    CHECK(qldpc_polar_recon_ladder_extra_host(10, 512, 128, 1024, 0.11, 1.5) == 128 && qldpc_polar_recon_ladder_extra_host(10, 512, 128, 1024, 0.01, 1.0) == 0);
    CHECK(qldpc_polar_recon_ladder_extra_host(0, 0, 0, 1, 0.1, 1.0) == QLDPC_ESIZE && qldpc_polar_recon_ladder_extra_host(4, 8, 9, 16, 0.1, 1.0) == QLDPC_ESIZE);
    CHECK(qldpc_polar_recon_ladder_extra_host(4, 8, 8, 17, 0.1, 1.0) == QLDPC_ESIZE && qldpc_polar_recon_ladder_extra_host(4, 8, 8, 16, 0.7, 1.0) == QLDPC_EINVAL);
    printf("polar ladder: sanitizer pass ok\n");
    return 0;
}
