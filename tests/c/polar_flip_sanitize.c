/* Sanitizer pass over SC-Flip trials on the host (qldpc_polar_flip_core.h and the mirrors of qldpc_polar_flip_host.c, no HIP): every size up to 2^9,
 * both message types, every array malloc'ed at its stated size.  The select on random leaf rows with and without a ladder: ascending keys, only
 * candidates, void entries exactly where the candidates run out.  The session mirror on blocks Bob holds without an error (OK at once, one
 * decode, flip_pos -1), on blocks with one wrong bit and on junk, with the bookkeeping of status, corrected, flip_pos, decodes and n_tried
 * checked against each other, every optional output left out once, a resumed call, and every refusal.
 * Built with -fsanitize=address,undefined by tests/test_polar_flip_host.py */
#include "qldpc.h"
#include "qldpc_polar_flip_core.h"

#include "polar_sanitize_common.h"

static int run(int n, int f32, int maxq, int K, int E, int crc_len, uint32_t poly, int T)
{
    const long N = 1l << n, W = pl_words(n), Nf = N - K, Wf = (Nf + 31) / 32, We = (E + 31) / 32;
    const int B = 7, F = 3, kind = f32 ? QLDPC_POLAR_F32 : QLDPC_POLAR_I8;
    const double prior = 1.0, pin = f32 ? 16777216.0 : (double)maxq;
    const size_t esz = f32 ? sizeof(float) : 1, row = 4 * (size_t)(B * W);
    int *pos = draw_info_pos(N, K), *xp = (int *)malloc(sizeof(int) * (size_t)(E ? E : 1));
    for (int m = 0; m < E; m++) xp[m] = pos[K - 1 - m];
    uint32_t *mask = (uint32_t *)malloc(4 * (size_t)W);
    int *rank = (int *)malloc(sizeof(int) * (size_t)N);
    for (long w = 0; w < W; w++) mask[w] = 0xffffffffu;
    for (int m = 0; m < K; m++) mask[pos[m] >> 5] &= ~(1u << (31 - (pos[m] & 31)));
    CHECK(pld_rank_table(n, mask, K, E, xp, rank) == 0);
    /* the select */
    {
        void *leaf = malloc(esz * (size_t)(F * N));
        int *sel = (int *)malloc(sizeof(int) * (size_t)(F * T)), *extra = (int *)malloc(sizeof(int) * (size_t)F);
        fill_llr(leaf, F * N, f32, 3, 1.0f);                      /* few levels: ties */
        if (!f32) for (long i = 0; i < F * N; i++) if (((int8_t *)leaf)[i] == -128) ((int8_t *)leaf)[i] = -127;
        for (int f = 0; f < F; f++) extra[f] = f == 0 ? 0 : (f == 1 ? E : (int)(rnd() % (uint64_t)(E + 1)));
        for (int with = 0; with < 2; with++) {
            CHECK(qldpc_polar_flip_select_host(n, kind, F, leaf, mask, with ? rank : NULL, with ? extra : NULL, T, sel) == QLDPC_OK);
            for (int f = 0; f < F; f++) {
                const int cand = K - (with ? extra[f] : 0);
                uint64_t last = 0;
                for (int t = 0; t < T; t++) {
                    const int p = sel[f * T + t];
                    if (t >= cand) { CHECK(p == -1); continue; }
                    CHECK(p >= 0 && p < N && !get(mask, p) && (!with || rank[p] >= extra[f]));
                    const uint32_t mag = f32 ? pfl_mag_f32(((float *)leaf)[f * N + p]) : pfl_mag_i8(((int8_t *)leaf)[f * N + p]);
                    const uint64_t key = (uint64_t)mag << 32 | (uint64_t)p;
                    CHECK(t == 0 || key > last);
                    last = key;
                }
            }
        }
        free(leaf); free(sel); free(extra);
    }
    /* the session */
    uint32_t *ka = (uint32_t *)malloc(row), *kb = (uint32_t *)malloc(row), *before = (uint32_t *)malloc(row), *syn = (uint32_t *)malloc(4 * (size_t)(Wf ? B * Wf : 1)),
             *crc = (uint32_t *)malloc(4 * (size_t)B), *xb = (uint32_t *)malloc(4 * (size_t)(We ? B * We : 1));
    int *bits = (int *)malloc(sizeof(int) * (size_t)B), *extra = (int *)malloc(sizeof(int) * (size_t)B), *status = (int *)malloc(sizeof(int) * (size_t)B),
        *corrected = (int *)malloc(sizeof(int) * (size_t)B), *decodes = (int *)malloc(sizeof(int) * (size_t)B);
    int32_t *fp = (int32_t *)malloc(sizeof(int32_t) * (size_t)B);
    int tried = -1;
    const int lens[7] = {(int)N, (int)(N > 1 ? N - 1 : 1), 1, (int)(1 + rnd() % (uint64_t)N), (int)(N + 1), (int)N, (int)N};
    for (int f = 0; f < B; f++) { bits[f] = lens[f]; extra[f] = f == 5 ? E + 1 : (int)(rnd() % (uint64_t)(E + 1)); }
    for (long i = 0; i < B * W; i++) ka[i] = (uint32_t)rnd();
    CHECK(qldpc_polar_recon_encode_ladder_host(n, K, pos, crc_len, poly, E, xp, B, ka, bits, Nf ? syn : NULL, crc, E ? xb : NULL) == QLDPC_OK);
    for (int f = 0; f < B; f++)
        for (long w = 0; w < W; w++) kb[f * W + w] = ka[f * W + w] & prc_key_mask(prc_key_bits(bits[f], n), (uint32_t)w);
    /* nothing to correct: OK at once; block 4 has no valid length, block 5 no valid count */
    memcpy(before, kb, row);
    CHECK(qldpc_polar_recon_decode_flip_host(n, K, pos, kind, maxq, crc_len, poly, prior, pin, E, xp, B, kb, bits, Nf ? syn : NULL, crc, E ? xb : NULL, extra, T, 0, status,
                                             corrected, fp, decodes, &tried) == QLDPC_OK);
    for (int f = 0; f < B; f++) {
        CHECK(fp[f] == -1 && !memcmp(kb + f * W, before + f * W, 4 * (size_t)W));
        if (f == 4 || f == 5) CHECK(status[f] == QLDPC_ESIZE && corrected[f] == -1 && decodes[f] == 0);
        else CHECK(status[f] == QLDPC_OK && corrected[f] == 0 && decodes[f] == 1);
    }
    CHECK(tried == 0);
    /* one wrong bit in blocks 0 and 6, junk in block 1, every count 0 through a NULL extra; the optional outputs left out once */
    kb[0] ^= 0x80000000u;
    kb[6 * W + (W - 1)] ^= 1u << (n >= 5 ? 0 : 32 - (int)N);
    for (long w = 0; w < W; w++) kb[W + w] = (uint32_t)rnd() & pl_row_mask(n);
    bits[5] = (int)N;
    memcpy(before, kb, row);
    CHECK(qldpc_polar_recon_decode_flip_host(n, K, pos, kind, maxq, crc_len, poly, prior, pin, E, xp, B, kb, bits, Nf ? syn : NULL, crc, E ? xb : NULL, NULL, T, 0, status,
                                             corrected, fp, decodes, &tried) == QLDPC_OK);
    int open = 0;
    for (int f = 0; f < B; f++) {
        if (f == 4) { CHECK(status[f] == QLDPC_ESIZE && decodes[f] == 0 && fp[f] == -1); continue; }
        CHECK(decodes[f] == 1 || decodes[f] == 2 + T);
        open += decodes[f] > 1;
        CHECK(status[f] == QLDPC_OK || status[f] == QLDPC_EDECODE);
        CHECK((status[f] == QLDPC_OK) == (corrected[f] >= 0) && (fp[f] >= 0 ? status[f] == QLDPC_OK && decodes[f] > 1 : 1));
        if (fp[f] >= 0) CHECK(fp[f] < N && !get(mask, fp[f]));
        if (status[f] != QLDPC_OK) CHECK(fp[f] == -1 && !memcmp(kb + f * W, before + f * W, 4 * (size_t)W));
        if (decodes[f] == 1) CHECK(status[f] == QLDPC_OK && fp[f] == -1);
    }
    CHECK(tried == open);
    /* a resumed call on what is left, without the optional outputs: an OK block and the refused one are left alone */
    memcpy(before, kb, row);
    int left = 0;
    for (int f = 0; f < B; f++) left += status[f] == QLDPC_EDECODE;
    CHECK(qldpc_polar_recon_decode_flip_host(n, K, pos, kind, maxq, crc_len, poly, prior, pin, E, xp, B, kb, bits, Nf ? syn : NULL, crc, E ? xb : NULL, NULL, T, 1, status, NULL,
                                             fp, NULL, &tried) == QLDPC_OK);
    CHECK(tried == left && status[4] == QLDPC_ESIZE);
    for (int f = 0; f < B; f++) CHECK(fp[f] == -1 && !memcmp(kb + f * W, before + f * W, 4 * (size_t)W));      /* the same trials fail again */
    CHECK(qldpc_polar_recon_decode_flip_host(n, K, pos, kind, maxq, crc_len, poly, prior, pin, E, xp, B, kb, bits, Nf ? syn : NULL, crc, E ? xb : NULL, NULL, T, 1, status, NULL,
                                             fp, NULL, NULL) == QLDPC_OK);
    free(pos); free(xp); free(mask); free(rank); free(ka); free(kb); free(before); free(syn); free(crc); free(xb); free(bits); free(extra); free(status); free(corrected);
    free(decodes); free(fp);
    return 0;
}

int main(void)
{
    const int Ts[6] = {1, 2, 4, 8, 16, 32};
    int k = 0;
    for (int n = 1; n <= 9; n++) {
        const long N = 1l << n;
        const int ks[3] = {(int)N, (int)(N / 2), (int)(1 + rnd() % (uint64_t)N)};
        for (int j = 0; j < 3; j++)
            for (int e = 0; e < 3; e++, k++) {                    /* E = 0, 1, K / 2 */
                const int K = ks[j], crc_len = K >= 32 && j == 0 ? 32 : (K >= 11 ? 11 : K), Es[3] = {0, 1, K / 2};
                const uint32_t poly = crc_len == 11 ? 0x621u : (crc_len == 32 ? 0x04C11DB7u : (uint32_t)rnd() & pll_crc_mask(crc_len));
                if (run(n, 0, n % 3 == 0 ? 1 : (n % 3 == 1 ? 31 : 126), K, Es[e], crc_len, poly, Ts[k % 6])) return 1;
                if (run(n, 1, 0, K, Es[e], crc_len, poly, Ts[(k + 3) % 6])) return 1;
            }
    }
    /* the rule on its own */
    CHECK(pfl_flips_pow2(1) && pfl_flips_pow2(32) && !pfl_flips_pow2(0) && !pfl_flips_pow2(-4) && !pfl_flips_pow2(12));
    CHECK(pfl_mag_i8(-127) == 127u && pfl_mag_i8(0) == 0u && pfl_mag_f32(-0.0f) == 0u && pfl_mag_f32(0.0f) == 0u && pfl_mag_f32(-1.5f) == pfl_mag_f32(1.5f));
    CHECK(pfl_mag_f32(1.401298464324817e-45f) == 1u && pfl_mag_f32(2.0f) > pfl_mag_f32(1.5f));
    CHECK(pfl_flip_bit_i8(0) == 1u && pfl_flip_bit_i8(-1) == 0u && pfl_flip_bit_f32(-0.0f) == 1u && pfl_flip_bit_f32(-1.0f) == 0u);
    CHECK(pfl_pass_key(3u, 5, 0, PLD_NO_RANK, 0, 0) == ((uint64_t)3 << 32 | 5u) && pfl_pass_key(3u, 5, 1, PLD_NO_RANK, 0, 0) == PFL_NO_KEY);
    CHECK(pfl_pass_key(3u, 5, 0, 2, 3, 0) == PFL_NO_KEY && pfl_pass_key(3u, 5, 0, 3, 3, 0) != PFL_NO_KEY && pfl_pass_key(3u, 5, 0, 3, 3, ((uint64_t)3 << 32 | 6u)) == PFL_NO_KEY);
    CHECK(pfl_pass_pos(PFL_NO_KEY) == -1 && pfl_pass_next(PFL_NO_KEY) == PFL_NO_KEY && pfl_winner(0u) == -1 && pfl_winner(0x80000000u) == 31 && pfl_winner(6u) == 1);
    /* refusals */
    uint32_t w[4] = {0}, c1[1] = {0};
    int8_t z[8] = {0};
    int st[1], ex[1] = {0}, p2[2] = {1, 1}, p3[3] = {1, 2, 3}, x1[1] = {2}, x4[4] = {1, 2, 3, 4}, sel[32];
    int32_t fp[1];
    CHECK(qldpc_polar_flip_select_host(3, 0, 1, z, w, NULL, NULL, 0, sel) == QLDPC_EINVAL && strstr(msg, "n_flips"));
    CHECK(qldpc_polar_flip_select_host(3, 0, 1, z, w, NULL, NULL, 3, sel) == QLDPC_EINVAL && qldpc_polar_flip_select_host(3, 0, 1, z, w, NULL, NULL, 64, sel) == QLDPC_ESIZE);
    CHECK(qldpc_polar_flip_select_host(0, 0, 1, z, w, NULL, NULL, 1, sel) == QLDPC_ESIZE && qldpc_polar_flip_select_host(3, 2, 1, z, w, NULL, NULL, 1, sel) == QLDPC_EINVAL);
    CHECK(qldpc_polar_flip_select_host(3, 0, -1, z, w, NULL, NULL, 1, sel) == QLDPC_EINVAL && qldpc_polar_flip_select_host(3, 0, 0, NULL, NULL, NULL, NULL, 1, NULL) == QLDPC_OK);
    CHECK(qldpc_polar_flip_select_host(3, 0, 1, NULL, w, NULL, NULL, 1, sel) == QLDPC_EINVAL && qldpc_polar_flip_select_host(3, 0, 1, z, NULL, NULL, NULL, 1, sel) == QLDPC_EINVAL);
    CHECK(qldpc_polar_flip_select_host(3, 0, 1, z, w, NULL, NULL, 1, NULL) == QLDPC_EINVAL && qldpc_polar_flip_select_host(3, 0, 1, z, w, NULL, NULL, 32, sel) == QLDPC_OK);
#define FLIP(E, xp, B, keys, xb, T, resume, status, flip) \
    qldpc_polar_recon_decode_flip_host(3, 3, p3, 0, 31, 3, 3, 1.0, 31.0, E, xp, B, keys, NULL, w, c1, xb, ex, T, resume, status, NULL, flip, NULL, NULL)
    CHECK(FLIP(1, x1, 1, w, w, 0, 0, st, fp) == QLDPC_EINVAL && strstr(msg, "n_flips"));
    CHECK(FLIP(1, x1, 1, w, w, 6, 0, st, fp) == QLDPC_EINVAL && FLIP(1, x1, 1, w, w, 64, 0, st, fp) == QLDPC_ESIZE);
    CHECK(FLIP(1, x1, 1, w, w, 2, 2, st, fp) == QLDPC_EINVAL && FLIP(1, x1, 1, w, w, 2, -1, st, fp) == QLDPC_EINVAL);
    CHECK(FLIP(4, x4, 1, w, w, 2, 0, st, fp) == QLDPC_ESIZE && FLIP(2, p2, 1, w, w, 2, 0, st, fp) == QLDPC_EINVAL);
    CHECK(FLIP(1, x1, 1, NULL, w, 2, 0, st, fp) == QLDPC_EINVAL && FLIP(1, x1, 1, w, NULL, 2, 0, st, fp) == QLDPC_EINVAL);
    CHECK(FLIP(1, x1, 1, w, w, 2, 0, NULL, fp) == QLDPC_EINVAL && FLIP(1, x1, 1, w, w, 2, 0, st, NULL) == QLDPC_EINVAL && strstr(msg, "flip_pos"));
    CHECK(FLIP(1, x1, -1, w, w, 2, 0, st, fp) == QLDPC_EINVAL && FLIP(1, x1, 0, NULL, NULL, 2, 0, NULL, NULL) == QLDPC_OK);
    CHECK(FLIP(0, NULL, 1, w, NULL, 2, 0, st, fp) == QLDPC_OK && FLIP(1, x1, 1, w, w, 32, 0, st, fp) == QLDPC_OK);
    CHECK(qldpc_polar_recon_decode_flip_host(3, 3, p3, 0, 31, 3, 3, 0.0, 31.0, 1, x1, 1, w, NULL, w, c1, w, ex, 2, 0, st, NULL, fp, NULL, NULL) == QLDPC_EINVAL && strstr(msg, "prior"));
    CHECK(qldpc_polar_recon_decode_flip_host(3, 3, p3, 0, 31, 4, 3, 1.0, 31.0, 1, x1, 1, w, NULL, w, c1, w, ex, 2, 0, st, NULL, fp, NULL, NULL) == QLDPC_ESIZE);
    CHECK(qldpc_polar_recon_decode_flip_host(3, 3, p3, 0, 31, 3, 3, 1.0, 31.0, 1, x1, 1, w, NULL, NULL, c1, w, ex, 2, 0, st, NULL, fp, NULL, NULL) == QLDPC_EINVAL);
    CHECK(qldpc_polar_recon_decode_flip_host(3, 3, p3, 0, 31, 3, 3, 1.0, 31.0, 1, x1, 1, w, NULL, w, NULL, w, ex, 2, 0, st, NULL, fp, NULL, NULL) == QLDPC_EINVAL);
    printf("polar flip: sanitizer pass ok\n");
    return 0;
}
