/* Sanitizer pass over the error-verification hash on the host (qldpc_polyhash_core.h and the mirror qldpc_polyhash_host.c, no HIP): the field
 * arithmetic against unsigned __int128, the split of a tile into fast and checked rows and the groups a lane may load at its edges, the doubling table, and the mirror at
 * every lane count and tile against the Horner loop of the definition.  Every buffer is malloc'ed at its exact size, at each of the four
 * offsets from a 16-byte boundary, so a fast row that read past a key, or in front of it, would be caught.
 * Built with -fsanitize=address,undefined by tests/test_polyhash_host.py */
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "qldpc_polyhash_core.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)
#define COUNT(a) ((int)(sizeof(a) / sizeof((a)[0])))

static char msg[256];
void qldpc_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, sizeof(msg), fmt, ap);
    va_end(ap);
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd(void)
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}

static uint64_t mul_ref(uint64_t a, uint64_t b) { return (uint64_t)((unsigned __int128)a * b % PH_P); }

/* the definition: h = 0; for every coefficient: h = (h + c) k */
static uint64_t tag_ref(const uint32_t *w, int n, uint64_t k)
{
    const uint32_t W = ((uint32_t)n + 31u) / 32u;
    uint64_t h = 0;
    for (uint32_t j = 0; j <= W; j++) {
        uint32_t c = j < W ? w[j] : (uint32_t)n;
        if (j + 1 == W && (n & 31)) c &= 0xFFFFFFFFu << (32 - (n & 31));
        h = mul_ref((h + c) % PH_P, k);
    }
    return h;
}

static int arithmetic(long *products)
{
    const uint64_t edge[] = {0, 1, 2, 0xFFFFFFFFull, 0x100000000ull, 0x1FFFFFFFull, 0x20000000ull, PH_P - 1, PH_P - 2, PH_P >> 1, 0x1FFFFFFF00000000ull, 0x1FFFFFFFFFFFFFFEull};
    for (int i = 0; i < COUNT(edge); i++)
        for (int j = 0; j < COUNT(edge); j++, ++*products) {
            CHECK(ph_mul(edge[i], edge[j]) == mul_ref(edge[i], edge[j]));
            CHECK(ph_mul_add(edge[i], edge[j], PH_P - 1) == (mul_ref(edge[i], edge[j]) + PH_P - 1) % PH_P);
            CHECK(ph_add(edge[i], edge[j]) == (edge[i] + edge[j]) % PH_P);
        }
    for (int i = 0; i < 200000; i++, ++*products) {
        const uint64_t a = rnd() % PH_P, b = rnd() % PH_P, c = rnd() % PH_P;
        CHECK(ph_mul_add(a, b, c) == (mul_ref(a, b) + c) % PH_P);
    }
    CHECK(ph_fold(~0ull) == (~0ull) % PH_P && ph_fold(PH_P) == 0 && ph_fold(PH_P + 1) == 1 && ph_fold(0) == 0);
    CHECK(ph_key(0xFFFFFFFFu, 0xFFFFFFFFu) == 0 && ph_key(0x1FFFFFFFu, 0xFFFFFFFFu) == 0 && ph_key(0x20000000u, 0) == 0);
    CHECK(ph_key(0x1FFFFFFFu, 0xFFFFFFFEu) == PH_P - 1 && ph_key(0xFFFFFFFFu, 0xFFFFFFFEu) == PH_P - 1 && ph_key(0x01234567u, 0x89ABCDEFu) == 0x0123456789ABCDEFull);
    CHECK(ph_pow(3, 0) == 1 && ph_pow(3, 5) == 243 && ph_pow(PH_P - 1, 2) == 1 && ph_pow(PH_P - 1, 3) == PH_P - 1 && ph_pow(2, 61) == 1);
    uint32_t two[2];
    ph_store_tag(two, 0x1234567890ABCDEFull);
    CHECK(two[0] == 0x12345678u && two[1] == 0x90ABCDEFu);
    return 0;
}

static int tables(void)
{
    static const uint32_t ns[] = {1, 2, 3, 4, 5, 12, 256, 1000, 1024};
    static const uint32_t lanes[] = {1, 3, 256};
    for (int a = 0; a < COUNT(ns); a++)
        for (int l = 0; l < COUNT(lanes); l++) {
            const uint32_t n = ns[a];
            const uint64_t x = rnd() % PH_P;
            uint64_t *tab = malloc(sizeof(uint64_t) * (n + 1));
            tab[0] = 1; tab[1] = x;
            for (uint32_t i = 2; i <= n; i++) tab[i] = ~0ull;
            for (uint32_t half = 1; half < n; half *= 2)
                for (uint32_t t = 0; t < lanes[l]; t++) ph_pow_step(tab, half, n, t, lanes[l]);
            uint64_t p = 1;
            for (uint32_t i = 0; i <= n; i++, p = mul_ref(p, x)) CHECK(tab[i] == p);
            free(tab);
        }
    return 0;
}

/* every position of a tile is met exactly once, by a fast row only where a whole key word lies, and the weights are the exponents */
static int splits(long *tiles_checked)
{
    static const uint32_t Ts[] = {4, 8, 12, 1024};
    for (int ti = 0; ti < COUNT(Ts); ti++)
        for (uint32_t a = 0; a < 4; a++)
            for (uint32_t m = 1; m <= 3 * Ts[ti] + 5; m += (Ts[ti] > 100 ? 97 : 1))
                for (uint32_t cut = 0; cut <= 2 && cut <= m; cut++, ++*tiles_checked) {
                    const uint32_t T = Ts[ti], plain = m - cut;
                    const ph_split sp = ph_rows(m, plain, a, T);
                    CHECK(sp.rows * T >= m + a && (sp.rows - 1) * T < m + a && sp.fast <= sp.rows && sp.rows - sp.fast <= 2);
                    for (uint32_t i = 0; i < sp.fast; i++) CHECK((i + 1) * T - a <= plain);
                    /* a group is loaded exactly where one of its four positions holds a word that lies in memory (here: the first `avail`) */
                    for (uint32_t p0 = 0; p0 < sp.rows * T; p0 += 4) {
                        int any = 0;
                        for (uint32_t s4 = 0; s4 < 4; s4++) any |= p0 + s4 >= a && p0 + s4 - a < plain;
                        CHECK(ph_group_has_word(p0, a, plain) == any);
                    }
                    for (uint32_t u = 0; u < T; u++) {
                        uint32_t last = 0, have = 0;
                        for (uint32_t i = 0; i < sp.rows; i++)
                            if (i * T + u >= a && i * T + u - a < m) { last = i * T + u - a; have = 1; }
                        if (have) CHECK(ph_weight_exp(sp.r, u, T) == m - 1 - last);
                        else CHECK(ph_weight_exp(sp.r, u, T) < T);
                    }
                }
    return 0;
}

static int mirror(long *tags_checked)
{
    static const int coefs[] = {255, 256, 257, 1023, 1024, 1025, 2047, 2049, 3072};
    static const int lanes[] = {1, 2, 3, 64, 256, 1000};
    static const int tiles[] = {0, 1024, 8192};
    int bits[8 + 3 * COUNT(coefs) + 1] = {1, 31, 32, 33, 63, 64, 65, 70}, nb = 8;
    for (int c = 0; c < COUNT(coefs); c++)
        for (int d = -1; d <= 1; d++) bits[nb++] = 32 * coefs[c] - 32 + d;
    bits[nb++] = 100000;
    const uint64_t keys[] = {0, 1, 2, PH_P - 1, PH_P, 1ull << 61, ~0ull, rnd()};
    for (int b = 0; b < nb; b++) {
        const uint32_t W = ((uint32_t)bits[b] + 31u) / 32u, shift = (uint32_t)b & 3u;
        /* the key at each offset from a 16-byte boundary, its last word the last of the allocation */
        uint32_t *raw = malloc(4 * ((size_t)W + shift)), *w = raw + shift;
        for (uint32_t j = 0; j < W; j++) w[j] = (b & 1) ? 0xFFFFFFFFu : (uint32_t)rnd();
        for (int ki = 0; ki < COUNT(keys); ki++) {
            const uint32_t hk[2] = {(uint32_t)(keys[ki] >> 32), (uint32_t)keys[ki]};
            const uint64_t want = tag_ref(w, bits[b], ph_key(hk[0], hk[1]));
            for (int l = 0; l < COUNT(lanes); l++)
                for (int t = 0; t < COUNT(tiles); t++, ++*tags_checked) {
                    uint32_t *tag = malloc(8);
                    CHECK(qldpc_polyhash_host(w, bits[b], hk, lanes[l], tiles[t], tag) == QLDPC_OK);
                    CHECK((((uint64_t)tag[0] << 32) | tag[1]) == want && want < PH_P);
                    free(tag);
                }
        }
        free(raw);
    }
    return 0;
}

static int refusals(void)
{
    uint32_t w[1] = {0}, hk[2] = {1, 2}, tag[2] = {7, 7};
    CHECK(qldpc_polyhash_host(w, 0, hk, 1, 0, tag) == QLDPC_ESIZE && qldpc_polyhash_host(w, HB_MAX_BITS + 1, hk, 1, 0, tag) == QLDPC_ESIZE);
    CHECK(qldpc_polyhash_host(w, 1, hk, 0, 0, tag) == QLDPC_EINVAL && qldpc_polyhash_host(w, 1, hk, 1, 512, tag) == QLDPC_EINVAL && strstr(msg, "tile_words=512"));
    CHECK(qldpc_polyhash_host(NULL, 1, hk, 1, 0, tag) == QLDPC_EINVAL && qldpc_polyhash_host(w, 1, NULL, 1, 0, tag) == QLDPC_EINVAL && qldpc_polyhash_host(w, 1, hk, 1, 0, NULL) == QLDPC_EINVAL);
    CHECK(tag[0] == 7 && tag[1] == 7);
    CHECK(qldpc_polyhash_leaked_bits(1) == 61 && qldpc_polyhash_leaked_bits(4) == 244 && qldpc_polyhash_leaked_bits(0) == 0 && qldpc_polyhash_leaked_bits(5) == 0);
    CHECK(qldpc_polyhash_bound_log2(32, 1) < -59.4 && qldpc_polyhash_bound_log2(32, 1) > -59.5 && qldpc_polyhash_bound_log2(0, 1) == 0.0 && qldpc_polyhash_bound_log2(32, 5) == 0.0);
    CHECK(ph_tile_words(0) == 8192 && ph_tile_words(8192) == 8192 && ph_tile_words(1024) == 1024 && ph_tile_words(-1) == 0 && ph_tile_words(4096) == 0);
    return 0;
}

int main(void)
{
    long products = 0, tiles_checked = 0, tags_checked = 0;
    if (arithmetic(&products) || tables() || splits(&tiles_checked) || mirror(&tags_checked) || refusals()) return 1;
    CHECK(tags_checked == 36L * 8 * 6 * 3);
    printf("sanitizer pass ok: %ld products, %ld tile splits, %ld tags\n", products, tiles_checked, tags_checked);
    return 0;
}
