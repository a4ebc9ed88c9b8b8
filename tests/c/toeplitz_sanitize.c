/* Sanitizer pass over the arithmetic of the Toeplitz hash (qldpc_toeplitz_core.h, no HIP): every lane of the edge sizes through
 * tz_lane_words, in tiles, against a bit-serial loop.  Built with -fsanitize=address,undefined by tests/test_toeplitz.py */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../qcrypto-ldpc_amd/csrc/qldpc_toeplitz_core.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

static uint64_t rng_state = 0x243f6a8885a308d3ull;
static uint32_t rng32(void)
{
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return (uint32_t)((z ^ (z >> 31)) >> 16);
}

static int bit(const uint32_t *w, uint32_t k) { return (int)((w[k >> 5] >> (31 - (k & 31))) & 1u); }

/* as qldpc_toeplitz_host: the key in tiles, the window of a tile rebuilt from exactly the seed words the block owns */
static void hash_tiles(const uint32_t *key, int n, const uint32_t *seed, int m, uint32_t tile, uint32_t *out)
{
    const uint32_t nw = ((uint32_t)n + 31u) / 32u, ow = ((uint32_t)m + 31u) / 32u, sw = tz_seed_words(n, m);
    uint32_t *win = malloc(4 * ((size_t)(tile < nw ? tile : nw) + 1));      /* exactly what a tile reads: one word past is an ASan report */
    for (uint32_t w = 0; w < ow; w++) {
        uint32_t acc[32] = {0}, word = 0;
        for (uint32_t j0 = 0; j0 < nw; j0 += tile) {
            const uint32_t tw = nw - j0 < tile ? nw - j0 : tile;
            for (uint32_t k = 0; k <= tw; k++) win[k] = w + j0 + k < sw ? tz_brev(seed[w + j0 + k]) : 0u;
            for (uint32_t s = 0; s < 32; s++) acc[s] = tz_lane_words(acc[s], key, j0, tw, nw - 1u, tz_tail_mask(n), win, s);
        }
        for (uint32_t s = 0; s < 32; s++)
            if (32u * w + s < (uint32_t)m) word |= tz_parity(acc[s]) << (31 - s);
        out[w] = word;
    }
    free(win);
}

int main(void)
{
    static const int ns[] = {1, 31, 32, 33, 63, 64, 65, 1000, 4097}, ms[] = {1, 31, 32, 33, 63, 64, 65, 257};
    static const uint32_t tiles[] = {1, 2, 7, 64, 2048};
    CHECK(tz_brev(1u) == 0x80000000u && tz_brev(0x80000001u) == 0x80000001u && tz_brev(0x12345678u) == 0x1e6a2c48u);
    CHECK(tz_window(0xdeadbeefu, 0x12345678u, 0) == 0xdeadbeefu && tz_window(0xdeadbeefu, 0x12345678u, 31) == ((0x12345678u << 1) | 1u));
    CHECK(tz_tail_mask(32) == 0xffffffffu && tz_tail_mask(1) == 0x80000000u && tz_tail_mask(33) == 0x80000000u);
    CHECK(tz_seed_words(1, 1) == 1 && tz_seed_words(32, 1) == 1 && tz_seed_words(32, 2) == 2 && tz_seed_words(0, 5) == 0 && tz_seed_words(5, 0) == 0);
    CHECK(tz_seed_words(TZ_MAX_BITS, TZ_MAX_BITS) == (1u << 20));
    int cases = 0;
    for (size_t a = 0; a < sizeof(ns) / sizeof(*ns); a++)
        for (size_t b = 0; b < sizeof(ms) / sizeof(*ms); b++) {
            const int n = ns[a], m = ms[b];
            const uint32_t nw = ((uint32_t)n + 31u) / 32u, ow = ((uint32_t)m + 31u) / 32u, sw = tz_seed_words(n, m);
            uint32_t *key = malloc(4 * (size_t)nw), *seed = malloc(4 * (size_t)sw), *ref = calloc(ow, 4), *got = malloc(4 * (size_t)ow);
            for (uint32_t k = 0; k < nw; k++) key[k] = rng32();      /* garbage past n and past n + m - 1 stays in */
            for (uint32_t k = 0; k < sw; k++) seed[k] = rng32();
            for (int i = 0; i < m; i++) {
                int y = 0;
                for (int j = 0; j < n; j++) y ^= bit(key, (uint32_t)j) & bit(seed, (uint32_t)(i + j));
                ref[i >> 5] |= (uint32_t)y << (31 - (i & 31));
            }
            for (size_t t = 0; t < sizeof(tiles) / sizeof(*tiles); t++) {
                hash_tiles(key, n, seed, m, tiles[t], got);
                if (memcmp(got, ref, 4 * (size_t)ow)) { fprintf(stderr, "FAILED n=%d m=%d tile=%u\n", n, m, tiles[t]); return 1; }
                cases++;
            }
            free(key); free(seed); free(ref); free(got);
        }
    printf("sanitizer pass ok: %d cases\n", cases);
    return 0;
}
