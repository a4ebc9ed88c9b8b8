/*
 * qldpc_polyhash_host.c -- the host side of the error-verification hash that needs no device: the mirror of the two kernels of
 * qldpc_polyhash.hip over the functions of qldpc_polyhash_core.h (the same tiles, virtual lanes, fast and checked rows, power tables and
 * fold of the partials, for any lane count), the field arithmetic for tests, and the bound and the leak of a tag.
 */
#include <math.h>
#include <stdlib.h>

#include "../../include/qldpc.h"
#include "qldpc_graph.h"
#include "qldpc_polyhash_core.h"

#define PH_HOST_MAX_LANES (1 << 20)

/* tab[i] = x^i, i <= n, by the doubling steps of the kernels */
static void ph_table_host(uint64_t *tab, uint32_t n, uint64_t x)
{
    tab[0] = 1ull;
    tab[1] = x;
    for (uint32_t half = 1; half < n; half *= 2) ph_pow_step(tab, half, n, 0, 1);
}

/* the partial of one tile: m coefficients from `base` on, T virtual lanes, tab of T + 1 entries */
static uint64_t ph_tile_host(const uint32_t *key, uint32_t key_words, uint32_t mask, uint32_t key_bits, uint32_t base, uint32_t m,
                             uint64_t k, uint32_t T, uint64_t *tab)
{
    const uint32_t a = ph_shift(key + base), avail = ph_tile_avail(key_words, base, m);
    const ph_split sp = ph_rows(m, ph_tile_plain(key_words, base, m), a, T);
    ph_table_host(tab, T, k);
    const uint64_t X = tab[T];
    uint64_t sum = 0;
    for (uint32_t u = 0; u < T; u++) {
        uint64_t h = 0;
        for (uint32_t i = 0; i < sp.rows; i++) {
            const uint32_t pos = i * T + u;
            /* what a lane's load gives: the key word where one lies (the host reads nothing else), 0 in front of the tile */
            const uint32_t word = pos >= a && pos - a < avail ? key[base + pos - a] : 0u;
            h = i < sp.fast ? ph_mul_add(h, X, word) : ph_checked(h, X, word, base, pos, a, m, key_words, mask, key_bits);
        }
        sum = ph_add(sum, ph_mul(h, tab[ph_weight_exp(sp.r, u, T)]));
    }
    return sum;
}

int qldpc_polyhash_host(const uint32_t *key_words, int key_bits, const uint32_t hash_key[2], int lanes, int tile_words, uint32_t tag[2])
{
    const uint32_t tile = ph_tile_words(tile_words);
    if (key_bits <= 0 || key_bits > HB_MAX_BITS) { qldpc_set_error("polyhash_host: key_bits=%d", key_bits); return QLDPC_ESIZE; }
    if (lanes < 1 || lanes > PH_HOST_MAX_LANES || !tile) { qldpc_set_error("polyhash_host: lanes=%d tile_words=%d", lanes, tile_words); return QLDPC_EINVAL; }
    if (!key_words || !hash_key || !tag) return QLDPC_EINVAL;
    const uint32_t W = hb_words(key_bits), coefs = ph_coefs(key_bits), tiles = ph_tiles(coefs, tile), mask = hb_tail_mask(key_bits);
    const uint32_t L = (uint32_t)lanes, T = PH_LANE_WORDS * L;
    const uint64_t k = ph_key(hash_key[0], hash_key[1]);
    uint64_t *tab = (uint64_t *)malloc(sizeof(uint64_t) * ((size_t)T + 1)), *part = (uint64_t *)calloc(tiles, sizeof(uint64_t));
    if (!tab || !part) { free(tab); free(part); return QLDPC_ENOMEM; }
    for (uint32_t tau = 0; tau < tiles; tau++)
        part[tau] = ph_tile_host(key_words, W, mask, (uint32_t)key_bits, tau * tile, ph_tile_len(coefs, tile, tau), k, T, tab);
    uint64_t E = part[0];
    if (tiles > 1) {                                             /* the fold kernel: the tiles before the last by L lanes in Y = k^tile */
        const uint32_t m = tiles - 1u, r = m % L;
        ph_table_host(tab, L, ph_pow(k, tile));
        const uint64_t X = tab[L];
        uint64_t sum = 0;
        for (uint32_t u = 0; u < L; u++) {
            uint64_t h = 0;
            for (uint32_t j = u; j < m; j += L) h = ph_mul_add(h, X, part[j]);
            sum = ph_add(sum, ph_mul(h, tab[ph_weight_exp(r, u, L)]));
        }
        E = ph_mul_add(sum, ph_pow(k, ph_tile_len(coefs, tile, m)), part[m]);
    }
    ph_store_tag(tag, ph_mul(E, k));
    free(tab);
    free(part);
    return QLDPC_OK;
}

uint64_t qldpc_polyhash_mul_host(uint64_t a, uint64_t b) { return ph_mul(ph_fold(a), ph_fold(b)); }

uint64_t qldpc_polyhash_key_host(uint32_t hi, uint32_t lo) { return ph_key(hi, lo); }

double qldpc_polyhash_bound_log2(int key_bits, int n_keys)
{
    if (key_bits <= 0 || n_keys < 1 || n_keys > PH_MAX_KEYS) return 0.0;
    return (double)n_keys * (log2((double)hb_words(key_bits) + 2.0) - 61.0);
}

int qldpc_polyhash_leaked_bits(int n_keys) { return n_keys >= 1 && n_keys <= PH_MAX_KEYS ? 61 * n_keys : 0; }
