/*
 * qldpc_recon_tag_host.c -- the host side of the sessions' keyed tag that needs no device: the mirror of the chunked Horner and its fold
 * (qldpc_recon_tag_core.h, what rk_verify_tag and rk_tag run) for any power-of-two lane count, the whole verdict of rk_verify_tag on host pointers
 * with the serial CRC-32 of qldpc_recon_core.h (what qldpc_crc32_words computes) in place of the chunked fold.
 */
#include <stdlib.h>
#include <string.h>

#include "../../include/qldpc.h"
#include "qldpc_graph.h"
#include "qldpc_recon_tag_core.h"

#define RT_HOST_LANES 256          /* the kernels' RK_LANES */
#define RT_HOST_MAX_LANES (1 << 20)

int qldpc_recon_tag_host(const uint32_t *key_words, int key_bits, const uint32_t hash_key[2], int lanes, uint32_t tag[2])
{
    if (key_bits <= 0 || key_bits > HB_MAX_BITS) { qldpc_set_error("recon_tag_host: key_bits=%d", key_bits); return QLDPC_ESIZE; }
    if (lanes < 1 || lanes > RT_HOST_MAX_LANES || (lanes & (lanes - 1))) { qldpc_set_error("recon_tag_host: lanes=%d is not a power of two in 1 .. %d", lanes, RT_HOST_MAX_LANES); return QLDPC_EINVAL; }
    if (!key_words || !hash_key || !tag) return QLDPC_EINVAL;
    uint64_t *part = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)lanes);
    if (!part) return QLDPC_ENOMEM;
    ph_store_tag(tag, rt_tag_chunked(key_words, key_bits, ph_key(hash_key[0], hash_key[1]), lanes, part));
    free(part);
    return QLDPC_OK;
}

int qldpc_recon_verify_tag_host(int n, int n_keys, int Wk, int Wn, const uint32_t *out_rows, const uint32_t *keys, const int *key_bits, const uint32_t *crc_want,
                                const int *ok, const int *iters, const uint32_t *hash_keys, size_t hash_key_stride, uint32_t *res_keys, int *res, uint32_t *tags)
{
    if (!out_rows || !keys || !key_bits || !crc_want || !ok || !iters || !hash_keys || !res_keys || !res || !tags) return QLDPC_EINVAL;
    if (n_keys < 1 || n_keys > RT_MAX_KEYS) { qldpc_set_error("recon_verify_tag_host: n_keys=%d, outside 1 .. %d", n_keys, RT_MAX_KEYS); return QLDPC_EINVAL; }
    if (n < 0 || Wk < 1 || Wn < Wk || (hash_key_stride && hash_key_stride < 2 * (size_t)n_keys)) {
        qldpc_set_error("recon_verify_tag_host: n=%d (not negative), key row of %d words (at least 1) in decoded rows of %d, hash-key rows %zu words apart (0 or at least %d)",
                        n, Wk, Wn, hash_key_stride, 2 * n_keys);
        return QLDPC_ESIZE;
    }
    for (int b = 0; b < n; b++)
        if (key_bits[b] < 1 || key_bits[b] > 32 * Wk) {
            qldpc_set_error("recon_verify_tag_host: block %d has key_bits=%d, outside 1 .. %d (key rows of %d words)", b, key_bits[b], 32 * Wk, Wk);
            return QLDPC_ESIZE;
        }
    uint32_t table[256];
    uint64_t part[RT_HOST_LANES];
    for (uint32_t i = 0; i < 256; i++) table[i] = crc_table_entry(i);
    for (int b = 0; b < n; b++) {
        const int kb = key_bits[b], nw = (kb + 31) / 32;
        const uint32_t *row = out_rows + (size_t)b * Wn, *old = keys + (size_t)b * Wk, *hk = hash_keys + (size_t)b * hash_key_stride;
        uint32_t *dst = res_keys + (size_t)b * Wk, *tg = tags + (size_t)b * 2 * (size_t)n_keys;
        const uint32_t crc = crc_serial(row, kb, table);
        const int good = ok[b] && crc == crc_want[b];
        int flips = 0;
        for (int i = 0; i < nw; i++) {
            const uint32_t m = tail_mask(i, nw, kb), x = row[i] & m;
            flips += __builtin_popcount((old[i] & m) ^ x);
            dst[i] = good ? x : old[i];
        }
        res[b] = good ? QLDPC_OK : QLDPC_EDECODE;
        res[(size_t)n + b] = good ? flips : 0;
        res[2 * (size_t)n + b] = iters[b];
        res[3 * (size_t)n + b] = (int)crc;
        for (int q = 0; q < n_keys; q++)
            ph_store_tag(tg + 2 * q, good ? rt_tag_chunked(row, kb, ph_key(hk[2 * q], hk[2 * q + 1]), RT_HOST_LANES, part) : 0ull);
    }
    return QLDPC_OK;
}
