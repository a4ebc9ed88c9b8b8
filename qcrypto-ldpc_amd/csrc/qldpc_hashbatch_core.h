/*
 * qldpc_hashbatch_core.h -- what the batch contexts of the privacy-amplification hashes (qldpc_privamp_blocks*, qldpc_toeplitz_blocks*) share
 * before anything touches the device, plain C, compiled on its own by the CPU suite (tests/c/hashbatch_sanitize.c), each piece stated once:
 * the limits of a context and their check, the argument checks of a call, the row layout of its blocks, the tail mask.
 * The hashes differ in what they call a block's two sizes (workbits / final_bits, key_bits / out_bits): a check takes those words from its
 * caller (hb_names) and leaves the reason of a refusal, the block named, in qldpc_last_error().
 */
#ifndef QLDPC_HASHBATCH_CORE_H
#define QLDPC_HASHBATCH_CORE_H

#include <stddef.h>
#include <stdint.h>

#include "../../include/qldpc.h"
#include "qldpc_graph.h"

#if defined(__HIPCC__)
#define HB_FN __host__ __device__ static inline
#else
#define HB_FN static inline
#endif

#define HB_MAX_BLOCKS 65535        /* blocks are the y dimension of the grid */
#define HB_MAX_BITS (1 << 24)      /* key and output bits of a block (qldpc.h states it) */

HB_FN uint32_t hb_words(int bits) { return ((uint32_t)bits + 31u) / 32u; }
/* the bits of the last word of a row of `bits` bits, MSB-first */
HB_FN uint32_t hb_tail_mask(int bits) { return (bits & 31) ? 0xFFFFFFFFu << (32 - (bits & 31)) : 0xFFFFFFFFu; }

typedef struct hb_limits { int max_blocks, max_key_bits, max_out_bits; } hb_limits;
typedef struct hb_names { const char *key_bits, *out_bits; } hb_names;
/* words of a block's third row (the Toeplitz seed); a NULL function: the hash has no such row */
typedef uint32_t (*hb_extra_fn)(int key_bits, int out_bits);

/* extra_words: the third row of a block of the largest sizes.  The 16 words per block cover the descriptor rows in front of the payload */
static inline int hb_limits_check(const hb_limits *l, uint64_t extra_words, const char *who, const hb_names *nm)
{
    if (l->max_blocks > HB_MAX_BLOCKS) { qldpc_set_error("%s: max_blocks=%d (up to %d)", who, l->max_blocks, HB_MAX_BLOCKS); return QLDPC_ESIZE; }
    if (l->max_blocks < 1 || l->max_key_bits < 1 || l->max_out_bits < 0 || l->max_key_bits > HB_MAX_BITS || l->max_out_bits > HB_MAX_BITS)
        qldpc_set_error("%s: max_blocks=%d max_key_bits=%d max_%s=%d (bits up to %d)", who, l->max_blocks, l->max_key_bits, nm->out_bits, l->max_out_bits, HB_MAX_BITS);
    else if ((uint64_t)l->max_blocks * (hb_words(l->max_key_bits) + extra_words + hb_words(l->max_out_bits) + 16) >= (1ull << 31))
        qldpc_set_error("%s: %d blocks of %d -> %d bits pass 2^31 staged words", who, l->max_blocks, l->max_key_bits, l->max_out_bits);
    else return QLDPC_OK;
    return QLDPC_ESIZE;
}

/* the arguments of both call forms, before anything is written; other_null: another argument array of the call is NULL */
static inline int hb_check_blocks(const hb_limits *l, int n, const int *key_bits, const int *out_bits, int other_null, const char *who, const hb_names *nm)
{
    if (n < 0) return QLDPC_EINVAL;
    if (n > l->max_blocks) { qldpc_set_error("%s: %d blocks, the context holds %d", who, n, l->max_blocks); return QLDPC_ESIZE; }
    if (n == 0) return QLDPC_OK;
    if (!key_bits || !out_bits || other_null) { qldpc_set_error("%s: NULL argument array", who); return QLDPC_EINVAL; }
    for (int i = 0; i < n; i++) {
        if (key_bits[i] <= 0 || out_bits[i] < 0) qldpc_set_error("%s: block %d: %s=%d %s=%d", who, i, nm->key_bits, key_bits[i], nm->out_bits, out_bits[i]);
        else if (key_bits[i] > l->max_key_bits) qldpc_set_error("%s: block %d: %s=%d, the context holds %d", who, i, nm->key_bits, key_bits[i], l->max_key_bits);
        else if (out_bits[i] > l->max_out_bits) qldpc_set_error("%s: block %d: %s=%d, the context holds %d", who, i, nm->out_bits, out_bits[i], l->max_out_bits);
        else continue;
        return QLDPC_ESIZE;
    }
    return QLDPC_OK;
}

/* host form: the row pointers of every block; extra_rows NULL: the hash has none; a block of 0 output bits needs no output row */
static inline int hb_check_rows(int n, const int *out_bits, const uint32_t *const *key_rows, const uint32_t *const *extra_rows, uint32_t *const *out_rows, const char *who)
{
    for (int i = 0; i < n; i++) {
        const char *what = !key_rows[i] ? "key" : (extra_rows && !extra_rows[i]) ? "seed" : (!out_rows[i] && out_bits[i] > 0) ? "output" : NULL;
        if (what) { qldpc_set_error("%s: block %d: NULL %s row", who, i, what); return QLDPC_EINVAL; }
    }
    return QLDPC_OK;
}

/* device form: rows `key`, `out` and `extra` words apart; extra == 0: every block reads the one row at the base */
typedef struct hb_strides { size_t key, out, extra; } hb_strides;

static inline int hb_check_strides(int n, const int *key_bits, const int *out_bits, hb_extra_fn extra, const hb_strides *st, const char *who, const hb_names *nm)
{
    for (int i = 0; i < n; i++) {
        if (hb_words(key_bits[i]) > st->key) qldpc_set_error("%s: block %d: %s=%d pass a key row of %zu words", who, i, nm->key_bits, key_bits[i], st->key);
        else if (extra && st->extra && extra(key_bits[i], out_bits[i]) > st->extra) qldpc_set_error("%s: block %d: %d -> %d bits pass a seed row of %zu words", who, i, key_bits[i], out_bits[i], st->extra);
        else if (hb_words(out_bits[i]) > st->out) qldpc_set_error("%s: block %d: %s=%d pass an output row of %zu words", who, i, nm->out_bits, out_bits[i], st->out);
        else continue;
        return QLDPC_ESIZE;
    }
    return QLDPC_OK;
}

/* the rows of block i, in words from the key / output / extra base of the call */
typedef struct hb_row { uint32_t key_words, out_words, extra_words; uint64_t key_off, out_off, extra_off; } hb_row;
/* the words of the three areas when packed (extra_shared: of the longest extra row) and the widest output row of the call, which gives the grid */
typedef struct hb_sums { size_t key_words, out_words, extra_words; uint32_t widest_out; } hb_sums;

/* strides NULL: rows packed one after the other (host form), and with extra_shared every block's extra row at 0; else rows a stride apart */
static inline hb_sums hb_layout(int n, const int *key_bits, const int *out_bits, hb_extra_fn extra, const hb_strides *strides, int extra_shared, hb_row *rows)
{
    hb_sums s = {0, 0, 0, 0};
    size_t longest = 0;
    for (int i = 0; i < n; i++) {
        hb_row *r = &rows[i];
        r->key_words = hb_words(key_bits[i]);
        r->out_words = hb_words(out_bits[i]);
        r->extra_words = extra ? extra(key_bits[i], out_bits[i]) : 0u;
        r->key_off = strides ? (uint64_t)i * strides->key : s.key_words;
        r->out_off = strides ? (uint64_t)i * strides->out : s.out_words;
        r->extra_off = strides ? (uint64_t)i * strides->extra : extra_shared ? 0 : s.extra_words;
        s.key_words += r->key_words; s.out_words += r->out_words; s.extra_words += r->extra_words;
        if (r->extra_words > longest) longest = r->extra_words;
        if (r->out_words > s.widest_out) s.widest_out = r->out_words;
    }
    if (extra_shared) s.extra_words = longest;
    return s;
}

#endif /* QLDPC_HASHBATCH_CORE_H */
