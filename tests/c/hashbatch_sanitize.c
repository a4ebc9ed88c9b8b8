/* Sanitizer pass over what the batch contexts of the two privacy-amplification hashes share on the host (qldpc_hashbatch_core.h, no HIP): the
 * row layout against a naive restatement that works one block at a time from the definitions (no running state), the limit checks at their
 * edges, the argument checks of a call, the tail mask.  Every buffer is malloc'ed at its exact size.
 * Built with -fsanitize=address,undefined by tests/test_hashbatch_host.py */
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "qldpc_hashbatch_core.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)
#define COUNT(a) ((int)(sizeof(a) / sizeof((a)[0])))

static const hb_names names = {"workbits", "final_bits"};

/* the library's error text, kept here: the header leaves the reason of a refusal in it */
static char msg[256];
void qldpc_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(msg, sizeof(msg), fmt, ap);
    va_end(ap);
}

/* a third row as the Toeplitz hash has it: key_bits + out_bits - 1 bits, none for a block that asks for nothing */
static uint32_t seed_words(int key_bits, int out_bits) { return key_bits > 0 && out_bits > 0 ? (uint32_t)((key_bits + out_bits - 1 + 31) / 32) : 0u; }

static size_t words_of(int bits) { return ((size_t)bits + 31) / 32; }

/* block i of a call, from the definitions alone: a packed row starts where the rows of the blocks before it end */
static int naive_row(int n, const int *kb, const int *ob, int with_seed, const hb_strides *strides, int shared, int i, const hb_row *got)
{
    size_t koff = 0, ooff = 0, soff = 0;
    for (int j = 0; j < i; j++) { koff += words_of(kb[j]); ooff += words_of(ob[j]); soff += with_seed ? seed_words(kb[j], ob[j]) : 0; }
    if (strides) { koff = (size_t)i * strides->key; ooff = (size_t)i * strides->out; soff = (size_t)i * strides->extra; }
    else if (shared) soff = 0;
    CHECK(i < n);
    CHECK(got->key_words == words_of(kb[i]) && got->out_words == words_of(ob[i]) && got->extra_words == (with_seed ? seed_words(kb[i], ob[i]) : 0u));
    CHECK(got->key_off == koff && got->out_off == ooff && got->extra_off == soff);
    return 0;
}

static int layouts(long *rows_checked)
{
    static const int ns[] = {0, 1, 2, 5}, kbs[] = {1, 31, 32, 33, 1000}, obs[] = {0, 1, 32, 33, 500};
    static const hb_strides apart = {32, 16, 48};                /* >= the longest rows above: 1000 -> 32, 500 -> 16, 1499 -> 47 words */
    static const hb_strides apart_one_seed = {40, 17, 0};
    const hb_strides *forms[] = {NULL, &apart, &apart_one_seed};
    for (int a = 0; a < COUNT(ns); a++)
        for (int rk = 0; rk < 5; rk++)
            for (int ro = 0; ro < 5; ro++)
                for (int f = 0; f < 3; f++)
                    for (int seed = 0; seed < 3; seed++) {       /* 0: no third row, 1: one per block, 2: one shared (packed form) */
                        const int n = ns[a], shared = seed == 2;
                        if (shared && forms[f]) continue;       /* rows a stride apart share by a stride of 0 */
                        int *kb = malloc(sizeof(int) * (size_t)n), *ob = malloc(sizeof(int) * (size_t)n);
                        hb_row *rows = malloc(sizeof(hb_row) * (size_t)n);
                        for (int i = 0; i < n; i++) { kb[i] = kbs[(i + rk) % 5]; ob[i] = obs[(2 * i + ro) % 5]; }
                        const hb_sums s = hb_layout(n, kb, ob, seed ? seed_words : NULL, forms[f], shared, rows);
                        size_t kt = 0, ot = 0, st = 0, longest = 0, widest = 0;
                        for (int i = 0; i < n; i++, ++*rows_checked) {
                            if (naive_row(n, kb, ob, seed != 0, forms[f], shared, i, &rows[i])) return 1;
                            const size_t sw = seed ? seed_words(kb[i], ob[i]) : 0;
                            kt += words_of(kb[i]); ot += words_of(ob[i]); st += sw;
                            if (sw > longest) longest = sw;
                            if (words_of(ob[i]) > widest) widest = words_of(ob[i]);
                            if (forms[f]) {                      /* a row a stride apart ends before the next one begins */
                                CHECK(rows[i].key_words <= forms[f]->key && rows[i].out_words <= forms[f]->out);
                            } else if (i + 1 < n) {              /* packed rows tile their area */
                                CHECK(rows[i + 1].key_off == rows[i].key_off + rows[i].key_words && rows[i + 1].out_off == rows[i].out_off + rows[i].out_words);
                                if (!shared) CHECK(rows[i + 1].extra_off == rows[i].extra_off + rows[i].extra_words);
                            }
                        }
                        CHECK(s.key_words == kt && s.out_words == ot && s.extra_words == (shared ? longest : st) && s.widest_out == widest);
                        if (n == 0) CHECK(s.key_words == 0 && s.widest_out == 0);
                        free(kb); free(ob); free(rows);
                    }
    return 0;
}

static int refused(const hb_limits *l, uint64_t extra, const char *text)
{
    msg[0] = 0;
    CHECK(hb_limits_check(l, extra, "create", &names) == QLDPC_ESIZE && strstr(msg, text) && strstr(msg, "create: "));
    return 0;
}
static int accepted(const hb_limits *l, uint64_t extra)
{
    msg[0] = 0;
    CHECK(hb_limits_check(l, extra, "create", &names) == QLDPC_OK && msg[0] == 0);
    return 0;
}

static int limits(void)
{
    const hb_limits none = {0, 64, 64}, one = {1, 64, 64}, cap = {HB_MAX_BLOCKS, 64, 64}, past = {HB_MAX_BLOCKS + 1, 64, 64};
    if (refused(&none, 0, "max_blocks=0") || accepted(&one, 0) || accepted(&cap, 0) || refused(&past, 0, "(up to 65535)")) return 1;
    const hb_limits key_cap = {1, HB_MAX_BITS, 0}, key_past = {1, HB_MAX_BITS + 1, 0}, key_none = {1, 0, 0};
    const hb_limits out_cap = {1, 1, HB_MAX_BITS}, out_past = {1, 1, HB_MAX_BITS + 1}, out_neg = {1, 1, -1}, out_none = {1, 1, 0};
    if (accepted(&key_cap, 0) || refused(&key_past, 0, "max_key_bits=16777217") || refused(&key_none, 0, "max_key_bits=0")) return 1;
    if (accepted(&out_cap, 0) || refused(&out_past, 0, "max_final_bits=16777217") || refused(&out_neg, 0, "max_final_bits=-1") || accepted(&out_none, 0)) return 1;
    /* 2^15 blocks of 32760 + 32760 + 16 = 2^16 words are the first to reach 2^31; one output word or one block less stays under it */
    const hb_limits at = {32768, 32 * 32760, 32 * 32760}, word_less = {32768, 32 * 32760, 32 * 32760 - 32}, block_less = {32767, 32 * 32760, 32 * 32760};
    if (refused(&at, 0, "pass 2^31 staged words") || accepted(&word_less, 0) || accepted(&block_less, 0)) return 1;
    /* and with a third row: 32752 + 16 + 32752 + 16 words */
    const hb_limits with_extra = {32768, 32 * 32752, 32 * 32752};
    if (refused(&with_extra, 16, "pass 2^31 staged words") || accepted(&with_extra, 15)) return 1;
    /* the largest context there is stays inside 64 bits */
    const hb_limits all = {HB_MAX_BLOCKS, HB_MAX_BITS, HB_MAX_BITS};
    return refused(&all, (uint64_t)1 << 20, "pass 2^31 staged words");
}

static int call_checks(void)
{
    const hb_limits l = {5, 1000, 500};
    msg[0] = 0;
    int *kb = malloc(sizeof(int) * 5), *ob = malloc(sizeof(int) * 5);
    for (int i = 0; i < 5; i++) { kb[i] = 1000; ob[i] = 500; }
    CHECK(hb_check_blocks(&l, 5, kb, ob, 0, "call", &names) == QLDPC_OK && msg[0] == 0);
    CHECK(hb_check_blocks(&l, -1, kb, ob, 0, "call", &names) == QLDPC_EINVAL && msg[0] == 0);      /* the status alone says it */
    CHECK(hb_check_blocks(&l, 6, kb, ob, 0, "call", &names) == QLDPC_ESIZE && strstr(msg, "6 blocks, the context holds 5"));
    CHECK(hb_check_blocks(&l, 0, NULL, NULL, 1, "call", &names) == QLDPC_OK);
    CHECK(hb_check_blocks(&l, 5, NULL, ob, 0, "call", &names) == QLDPC_EINVAL && strstr(msg, "NULL argument array"));
    CHECK(hb_check_blocks(&l, 5, kb, ob, 1, "call", &names) == QLDPC_EINVAL && strstr(msg, "NULL argument array"));
    kb[3] = 0;
    CHECK(hb_check_blocks(&l, 5, kb, ob, 0, "call", &names) == QLDPC_ESIZE && strstr(msg, "call: block 3: workbits=0 final_bits=500"));
    CHECK(hb_check_blocks(&l, 3, kb, ob, 0, "call", &names) == QLDPC_OK);      /* blocks past n are not read */
    kb[3] = 1001;
    CHECK(hb_check_blocks(&l, 5, kb, ob, 0, "call", &names) == QLDPC_ESIZE && strstr(msg, "block 3: workbits=1001, the context holds 1000"));
    kb[3] = 1000; ob[0] = 501; ob[4] = -1;                       /* the first block that fails is the one named */
    CHECK(hb_check_blocks(&l, 5, kb, ob, 0, "call", &names) == QLDPC_ESIZE && strstr(msg, "block 0: final_bits=501, the context holds 500"));
    ob[0] = 500;
    CHECK(hb_check_blocks(&l, 5, kb, ob, 0, "call", &names) == QLDPC_ESIZE && strstr(msg, "block 4: workbits=1000 final_bits=-1"));
    ob[4] = 0;

    /* row pointers of the host form: a block of 0 bits needs no output row */
    uint32_t *word = malloc(4);
    const uint32_t **in = malloc(sizeof(*in) * 5), **seeds = malloc(sizeof(*seeds) * 5);
    uint32_t **out = malloc(sizeof(*out) * 5);
    for (int i = 0; i < 5; i++) { in[i] = word; seeds[i] = word; out[i] = word; }
    out[4] = NULL;
    msg[0] = 0;
    CHECK(hb_check_rows(5, ob, in, NULL, out, "call") == QLDPC_OK && hb_check_rows(5, ob, in, seeds, out, "call") == QLDPC_OK && msg[0] == 0);
    out[1] = NULL;
    CHECK(hb_check_rows(5, ob, in, seeds, out, "call") == QLDPC_EINVAL && strstr(msg, "call: block 1: NULL output row"));
    seeds[1] = NULL;
    CHECK(hb_check_rows(5, ob, in, seeds, out, "call") == QLDPC_EINVAL && strstr(msg, "block 1: NULL seed row"));
    CHECK(hb_check_rows(5, ob, in, NULL, out, "call") == QLDPC_EINVAL && strstr(msg, "block 1: NULL output row"));
    in[2] = NULL; in[1] = NULL;
    CHECK(hb_check_rows(5, ob, in, seeds, out, "call") == QLDPC_EINVAL && strstr(msg, "block 1: NULL key row"));
    free(word); free(in); free(seeds); free(out);

    /* rows of the device form against their strides: 1000 bits are 32 words, 500 are 16, 1499 are 47 */
    ob[4] = 500;
    const hb_strides fits = {32, 16, 47}, key_short = {31, 16, 47}, out_short = {32, 15, 47}, seed_short = {32, 16, 46}, one_seed = {32, 16, 0};
    msg[0] = 0;
    CHECK(hb_check_strides(5, kb, ob, seed_words, &fits, "call", &names) == QLDPC_OK && msg[0] == 0);
    CHECK(hb_check_strides(5, kb, ob, NULL, &fits, "call", &names) == QLDPC_OK && hb_check_strides(5, kb, ob, seed_words, &one_seed, "call", &names) == QLDPC_OK);
    CHECK(hb_check_strides(5, kb, ob, seed_words, &key_short, "call", &names) == QLDPC_ESIZE && strstr(msg, "block 0: workbits=1000 pass a key row of 31 words"));
    CHECK(hb_check_strides(5, kb, ob, seed_words, &out_short, "call", &names) == QLDPC_ESIZE && strstr(msg, "block 0: final_bits=500 pass an output row of 15 words"));
    CHECK(hb_check_strides(5, kb, ob, seed_words, &seed_short, "call", &names) == QLDPC_ESIZE && strstr(msg, "block 0: 1000 -> 500 bits pass a seed row of 46 words"));
    CHECK(hb_check_strides(5, kb, ob, NULL, &seed_short, "call", &names) == QLDPC_OK);
    kb[0] = 992; ob[0] = 480;                                    /* block 0 now fits the short rows; block 1 is the first that does not */
    CHECK(hb_check_strides(5, kb, ob, NULL, &key_short, "call", &names) == QLDPC_ESIZE && strstr(msg, "block 1: "));
    CHECK(hb_check_strides(1, kb, ob, seed_words, &key_short, "call", &names) == QLDPC_OK && hb_check_strides(1, kb, ob, NULL, &out_short, "call", &names) == QLDPC_OK);
    free(kb); free(ob);
    return 0;
}

int main(void)
{
    CHECK(hb_tail_mask(1) == 0x80000000u && hb_tail_mask(32) == 0xFFFFFFFFu && hb_tail_mask(33) == 0x80000000u && hb_tail_mask(31) == 0xFFFFFFFEu);
    CHECK(hb_words(0) == 0 && hb_words(1) == 1 && hb_words(32) == 1 && hb_words(33) == 2 && hb_words(HB_MAX_BITS) == (1u << 19));
    long rows_checked = 0;
    if (layouts(&rows_checked) || limits() || call_checks()) return 1;
    CHECK(rows_checked == 25 * 7 * (0 + 1 + 2 + 5));             /* 25 rotations, 3 forms x 3 seed cases less the 2 shared-and-strided ones */
    printf("sanitizer pass ok: %ld rows\n", rows_checked);
    return 0;
}
