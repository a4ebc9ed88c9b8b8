/* Sanitizer pass over the arithmetic the two sides of a reconciliation session share (qldpc_recon_core.h, no HIP): the chunked CRC fold the kernels
 * run against the serial CRC and a known answer, the two directions of the puncture map (rk_assemble's position -> rank, rk_disclose's rank ->
 * position) against each other, and the staging views against the column order of the header's comment.  Every buffer is malloc'ed at its exact size.
 * Built with -fsanitize=address,undefined by tests/test_recon_host.py */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "qldpc_recon_core.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

static uint64_t state = 0x243F6A8885A308D3ull;
static uint32_t next32(void)
{
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(state >> 32);
}

static int crc_forms(const uint32_t *table)
{
    static const int n_bits[] = {1, 31, 32, 33, 257, 8191, 8192, 8193}, lanes[] = {1, 2, 4, 64, 256};
    for (size_t a = 0; a < sizeof(n_bits) / sizeof(n_bits[0]); a++) {
        const int nw = (n_bits[a] + 31) / 32;
        uint32_t *w = malloc(sizeof(uint32_t) * (size_t)nw);
        for (int i = 0; i < nw; i++) w[i] = next32();
        const uint32_t serial = crc_serial(w, n_bits[a], table);
        for (size_t b = 0; b < sizeof(lanes) / sizeof(lanes[0]); b++) {
            uint32_t *reg = malloc(sizeof(uint32_t) * (size_t)lanes[b]);
            CHECK(crc_chunked(w, n_bits[a], lanes[b], table, reg) == serial);
            free(reg);
        }
        if (n_bits[a] & 31) {      /* bits past n_bits do not matter */
            w[nw - 1] ^= 0xFFFFFFFFu >> (n_bits[a] & 31);
            CHECK(crc_serial(w, n_bits[a], table) == serial);
        }
        free(w);
    }
    /* "123456789": the standard check value over its 9 bytes is 0xCBF43926; whole words are hashed, so 72 bits are the text and three zero bytes */
    const unsigned char text[12] = "123456789";
    uint32_t *w = malloc(sizeof(uint32_t) * 3), *reg = malloc(sizeof(uint32_t) * 4);
    for (int i = 0; i < 3; i++) w[i] = (uint32_t)text[4 * i] << 24 | (uint32_t)text[4 * i + 1] << 16 | (uint32_t)text[4 * i + 2] << 8 | text[4 * i + 3];
    uint32_t c = 0xFFFFFFFFu;      /* byte by byte over the nine bytes alone */
    for (int i = 0; i < 9; i++) c = table[(c ^ text[i]) & 0xFF] ^ (c >> 8);
    CHECK((c ^ 0xFFFFFFFFu) == 0xCBF43926u);
    for (int i = 9; i < 12; i++) c = table[(c ^ text[i]) & 0xFF] ^ (c >> 8);
    CHECK(crc_serial(w, 72, table) == (c ^ 0xFFFFFFFFu) && crc_chunked(w, 72, 4, table, reg) == (c ^ 0xFFFFFFFFu));
    CHECK(crc_serial(w, 64, table) == 0x9AE0DAAFu);      /* CRC-32 of "12345678" */
    free(w); free(reg);
    return 0;
}

static int puncture_map(int M, long *triples)
{
    unsigned char *disclosed = malloc((size_t)M);
    for (int p = 0; p <= (int)(0.65 * M); p++) {
        int d = 0;
        for (int j = 0; j < M; j++) {
            disclosed[j] = !punct_at(j, p, M);
            if (!disclosed[j]) continue;
            CHECK(punct_rank(j, p, M) == j - punct_before(j, p, M) && punct_rank(j, p, M) == d);      /* ranks count the disclosed positions in order */
            CHECK(punct_position(d, p, M) == j);
            d++;
        }
        CHECK(d == M - p && punct_before(M, p, M) == p);
        for (int r = 0; r < d; r++, (*triples)++) {
            const int j = punct_position(r, p, M);
            CHECK(j >= 0 && j < M && disclosed[j] && punct_rank(j, p, M) == r);
        }
    }
    free(disclosed);
    return 0;
}

/* columns must follow each other in the order given, from word 0 to `words`, inside a block of exactly `words` words */
static int tiles(const uint32_t *base, size_t words, const void *const *col, const size_t *len, int n_cols)
{
    size_t at = 0;
    for (int k = 0; k < n_cols; k++) {
        CHECK((const uint32_t *)col[k] == base + at);
        at += len[k];
    }
    CHECK(at == words);
    return 0;
}

static int staging_views(int n, int Wk, int Wm)
{
    const size_t N = (size_t)n, in_words = N * (size_t)(Wk + Wm + 4), bob_words = N * (size_t)(Wk + 4), alice_words = N * (size_t)(Wm + 1);
    CHECK(recon_in_layout(NULL, n, Wk, Wm).words == in_words && recon_in_layout(NULL, n, Wk, Wm).crc == NULL);
    CHECK(recon_bob_layout(NULL, n, Wk).words == bob_words && recon_alice_layout(NULL, n, Wm).words == alice_words);
    {
        uint32_t *b = malloc(sizeof(uint32_t) * in_words);
        const recon_in_view v = recon_in_layout(b, n, Wk, Wm);
        const void *col[] = {v.keys, v.disc, v.mag, v.key_bits, v.n_punct, v.crc};
        const size_t len[] = {N * (size_t)Wk, N * (size_t)Wm, N, N, N, N};
        CHECK(v.words == in_words);
        if (tiles(b, in_words, col, len, 6)) return 1;
        memset(v.keys, 1, sizeof(uint32_t) * len[0]); memset(v.disc, 2, sizeof(uint32_t) * len[1]);      /* every column written in full: the block's size is exact */
        for (int t = 0; t < n; t++) { v.mag[t] = 1.0f; v.key_bits[t] = t; v.n_punct[t] = t; v.crc[t] = (uint32_t)t; }
        free(b);
    }
    {
        uint32_t *b = malloc(sizeof(uint32_t) * bob_words);
        const recon_bob_view v = recon_bob_layout(b, n, Wk);
        const void *col[] = {v.keys, v.status, v.flips, v.iters, v.crc};
        const size_t len[] = {N * (size_t)Wk, N, N, N, N};
        CHECK(v.words == bob_words);
        if (tiles(b, bob_words, col, len, 5)) return 1;
        memset(v.keys, 1, sizeof(uint32_t) * len[0]);
        for (int t = 0; t < n; t++) { v.status[t] = t; v.status[n + t] = t; v.status[2 * n + t] = t; v.status[3 * n + t] = t; }      /* as rk_verify writes its `res` */
        CHECK(v.flips[n - 1] == n - 1 && v.iters[n - 1] == n - 1 && v.crc[n - 1] == n - 1);
        free(b);
    }
    {
        uint32_t *b = malloc(sizeof(uint32_t) * alice_words);
        const recon_alice_view v = recon_alice_layout(b, n, Wm);
        const void *col[] = {v.disc, v.crc};
        const size_t len[] = {N * (size_t)Wm, N};
        CHECK(v.words == alice_words);
        if (tiles(b, alice_words, col, len, 2)) return 1;
        memset(v.disc, 1, sizeof(uint32_t) * len[0]);
        for (int t = 0; t < n; t++) v.crc[t] = (uint32_t)t;
        free(b);
    }
    return 0;
}

int main(void)
{
    uint32_t *table = malloc(sizeof(uint32_t) * 256);
    for (uint32_t i = 0; i < 256; i++) table[i] = crc_table_entry(i);
    CHECK(table[1] == 0x77073096u && table[255] == 0x2D02EF8Du);      /* the published table of the reflected polynomial */
    if (crc_forms(table)) return 1;
    free(table);
    long triples = 0;
    static const int more[] = {511, 512, 513, 1000};
    for (int M = 2; M < 200; M++) if (puncture_map(M, &triples)) return 1;
    for (int k = 0; k < 4; k++) if (puncture_map(more[k], &triples)) return 1;
    CHECK(triples == 1956648);      /* every (M, p, r) of the ranges above */
    if (staging_views(1, 1, 1) || staging_views(3, 8, 5) || staging_views(8, 512, 129)) return 1;
    printf("sanitizer pass ok: %ld (M, p, r) triples\n", triples);
    return 0;
}
