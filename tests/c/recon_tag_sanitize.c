/* Sanitizer pass over the host side of the sessions' keyed tag (qldpc_recon_tag_core.h and the mirrors of qldpc_recon_tag_host.c, no HIP):
 * qldpc_recon_tag_host at every lane count against the Horner loop of the definition in unsigned __int128, and qldpc_recon_verify_tag_host over made-up
 * batches (good blocks, a CRC mismatch, a failed decode) against a restatement.  Every buffer is malloc'ed at its exact size, so a chunk that read past
 * a key or a decoded row, or a verdict that wrote past a key's words, would be caught.
 * Built with -fsanitize=address,undefined by tests/test_recon_tag_host.py */
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "qldpc.h"
#include "qldpc_recon_tag_core.h"

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

/* the definition: h = 0; for every coefficient: h = (h + c) k */
static uint64_t tag_ref(const uint32_t *w, int n, uint64_t k)
{
    const uint32_t W = ((uint32_t)n + 31u) / 32u;
    uint64_t h = 0;
    for (uint32_t j = 0; j <= W; j++) {
        uint32_t c = j < W ? w[j] : (uint32_t)n;
        if (j + 1 == W && (n & 31)) c &= 0xFFFFFFFFu << (32 - (n & 31));
        h = (uint64_t)((unsigned __int128)((h + c) % PH_P) * k % PH_P);
    }
    return h;
}

static uint32_t crc_ref(const uint32_t *w, int n)
{
    uint32_t c = 0xFFFFFFFFu;
    for (int v = 0; v < ((n + 31) / 32) * 32; v++) {
        /* bit by bit: the bytes of a word go in most significant first, each byte least significant bit first (reflected CRC), bits past n as 0 */
        const int src = (v >> 3) * 8 + (7 - (v & 7));
        const uint32_t b = src < n ? (w[src >> 5] >> (31 - (src & 31))) & 1u : 0u;
        c = ((c ^ b) & 1u) ? (c >> 1) ^ CRC_POLY : c >> 1;
    }
    return c ^ 0xFFFFFFFFu;
}

static const uint32_t special[][2] = {{0, 0}, {0, 1}, {0x1FFFFFFFu, 0xFFFFFFFFu}, {0x1FFFFFFFu, 0xFFFFFFFEu}, {0xFFFFFFFFu, 0xFFFFFFFFu}};
static const int lengths[] = {1, 31, 32, 33, 64, 255 * 32, 256 * 32, 257 * 32, 8191, 52429, 1 << 18};
static const int lane_counts[] = {1, 2, 64, 256, 1024};

static int tags(long *cases)
{
    for (int li = 0; li < COUNT(lengths); li++) {
        const int n = lengths[li], W = (n + 31) / 32;
        uint32_t *w = malloc(sizeof(uint32_t) * (size_t)W);
        for (int i = 0; i < W; i++) w[i] = (uint32_t)rnd();
        for (int ki = 0; ki < COUNT(special) + 2; ki++) {
            uint32_t hk[2], tag[2] = {7, 7};
            if (ki < COUNT(special)) { hk[0] = special[ki][0]; hk[1] = special[ki][1]; } else { hk[0] = (uint32_t)rnd(); hk[1] = (uint32_t)rnd(); }
            const uint64_t want = tag_ref(w, n, ph_key(hk[0], hk[1]));
            for (int l = 0; l < COUNT(lane_counts); l++, (*cases)++) {
                CHECK(qldpc_recon_tag_host(w, n, hk, lane_counts[l], tag) == QLDPC_OK);
                CHECK(tag[0] == (uint32_t)(want >> 32) && tag[1] == (uint32_t)want);
            }
        }
        free(w);
    }
    uint32_t w[2] = {1, 2}, hk[2] = {3, 4}, tag[2] = {7, 7};
    CHECK(qldpc_recon_tag_host(w, 0, hk, 256, tag) == QLDPC_ESIZE && qldpc_recon_tag_host(w, 64, hk, 3, tag) == QLDPC_EINVAL);
    CHECK(qldpc_recon_tag_host(w, 64, hk, 0, tag) == QLDPC_EINVAL && qldpc_recon_tag_host(NULL, 64, hk, 256, tag) == QLDPC_EINVAL);
    CHECK(qldpc_recon_tag_host(w, 64, hk, 256, NULL) == QLDPC_EINVAL && tag[0] == 7 && tag[1] == 7);
    return 0;
}

/* a batch of n blocks of mixed lengths up to max_bits: key rows of exactly Wk words, decoded rows of exactly Wn */
static int verdicts(int n, int r, int max_bits, int shared, long *cases)
{
    const int Wk = (max_bits + 31) / 32, Wn = Wk + 3;
    uint32_t *out = malloc(sizeof(uint32_t) * (size_t)n * Wn), *keys = malloc(sizeof(uint32_t) * (size_t)n * Wk), *res_keys = malloc(sizeof(uint32_t) * (size_t)n * Wk);
    uint32_t *want = malloc(sizeof(uint32_t) * (size_t)n), *hk = malloc(sizeof(uint32_t) * (size_t)(shared ? 1 : n) * 2 * r), *tg = malloc(sizeof(uint32_t) * (size_t)n * 2 * r);
    int *kb = malloc(sizeof(int) * (size_t)n), *ok = malloc(sizeof(int) * (size_t)n), *it = malloc(sizeof(int) * (size_t)n), *res = malloc(sizeof(int) * 4 * (size_t)n);
    for (int i = 0; i < n * Wn; i++) out[i] = (uint32_t)rnd();
    for (int i = 0; i < n * Wk; i++) { keys[i] = (uint32_t)rnd(); res_keys[i] = 0xA5A5A5A5u; }
    for (int i = 0; i < (shared ? 1 : n) * 2 * r; i++) hk[i] = (uint32_t)rnd();
    for (int b = 0; b < n; b++) {
        kb[b] = b == 0 ? max_bits : 1 + (int)(rnd() % (uint64_t)max_bits);
        ok[b] = b % 3 != 2;                                                            /* every third block: the decode failed */
        it[b] = (int)(rnd() % 60);
        want[b] = crc_ref(out + (size_t)b * Wn, kb[b]) ^ (b % 3 == 1 ? 0x10u : 0u);      /* ... and every third: ok with another CRC */
    }
    CHECK(qldpc_recon_verify_tag_host(n, r, Wk, Wn, out, keys, kb, want, ok, it, hk, shared ? 0 : 2 * (size_t)r, res_keys, res, tg) == QLDPC_OK);
    for (int b = 0; b < n; b++, (*cases)++) {
        const int nw = (kb[b] + 31) / 32, good = b % 3 == 0;
        const uint32_t *row = out + (size_t)b * Wn, *old = keys + (size_t)b * Wk, *key = hk + (shared ? 0 : (size_t)b * 2 * r);
        int flips = 0;
        for (int v = 0; v < kb[b]; v++) flips += (int)(((row[v >> 5] ^ old[v >> 5]) >> (31 - (v & 31))) & 1u);
        CHECK(res[b] == (good ? QLDPC_OK : QLDPC_EDECODE) && res[n + b] == (good ? flips : 0) && res[2 * n + b] == it[b]);
        CHECK((uint32_t)res[3 * n + b] == crc_ref(row, kb[b]));
        for (int i = 0; i < Wk; i++) {
            const uint32_t m = (i == nw - 1 && (kb[b] & 31)) ? 0xFFFFFFFFu << (32 - (kb[b] & 31)) : 0xFFFFFFFFu;
            CHECK(res_keys[(size_t)b * Wk + i] == (i >= nw ? 0xA5A5A5A5u : good ? (row[i] & m) : old[i]));
        }
        for (int q = 0; q < r; q++) {
            const uint64_t t = good ? tag_ref(row, kb[b], ph_key(key[2 * q], key[2 * q + 1])) : 0ull;
            CHECK(tg[((size_t)b * r + q) * 2] == (uint32_t)(t >> 32) && tg[((size_t)b * r + q) * 2 + 1] == (uint32_t)t);
        }
    }
    CHECK(qldpc_recon_verify_tag_host(n, 0, Wk, Wn, out, keys, kb, want, ok, it, hk, 0, res_keys, res, tg) == QLDPC_EINVAL);
    CHECK(qldpc_recon_verify_tag_host(n, 5, Wk, Wn, out, keys, kb, want, ok, it, hk, 0, res_keys, res, tg) == QLDPC_EINVAL);
    CHECK(qldpc_recon_verify_tag_host(n, r, Wk, Wk - 1, out, keys, kb, want, ok, it, hk, 0, res_keys, res, tg) == QLDPC_ESIZE);
    CHECK(qldpc_recon_verify_tag_host(n, r, Wk, Wn, out, keys, kb, want, ok, it, NULL, 0, res_keys, res, tg) == QLDPC_EINVAL);
    kb[n - 1] = 32 * Wk + 1;
    CHECK(qldpc_recon_verify_tag_host(n, r, Wk, Wn, out, keys, kb, want, ok, it, hk, 0, res_keys, res, tg) == QLDPC_ESIZE);
    free(out); free(keys); free(res_keys); free(want); free(hk); free(tg); free(kb); free(ok); free(it); free(res);
    return 0;
}

int main(void)
{
    long cases = 0;
    if (tags(&cases)) return 1;
    const int sizes[] = {1, 33, 1000, 255 * 32 + 5, 256 * 32, 257 * 32 - 1, 65536, 1 << 18};
    for (int i = 0; i < COUNT(sizes); i++)
        for (int r = 1; r <= RT_MAX_KEYS; r++)
            if (verdicts(sizes[i] > 60000 ? 3 : 7, r, sizes[i], (i + r) & 1, &cases)) return 1;
    printf("sanitizer pass ok: %ld cases\n", cases);
    return 0;
}
