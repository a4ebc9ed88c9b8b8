/* Sanitizer pass over the host side of the guessing rounds of a session (qldpc_recon_guess_settle_host in qldpc_recon_guess_host.c over
 * qldpc_recon_guess_core.h; no HIP): made-up sources in buffers of exactly the sizes the call names -- trial rows of Wn words, key rows of Wk words, with
 * Wk = the key's words and Wn = Wk as the tightest shape, and wider rows as well -- against a restatement bit by bit with a bitwise CRC-32.
 * Built with -fsanitize=address,undefined by tests/test_recon_guess_host.py */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "qldpc.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

static uint64_t state = 0x13198A2E03707344ull;
static uint32_t next(uint32_t below)
{
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(state >> 33) % below;
}
static uint32_t word(void) { return (next(65536) << 16) | next(65536); }

static int bit(const uint32_t *row, int v) { return (int)((row[v >> 5] >> (31 - (v & 31))) & 1u); }

/* CRC-32 (IEEE 802.3, reflected) of the first kb bits of a row, padded with zero bits to whole words, the bytes of a word most significant first */
static uint32_t crc_bits(const uint32_t *row, int kb)
{
    uint32_t c = 0xFFFFFFFFu;
    const int total = (kb + 31) / 32 * 32;
    for (int byte = 0; byte < total / 8; byte++)
        for (int k = 0; k < 8; k++) {      /* a reflected CRC takes the bits of a byte least significant first */
            const int v = byte * 8 + (7 - k), b = v < kb ? bit(row, v) : 0;
            c = ((c ^ (uint32_t)b) & 1u) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
        }
    return c ^ 0xFFFFFFFFu;
}

static int sources(int g, int n_src, int kb, int extra_k, int extra_n, unsigned pass_percent)
{
    const int T = 1 << g, nw = (kb + 31) / 32, Wk = nw + extra_k, Wn = Wk + extra_n;
    const size_t slots = (size_t)n_src * (size_t)T;
    uint32_t *rows = malloc(slots * (size_t)Wn * 4), *keys = malloc((size_t)n_src * (size_t)Wk * 4), *want = malloc((size_t)n_src * 4);
    uint32_t *crc_out = malloc(slots * 4), *res_keys = malloc((size_t)n_src * (size_t)Wk * 4), *alice = malloc((size_t)Wn * 4);
    int *ok = malloc(slots * sizeof(int)), *iters = malloc(slots * sizeof(int)), *kbs = malloc((size_t)n_src * sizeof(int)), *first = malloc((size_t)n_src * sizeof(int));
    int *pass = malloc(slots * sizeof(int)), *res = malloc(4 * (size_t)n_src * sizeof(int)), *guess = malloc(6 * (size_t)n_src * sizeof(int));
    for (int s = 0; s < n_src; s++) {
        kbs[s] = s & 1 ? (kb > 1 ? kb - 1 : 1) : kb;
        first[s] = 1 + (int)next(60);
        for (int w = 0; w < Wn; w++) alice[w] = word();
        want[s] = crc_bits(alice, kbs[s]);
        for (int w = 0; w < Wk; w++) { keys[(size_t)s * Wk + w] = alice[w] ^ (word() & word()); res_keys[(size_t)s * Wk + w] = 0xA5A5A5A5u; }
        for (int t = 0; t < T; t++) {
            uint32_t *r = rows + ((size_t)s * T + t) * Wn;
            const int passes = next(100) < pass_percent;
            for (int w = 0; w < Wn; w++) r[w] = passes && w < nw ? alice[w] : word();
            if (passes && (kbs[s] & 31)) r[(kbs[s] - 1) / 32] ^= word() & ~(0xFFFFFFFFu << (32 - (kbs[s] & 31)));      /* noise in the padding alone */
            ok[(size_t)s * T + t] = passes ? next(8) != 0 : next(3) == 0;
            iters[(size_t)s * T + t] = 1 + (int)next(60);
        }
    }
    CHECK(qldpc_recon_guess_settle_host(g, n_src, Wk, Wn, rows, ok, iters, keys, kbs, want, first, pass, crc_out, res_keys, res, guess) == QLDPC_OK);
    for (int s = 0; s < n_src; s++) {
        const int k = kbs[s], words = (k + 31) / 32;
        int win = -1, n_ok = 0, n_pass = 0, amb = 0, sum = 0, flips = 0;
        for (int t = 0; t < T; t++) {
            const size_t at = (size_t)s * T + t;
            const uint32_t c = crc_bits(rows + at * Wn, k);
            const int p = ok[at] && c == want[s];
            CHECK(crc_out[at] == c && pass[at] == p);
            if (p && win < 0) win = t;
            n_ok += ok[at] != 0; n_pass += p; sum += iters[at];
        }
        const uint32_t *wr = rows + ((size_t)s * T + (win >= 0 ? win : 0)) * Wn;
        for (int t = 0; t < T && win >= 0; t++)
            for (int v = 0; v < k && pass[(size_t)s * T + t]; v++) amb |= bit(rows + ((size_t)s * T + t) * Wn, v) != bit(wr, v);
        const int *gr = guess + 6 * s;
        CHECK(gr[0] == 1 && gr[1] == win && gr[2] == n_ok && gr[3] == n_pass && gr[4] == amb && gr[5] == sum);
        CHECK(res[s] == (win >= 0 ? QLDPC_OK : QLDPC_EDECODE));
        CHECK(res[2 * n_src + s] == first[s] + (win >= 0 ? iters[(size_t)s * T + win] : 0));
        CHECK((uint32_t)res[3 * n_src + s] == crc_out[(size_t)s * T + (win >= 0 ? win : 0)]);
        const uint32_t *out = res_keys + (size_t)s * Wk, *old = keys + (size_t)s * Wk;
        for (int v = 0; v < 32 * words; v++) {
            if (win < 0) { CHECK(bit(out, v) == bit(old, v)); continue; }
            CHECK(bit(out, v) == (v < k ? bit(wr, v) : 0));
            flips += v < k && bit(wr, v) != bit(old, v);
        }
        CHECK(res[n_src + s] == flips);
        for (int w = words; w < Wk; w++) CHECK(out[w] == 0xA5A5A5A5u);      /* nothing is written past the key's words */
    }
    free(rows); free(keys); free(want); free(crc_out); free(res_keys); free(alice); free(ok); free(iters); free(kbs); free(first); free(pass); free(res); free(guess);
    return 0;
}

int main(void)
{
    int cases = 0;
    const int bits[] = {1, 31, 32, 33, 1000}, gs[] = {0, 1, 3, 7, 10};
    for (unsigned i = 0; i < sizeof bits / sizeof *bits; i++)
        for (unsigned j = 0; j < sizeof gs / sizeof *gs; j++, cases += 4) {
            const int T = 1 << gs[j];
            if (sources(gs[j], 1, bits[i], 0, 0, 0) || sources(gs[j], 3, bits[i], 0, 0, 30) || sources(gs[j], 2, bits[i], 1, 3, 100)) return 1;
            if (sources(gs[j], 3, bits[i], 2, 0, T > 16 ? 2 : 50)) return 1;
        }
    /* argument checks: nothing is written */
    uint32_t u[8] = {0}, out[2] = {77, 77};
    int i4[8] = {0}, kb = 40, o[8] = {-7, -7, -7, -7, -7, -7, -7, -7};
    CHECK(qldpc_recon_guess_settle_host(-1, 1, 2, 4, u, i4, i4, u, &kb, u, i4, o, out, out, o, o) == QLDPC_ESIZE);
    CHECK(qldpc_recon_guess_settle_host(QLDPC_GUESS_MAX_BITS + 1, 1, 2, 4, u, i4, i4, u, &kb, u, i4, o, out, out, o, o) == QLDPC_ESIZE);
    CHECK(qldpc_recon_guess_settle_host(0, -1, 2, 4, u, i4, i4, u, &kb, u, i4, o, out, out, o, o) == QLDPC_ESIZE);
    CHECK(qldpc_recon_guess_settle_host(0, 1, 0, 4, u, i4, i4, u, &kb, u, i4, o, out, out, o, o) == QLDPC_ESIZE);
    CHECK(qldpc_recon_guess_settle_host(0, 1, 5, 4, u, i4, i4, u, &kb, u, i4, o, out, out, o, o) == QLDPC_ESIZE);
    kb = 65;
    CHECK(qldpc_recon_guess_settle_host(0, 1, 2, 4, u, i4, i4, u, &kb, u, i4, o, out, out, o, o) == QLDPC_ESIZE && strstr(qldpc_last_error(), "key_bits=65") != NULL);
    kb = 0;
    CHECK(qldpc_recon_guess_settle_host(0, 1, 2, 4, u, i4, i4, u, &kb, u, i4, o, out, out, o, o) == QLDPC_ESIZE);
    kb = 40;
    CHECK(qldpc_recon_guess_settle_host(0, 1, 2, 4, NULL, i4, i4, u, &kb, u, i4, o, out, out, o, o) == QLDPC_EINVAL);
    CHECK(qldpc_recon_guess_settle_host(0, 1, 2, 4, u, i4, i4, u, &kb, u, i4, o, out, out, o, NULL) == QLDPC_EINVAL);
    CHECK(out[0] == 77 && out[1] == 77 && o[0] == -7 && o[7] == -7);
    CHECK(qldpc_recon_guess_settle_host(3, 0, 2, 4, u, i4, i4, u, &kb, u, i4, o, out, out, o, o) == QLDPC_OK && o[0] == -7);      /* no source writes nothing */
    printf("sanitizer pass ok: %d cases\n", cases + 11);
    return 0;
}
