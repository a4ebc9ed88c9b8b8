/* Sanitizer pass over the arithmetic of the NTT method of the Toeplitz hash (qldpc_toeplitz_ntt_core.h, no HIP): the edge sizes through
 * the core's own functions, tile by tile and pass by pass as the kernels and qldpc_toeplitz_ntt_host walk them, from buffers of exactly
 * the words a block owns, against a bit-serial loop.  Built with -fsanitize=address,undefined by tests/test_toeplitz_ntt.py */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../qcrypto-ldpc_amd/csrc/qldpc_toeplitz_ntt_core.h"

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

typedef struct { uint32_t *w, *wi, *lo, *hi, kl, kmax; } tables;

static uint32_t to_mont(uint32_t a) { return tzn_mul(a, TZN_R1); }

/* each table in an allocation of its own: one entry past any of them is an ASan report */
static void build(tables *t, uint32_t B, uint32_t kmax)
{
    const uint32_t kl = tzn_table_split(kmax), half = 1u << (B - 1);
    t->w = malloc(4 * (size_t)half); t->wi = malloc(4 * (size_t)half);
    t->lo = malloc(4 * ((size_t)1 << kl)); t->hi = malloc(4 * ((size_t)1 << (kmax - kl)));
    t->kl = kl; t->kmax = kmax;
    const uint32_t rb = to_mont(tzn_root(B)), rbi = to_mont(tzn_pow(tzn_root(B), TZN_P - 2u));
    t->w[0] = t->wi[0] = t->lo[0] = t->hi[0] = TZN_R1;
    for (uint32_t x = 1; x < half; x++) { t->w[x] = tzn_mont(t->w[x - 1], rb); t->wi[x] = tzn_mont(t->wi[x - 1], rbi); }
    const uint32_t r = tzn_root(kmax), rl = to_mont(r), rh = to_mont(tzn_pow(r, 1u << kl));
    for (uint32_t x = 1; x < (1u << kl); x++) t->lo[x] = tzn_mont(t->lo[x - 1], rl);
    for (uint32_t x = 1; x < (1u << (kmax - kl)); x++) t->hi[x] = tzn_mont(t->hi[x - 1], rh);
}

static void drop(tables *t) { free(t->w); free(t->wi); free(t->lo); free(t->hi); }

static void forward(uint32_t *x, uint32_t k, uint32_t B, uint32_t pass, const tables *tb, int src, const uint32_t *bits, uint32_t count)
{
    const tzn_pass ps = tzn_pass_of(k, B, pass);
    const uint32_t E = 1u << ps.le;
    uint32_t *s = malloc(4 * (size_t)E), lo;
    for (uint32_t tile = 0; tile < (1u << (k - ps.le)); tile++) {
        for (uint32_t e = 0; e < E; e++) {
            const uint32_t g = tzn_index(ps, tile, e, &lo);
            s[e] = src == 1 ? tzn_key_residue(bits, count, k, g) : src == 2 ? tzn_seed_residue(bits, count, g) : x[g];
        }
        for (uint32_t lh = ps.b; lh-- > 0;)
            for (uint32_t u = 0; u < E / 2u; u++) {
                const uint32_t pos = tzn_pair(ps, u, lh);
                tzn_dif(&s[pos], &s[pos + (1u << (ps.sp + lh))], tb->w[tzn_pair_twiddle(ps, pos, lh, B)]);
            }
        for (uint32_t e = 0; e < E; e++) {
            const uint32_t g = tzn_index(ps, tile, e, &lo);
            x[g] = ps.sh ? tzn_mont(s[e], tzn_twiddle(tb->lo, tb->hi, tb->kl, tb->kmax, tzn_factor(ps, e, lo, tb->kmax), 0)) : s[e];
        }
    }
    free(s);
}

static void inverse(uint32_t *x, const uint32_t *y, uint32_t k, uint32_t B, uint32_t pass, const tables *tb, uint32_t n, uint32_t m, uint32_t *out)
{
    const tzn_pass ps = tzn_pass_of(k, B, pass);
    const uint32_t E = 1u << ps.le, scale = tzn_scale(k);
    uint32_t *s = malloc(4 * (size_t)E), lo;
    for (uint32_t tile = 0; tile < (1u << (k - ps.le)); tile++) {
        for (uint32_t e = 0; e < E; e++) {
            const uint32_t g = tzn_index(ps, tile, e, &lo);
            uint32_t v = y ? tzn_mont(x[g], y[g]) : x[g];
            if (ps.sh) v = tzn_mont(v, tzn_twiddle(tb->lo, tb->hi, tb->kl, tb->kmax, tzn_factor(ps, e, lo, tb->kmax), 1));
            s[e] = v;
        }
        for (uint32_t lh = 0; lh < ps.b; lh++)
            for (uint32_t u = 0; u < E / 2u; u++) {
                const uint32_t pos = tzn_pair(ps, u, lh);
                tzn_dit(&s[pos], &s[pos + (1u << (ps.sp + lh))], tb->wi[tzn_pair_twiddle(ps, pos, lh, B)]);
            }
        for (uint32_t e = 0; e < E; e++) {
            const uint32_t g = tzn_index(ps, tile, e, &lo);
            if (!out) { x[g] = s[e]; continue; }
            const uint32_t i = tzn_out_index(n, k, g);
            if (i < m) out[i >> 5] |= tzn_out_bit(s[e], scale) << (31u - (i & 31u));
        }
    }
    free(s);
}

static void hash(const uint32_t *key, uint32_t n, const uint32_t *seed, uint32_t m, uint32_t B, uint32_t *out)
{
    const uint32_t k = (uint32_t)tzn_log2_len((int)n, (int)m), P = tzn_passes(k, B);
    uint32_t *a = malloc(4 * ((size_t)1 << k)), *b = malloc(4 * ((size_t)1 << k));
    tables tb;
    build(&tb, B, k);
    for (uint32_t pass = 0; pass < P; pass++) {
        forward(a, k, B, pass, &tb, pass ? 0 : 1, key, n);
        forward(b, k, B, pass, &tb, pass ? 0 : 2, seed, n + m - 1u);
    }
    for (uint32_t pass = P; pass-- > 0;) inverse(a, pass == P - 1u ? b : NULL, k, B, pass, &tb, n, m, pass ? NULL : out);
    drop(&tb);
    free(a); free(b);
}

int main(void)
{
    static const int ns[] = {1, 31, 32, 33, 63, 64, 65, 1000, 4097}, ms[] = {1, 31, 32, 33, 63, 64, 65, 257};
    static const uint32_t Bs[] = {1, 2, 5, 9};
    CHECK((uint32_t)(TZN_P * TZN_PINV) == 1u && TZN_R1 == (uint32_t)((1ull << 32) % TZN_P) && TZN_R2 == (uint32_t)(((uint64_t)TZN_R1 * TZN_R1) % TZN_P));
    CHECK(tzn_mul(TZN_P - 1u, TZN_P - 1u) == 1u && tzn_mul(0u, 12345u) == 0u && tzn_mul(1u << 30, 1u << 16) == (uint32_t)((1ull << 46) % TZN_P));
    CHECK(tzn_add(TZN_P - 1u, TZN_P - 1u) == TZN_P - 2u && tzn_sub(0u, 1u) == TZN_P - 1u && tzn_sub(5u, 5u) == 0u);
    for (uint32_t i = 0; i < 2000; i++) {
        const uint32_t x = rng32() % TZN_P, y = rng32() % TZN_P;
        CHECK(tzn_mul(x, y) == (uint32_t)(((uint64_t)x * y) % TZN_P) && tzn_add(x, y) == (uint32_t)(((uint64_t)x + y) % TZN_P));
        CHECK(tzn_sub(x, y) == (uint32_t)(((uint64_t)x + TZN_P - y) % TZN_P));
    }
    for (uint32_t k = 1; k <= TZN_MAX_LOG2; k++) CHECK(tzn_pow(tzn_root(k), 1u << (k - 1)) == TZN_P - 1u);
    CHECK(tzn_log2_len(1, 1) == 5 && tzn_log2_len(16, 17) == 5 && tzn_log2_len(17, 17) == 6 && tzn_log2_len(0, 4) == -1 && tzn_log2_len(4, 0) == -1);
    CHECK(tzn_log2_len(1 << 24, 1 << 24) == 25 && tzn_out_base(1, 5) == 0 && tzn_out_base(2, 5) == 0 && tzn_out_base(33, 6) == 32 && tzn_turn(33) == 0);
    int cases = 0;
    for (size_t ai = 0; ai < sizeof(ns) / sizeof(*ns); ai++)
        for (size_t bi = 0; bi < sizeof(ms) / sizeof(*ms); bi++) {
            const int n = ns[ai], m = ms[bi];
            const uint32_t nw = ((uint32_t)n + 31u) / 32u, ow = ((uint32_t)m + 31u) / 32u, sw = ((uint32_t)(n + m - 1) + 31u) / 32u;
            uint32_t *key = malloc(4 * (size_t)nw), *seed = malloc(4 * (size_t)sw), *ref = calloc(ow, 4), *got = malloc(4 * (size_t)ow);
            for (uint32_t k = 0; k < nw; k++) key[k] = rng32();      /* garbage past n and past n + m - 1 stays in */
            for (uint32_t k = 0; k < sw; k++) seed[k] = rng32();
            for (int i = 0; i < m; i++) {
                int y = 0;
                for (int j = 0; j < n; j++) y ^= bit(key, (uint32_t)j) & bit(seed, (uint32_t)(i + j));
                ref[i >> 5] |= (uint32_t)y << (31 - (i & 31));
            }
            for (size_t c = 0; c < sizeof(Bs) / sizeof(*Bs); c++) {
                memset(got, 0, 4 * (size_t)ow);
                hash(key, (uint32_t)n, seed, (uint32_t)m, Bs[c], got);
                if (memcmp(got, ref, 4 * (size_t)ow)) { fprintf(stderr, "FAILED n=%d m=%d B=%u\n", n, m, Bs[c]); return 1; }
                cases++;
            }
            free(key); free(seed); free(ref); free(got);
        }
    /* the largest counts: an all-ones key of 2^12 bits against all-ones seed bits, every c_i = n */
    {
        const uint32_t n = 4096, m = 70, nw = n / 32, sw = (n + m - 1 + 31) / 32;
        uint32_t *key = malloc(4 * (size_t)nw), *seed = malloc(4 * (size_t)sw), got[3] = {0, 0, 0};
        memset(key, 0xff, 4 * (size_t)nw); memset(seed, 0xff, 4 * (size_t)sw);
        hash(key, n, seed, m, 9, got);
        CHECK(got[0] == 0 && got[1] == 0 && got[2] == 0);
        hash(key, n - 1, seed, m, 5, got);
        CHECK(got[0] == 0xffffffffu && got[1] == 0xffffffffu && got[2] == 0xfc000000u);
        free(key); free(seed);
    }
    printf("sanitizer pass ok: %d cases\n", cases);
    return 0;
}
