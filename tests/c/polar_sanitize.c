/* Sanitizer pass over the polar encoder and SC decoder on the host (qldpc_polar_core.h and the mirrors of qldpc_polar_host.c, no HIP): every size
 * up to 2^12 in both message types, every row malloc'ed at its exact size, each output asked for alone and all together, the decoder against a
 * plain recursion of the definition on unpacked bits, the encoder against the bit loop of the definition, and every refusal.
 * Built with -fsanitize=address,undefined by tests/test_polar_host.py */
#include "qldpc.h"
#include "qldpc_polar_core.h"

#include "polar_sanitize_common.h"

static void put(uint32_t *row, long i, int b) { if (b) row[i >> 5] |= 1u << (31 - (i & 31)); }

/* the definition on unpacked values, in floats (exact for both message types: small integers, or single float additions); c = the re-encoded
   decisions of the node, returned in place */
typedef struct ref { int f32, maxq; const unsigned char *frozen, *fval; unsigned char *u; float *leaf; } ref;
static void ref_node(const ref *r, const float *L, long s, long lo, unsigned char *c)
{
    if (s == 1) {
        r->leaf[lo] = L[0];
        c[0] = r->u[lo] = r->frozen[lo] ? r->fval[lo] : (unsigned char)(L[0] < 0);
        return;
    }
    const long h = s / 2;
    float *l = (float *)calloc((size_t)h, sizeof(float));
    for (long k = 0; k < h; k++) {
        const float a = L[k], b = L[k + h], ma = a < 0 ? -a : a, mb = b < 0 ? -b : b, m = ma < mb ? ma : mb;
        l[k] = ((a < 0) != (b < 0)) ? -m : m;
    }
    ref_node(r, l, h, lo, c);
    for (long k = 0; k < h; k++) {
        float v = c[k] ? L[k + h] - L[k] : L[k + h] + L[k];
        if (!r->f32) v = v > r->maxq ? r->maxq : (v < -(r->maxq + 1) ? -(r->maxq + 1) : v);
        l[k] = v;
    }
    ref_node(r, l, h, lo + h, c + h);
    for (long k = 0; k < h; k++) c[k] ^= c[k + h];
    free(l);
}

static int run(int n, int f32, int maxq, int n_info, int with_fval)
{
    const long N = 1l << n, W = pl_words(n), Wi = (n_info + 31) / 32;
    const int F = 3;
    int *pos = draw_info_pos(N, n_info);
    unsigned char *frozen = (unsigned char *)malloc((size_t)N), *fvb = (unsigned char *)calloc((size_t)N, 1), *ub = (unsigned char *)malloc((size_t)N),
                  *cb = (unsigned char *)malloc((size_t)N);
    memset(frozen, 1, (size_t)N);
    for (int m = 0; m < n_info; m++) frozen[pos[m]] = 0;
    const size_t esz = f32 ? sizeof(float) : 1;
    void *llr = malloc(esz * (size_t)(F * N)), *leaf = malloc(esz * (size_t)(F * N));
    uint32_t *fv = (uint32_t *)calloc((size_t)(F * W), 4), *u = (uint32_t *)malloc(4 * (size_t)(F * W)), *x = (uint32_t *)malloc(4 * (size_t)(F * W)),
             *info = (uint32_t *)malloc(4 * (size_t)(Wi ? F * Wi : 1)), *u1 = (uint32_t *)malloc(4 * (size_t)(F * W)), *x2 = (uint32_t *)malloc(4 * (size_t)(F * W));
    float *Lf = (float *)malloc(sizeof(float) * (size_t)N), *leaf_ref = (float *)malloc(sizeof(float) * (size_t)N);
    fill_llr(llr, F * N, f32, 1000, 64.0f);
    if (with_fval) for (long i = 0; i < F * W; i++) fv[i] = (uint32_t)rnd();
    const int kind = f32 ? QLDPC_POLAR_F32 : QLDPC_POLAR_I8;
    CHECK(qldpc_polar_decode_host(n, n_info, pos, kind, maxq, F, llr, with_fval ? fv : NULL, u, info, x, leaf) == QLDPC_OK);
    /* each output alone */
    CHECK(qldpc_polar_decode_host(n, n_info, pos, kind, maxq, F, llr, with_fval ? fv : NULL, u1, NULL, NULL, NULL) == QLDPC_OK && !memcmp(u, u1, 4 * (size_t)(F * W)));
    CHECK(qldpc_polar_decode_host(n, n_info, pos, kind, maxq, F, llr, with_fval ? fv : NULL, NULL, NULL, x2, NULL) == QLDPC_OK && !memcmp(x, x2, 4 * (size_t)(F * W)));
    CHECK(qldpc_polar_decode_host(n, n_info, pos, kind, maxq, F, llr, with_fval ? fv : NULL, NULL, info, NULL, NULL) == QLDPC_OK);
    CHECK(qldpc_polar_decode_host(n, n_info, pos, kind, maxq, F, llr, with_fval ? fv : NULL, NULL, NULL, NULL, leaf) == QLDPC_OK);
    CHECK(qldpc_polar_decode_host(n, n_info, pos, kind, maxq, F, llr, with_fval ? fv : NULL, NULL, NULL, NULL, NULL) == QLDPC_OK);
    /* x = encode(u), and encode is an involution, in place too */
    CHECK(qldpc_polar_encode_host(n, F, u, x2) == QLDPC_OK && !memcmp(x, x2, 4 * (size_t)(F * W)));
    CHECK(qldpc_polar_encode_host(n, F, x2, x2) == QLDPC_OK && !memcmp(u, x2, 4 * (size_t)(F * W)));
    for (int f = 0; f < F; f++) {
        for (long i = 0; i < N; i++) {
            float v = f32 ? ((float *)llr)[f * N + i] : (float)((int8_t *)llr)[f * N + i];
            if (!f32) v = v > maxq ? maxq : (v < -(maxq + 1) ? -(maxq + 1) : v);
            Lf[i] = v;
            fvb[i] = with_fval ? (unsigned char)get(fv + f * W, i) : 0;
        }
        const ref r = {f32, maxq, frozen, fvb, ub, leaf_ref};
        ref_node(&r, Lf, N, 0, cb);
        for (long i = 0; i < N; i++) {
            CHECK(get(u + f * W, i) == ub[i] && get(x + f * W, i) == cb[i]);
            CHECK((f32 ? ((float *)leaf)[f * N + i] : (float)((int8_t *)leaf)[f * N + i]) == leaf_ref[i]);
        }
        for (int m = 0; m < n_info; m++) CHECK(get(info + f * Wi, m) == ub[pos[m]]);
        /* the encoder by the bit loop of the definition */
        memcpy(cb, ub, (size_t)N);
        for (long m = 1; m < N; m *= 2)
            for (long b = 0; b < N; b += 2 * m)
                for (long k = 0; k < m; k++) cb[b + k] ^= cb[b + m + k];
        memset(x2, 0, 4 * (size_t)W);
        for (long i = 0; i < N; i++) put(x2, i, cb[i]);
        CHECK(!memcmp(x2, x + f * W, 4 * (size_t)W));
    }
    free(pos); free(frozen); free(fvb); free(ub); free(cb); free(llr); free(leaf); free(fv); free(u); free(x); free(info); free(u1); free(x2);
    free(Lf); free(leaf_ref);
    return 0;
}

int main(void)
{
    for (int n = 1; n <= 12; n++) {
        const long N = 1l << n;
        const int ks[4] = {0, (int)N, (int)(N / 2), (int)(rnd() % (uint64_t)(N + 1))};
        for (int k = 0; k < 4; k++)
            for (int with = 0; with < 2; with++) {
                if (run(n, 0, n % 3 == 0 ? 1 : (n % 3 == 1 ? 31 : 126), ks[k], with)) return 1;
                if (run(n, 1, 0, ks[k], with)) return 1;
            }
    }
    /* the word functions */
    for (int s = 0; s <= 5; s++) {
        const uint32_t w = (uint32_t)rnd() & (s == 5 ? 0xffffffffu : 0xffffffffu << (32 - (1 << s)));
        CHECK(pl_enc_word(pl_enc_word(w, s), s) == w);
    }
    /* refusals */
    int8_t z[8] = {0};
    uint32_t row[1] = {0};
    int p2[2] = {1, 1}, p8[1] = {8};
    CHECK(qldpc_polar_decode_host(0, 0, NULL, 0, 31, 1, z, NULL, row, NULL, NULL, NULL) == QLDPC_ESIZE);
    CHECK(qldpc_polar_decode_host(21, 0, NULL, 0, 31, 1, z, NULL, row, NULL, NULL, NULL) == QLDPC_ESIZE);
    CHECK(qldpc_polar_decode_host(3, 0, NULL, 0, 127, 1, z, NULL, row, NULL, NULL, NULL) == QLDPC_ESIZE && strstr(msg, "int8"));
    CHECK(qldpc_polar_decode_host(3, 0, NULL, 0, 0, 1, z, NULL, row, NULL, NULL, NULL) == QLDPC_ESIZE);
    CHECK(qldpc_polar_decode_host(3, 0, NULL, 2, 31, 1, z, NULL, row, NULL, NULL, NULL) == QLDPC_EINVAL);
    CHECK(qldpc_polar_decode_host(3, 2, p2, 0, 31, 1, z, NULL, row, NULL, NULL, NULL) == QLDPC_EINVAL);
    CHECK(qldpc_polar_decode_host(3, 1, p8, 0, 31, 1, z, NULL, row, NULL, NULL, NULL) == QLDPC_ESIZE);
    CHECK(qldpc_polar_decode_host(3, 9, p8, 0, 31, 1, z, NULL, row, NULL, NULL, NULL) == QLDPC_ESIZE);
    CHECK(qldpc_polar_decode_host(3, 1, NULL, 0, 31, 1, z, NULL, row, NULL, NULL, NULL) == QLDPC_ESIZE);
    CHECK(qldpc_polar_decode_host(3, 0, NULL, 0, 31, -1, z, NULL, row, NULL, NULL, NULL) == QLDPC_EINVAL);
    CHECK(qldpc_polar_decode_host(3, 0, NULL, 0, 31, 1, NULL, NULL, row, NULL, NULL, NULL) == QLDPC_EINVAL);
    CHECK(qldpc_polar_decode_host(3, 0, NULL, 0, 31, 0, NULL, NULL, NULL, NULL, NULL, NULL) == QLDPC_OK);
    CHECK(qldpc_polar_encode_host(0, 1, row, row) == QLDPC_ESIZE && qldpc_polar_encode_host(3, -1, row, row) == QLDPC_EINVAL);
    CHECK(qldpc_polar_encode_host(3, 1, NULL, row) == QLDPC_EINVAL && qldpc_polar_encode_host(3, 0, NULL, NULL) == QLDPC_OK);
    printf("polar: sanitizer pass ok\n");
    return 0;
}
