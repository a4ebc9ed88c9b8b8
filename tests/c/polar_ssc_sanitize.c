/* Sanitizer pass over the simplified SC decoder on the host (qldpc_polar_ssc_core.h, the mirror and the plan of qldpc_polar_ssc_host.c, no HIP):
 * every size up to 2^12 in both message types, every row malloc'ed at its exact size, each output asked for alone and all together, the decoder
 * against a plain recursion of the SSC rule on unpacked bits, the plan against its own invariants, and every refusal.
 * Built with -fsanitize=address,undefined by tests/test_polar_ssc_host.py */
#include "qldpc.h"
#include "qldpc_polar_ssc_core.h"

#include "polar_sanitize_common.h"

/* the rule on unpacked values, in floats (exact for both message types: small integers, or single float additions); c = the bits the node
   returns, in place */
typedef struct ref { int f32, maxq; const unsigned char *frozen, *fval; unsigned char *u; } ref;
static void enc(unsigned char *c, long s)
{
    for (long m = 1; m < s; m *= 2)
        for (long b = 0; b < s; b += 2 * m)
            for (long k = 0; k < m; k++) c[b + k] ^= c[b + m + k];
}
static void ref_node(const ref *r, const float *L, long s, long lo, unsigned char *c)
{
    long nf = 0;
    for (long k = 0; k < s; k++) nf += r->frozen[lo + k];
    if (nf == s || nf == 0) {
        for (long k = 0; k < s; k++) c[k] = nf ? r->fval[lo + k] : (unsigned char)(L[k] < 0);
        if (nf) { memcpy(r->u + lo, c, (size_t)s); enc(c, s); }
        else { memcpy(r->u + lo, c, (size_t)s); enc(r->u + lo, s); }
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

/* info positions in clusters: aligned runs of 2^t positions all information, so that rate-1 and rate-0 nodes of many sizes appear */
static int *draw_clustered(long N, int *n_info)
{
    unsigned char *in = (unsigned char *)calloc((size_t)N, 1);
    for (long lo = 0; lo < N;) {
        long s = 1l << (rnd() % 8);
        while (s > 1 && ((lo & (s - 1)) || lo + s > N)) s /= 2;
        const int kind = (int)(rnd() % 3);
        for (long k = 0; k < s; k++) in[lo + k] = kind == 0 ? 0 : (kind == 1 ? 1 : (unsigned char)(rnd() & 1));
        lo += s;
    }
    int K = 0;
    for (long i = 0; i < N; i++) K += in[i];
    int *pos = (int *)malloc(sizeof(int) * (size_t)(K ? K : 1));
    K = 0;
    for (long i = N - 1; i >= 0; i--) if (in[i]) pos[K++] = (int)i;      /* descending: the caller's order is not the natural one */
    free(in);
    *n_info = K;
    return pos;
}

static int run(int n, int f32, int maxq, int n_info, int *pos, int with_fval)
{
    const long N = 1l << n, W = pl_words(n), Wi = (n_info + 31) / 32;
    const int F = 3;
    unsigned char *frozen = (unsigned char *)malloc((size_t)N), *fvb = (unsigned char *)calloc((size_t)N, 1), *ub = (unsigned char *)malloc((size_t)N),
                  *cb = (unsigned char *)malloc((size_t)N);
    memset(frozen, 1, (size_t)N);
    for (int m = 0; m < n_info; m++) frozen[pos[m]] = 0;
    const size_t esz = f32 ? sizeof(float) : 1;
    void *llr = malloc(esz * (size_t)(F * N));
    uint32_t *fv = (uint32_t *)calloc((size_t)(F * W), 4), *u = (uint32_t *)malloc(4 * (size_t)(F * W)), *x = (uint32_t *)malloc(4 * (size_t)(F * W)),
             *info = (uint32_t *)malloc(4 * (size_t)(Wi ? F * Wi : 1)), *u1 = (uint32_t *)malloc(4 * (size_t)(F * W)), *x2 = (uint32_t *)malloc(4 * (size_t)(F * W));
    float *Lf = (float *)malloc(sizeof(float) * (size_t)N);
    fill_llr(llr, F * N, f32, 1000, 64.0f);
    if (with_fval) for (long i = 0; i < F * W; i++) fv[i] = (uint32_t)rnd();
    const int kind = f32 ? QLDPC_POLAR_F32 : QLDPC_POLAR_I8;
    const uint32_t *fz = with_fval ? fv : NULL;
    CHECK(qldpc_polar_decode_ssc_host(n, n_info, pos, kind, maxq, F, llr, fz, u, info, x) == QLDPC_OK);
    /* each output alone */
    CHECK(qldpc_polar_decode_ssc_host(n, n_info, pos, kind, maxq, F, llr, fz, u1, NULL, NULL) == QLDPC_OK && !memcmp(u, u1, 4 * (size_t)(F * W)));
    CHECK(qldpc_polar_decode_ssc_host(n, n_info, pos, kind, maxq, F, llr, fz, NULL, NULL, x2) == QLDPC_OK && !memcmp(x, x2, 4 * (size_t)(F * W)));
    CHECK(qldpc_polar_decode_ssc_host(n, n_info, pos, kind, maxq, F, llr, fz, NULL, info, NULL) == QLDPC_OK);
    CHECK(qldpc_polar_decode_ssc_host(n, n_info, pos, kind, maxq, F, llr, fz, NULL, NULL, NULL) == QLDPC_OK);
    /* x = encode(u) */
    CHECK(qldpc_polar_encode_host(n, F, u, x2) == QLDPC_OK && !memcmp(x, x2, 4 * (size_t)(F * W)));
    for (int f = 0; f < F; f++) {
        for (long i = 0; i < N; i++) {
            float v = f32 ? ((float *)llr)[f * N + i] : (float)((int8_t *)llr)[f * N + i];
            if (!f32) v = v > maxq ? maxq : (v < -(maxq + 1) ? -(maxq + 1) : v);
            Lf[i] = v;
            fvb[i] = with_fval ? (unsigned char)get(fv + f * W, i) : 0;
        }
        const ref r = {f32, maxq, frozen, fvb, ub};
        ref_node(&r, Lf, N, 0, cb);
        for (long i = 0; i < N; i++) CHECK(get(u + f * W, i) == ub[i] && get(x + f * W, i) == cb[i]);
        for (int m = 0; m < n_info; m++) CHECK(get(info + f * Wi, m) == ub[pos[m]]);
    }
    /* the plan, in a row of exactly its largest size: the steps tile the frame in leaf order, aligned, with the kinds of the mask */
    const long cap = pl_ssc_max_steps(n);
    int *steps = (int *)malloc(sizeof(int) * PL_SSC_STEP * (size_t)cap), n_steps = -1;
    CHECK(qldpc_polar_ssc_plan_host(n, n_info, pos, steps, &n_steps) == QLDPC_OK && n_steps >= 1 && n_steps <= cap);
    long next = 0;
    for (int i = 0; i < n_steps; i++) {
        const long j = steps[3 * i], lam = steps[3 * i + 1], leaves = 1l << lam, first = n < 5 ? 0 : j * 32;
        CHECK(j == next && lam >= (n < 5 ? n : 5) && lam <= n && first % leaves == 0 && first + leaves <= N);
        long nf = 0;
        for (long k = 0; k < leaves; k++) nf += frozen[first + k];
        if (n < 5) CHECK(steps[3 * i + 2] == PL_SSC_MIXED);
        else CHECK(steps[3 * i + 2] == (nf == leaves ? PL_SSC_RATE0 : (nf == 0 ? PL_SSC_RATE1 : PL_SSC_MIXED)) && (steps[3 * i + 2] != PL_SSC_MIXED || lam == 5));
        next = j + (n < 5 ? 1 : leaves / 32);
    }
    CHECK(next == (n < 5 ? 1 : N / 32));
    free(steps); free(frozen); free(fvb); free(ub); free(cb); free(llr); free(fv); free(u); free(x); free(info); free(u1); free(x2); free(Lf);
    return 0;
}

int main(void)
{
    for (int n = 1; n <= 12; n++) {
        const long N = 1l << n;
        const int ks[4] = {0, (int)N, (int)(N / 2), (int)(rnd() % (uint64_t)(N + 1))};
        for (int k = 0; k < 6; k++)
            for (int with = 0; with < 2; with++) {
                int n_info = k < 4 ? ks[k] : 0;
                int *pos = k < 4 ? draw_info_pos(N, n_info) : draw_clustered(N, &n_info);
                if (run(n, 0, n % 3 == 0 ? 1 : (n % 3 == 1 ? 31 : 126), n_info, pos, with)) return 1;
                if (run(n, 1, 0, n_info, pos, with)) return 1;
                free(pos);
            }
    }
    /* refusals */
    int8_t z[8] = {0};
    uint32_t row[1] = {0};
    int p2[2] = {1, 1}, p8[1] = {8}, steps[3], ns;
    CHECK(qldpc_polar_decode_ssc_host(0, 0, NULL, 0, 31, 1, z, NULL, row, NULL, NULL) == QLDPC_ESIZE);
    CHECK(qldpc_polar_decode_ssc_host(21, 0, NULL, 0, 31, 1, z, NULL, row, NULL, NULL) == QLDPC_ESIZE);
    CHECK(qldpc_polar_decode_ssc_host(3, 0, NULL, 0, 127, 1, z, NULL, row, NULL, NULL) == QLDPC_ESIZE && strstr(msg, "int8"));
    CHECK(qldpc_polar_decode_ssc_host(3, 0, NULL, 0, 0, 1, z, NULL, row, NULL, NULL) == QLDPC_ESIZE);
    CHECK(qldpc_polar_decode_ssc_host(3, 0, NULL, 2, 31, 1, z, NULL, row, NULL, NULL) == QLDPC_EINVAL);
    CHECK(qldpc_polar_decode_ssc_host(3, 2, p2, 0, 31, 1, z, NULL, row, NULL, NULL) == QLDPC_EINVAL);
    CHECK(qldpc_polar_decode_ssc_host(3, 1, p8, 0, 31, 1, z, NULL, row, NULL, NULL) == QLDPC_ESIZE);
    CHECK(qldpc_polar_decode_ssc_host(3, 9, p8, 0, 31, 1, z, NULL, row, NULL, NULL) == QLDPC_ESIZE);
    CHECK(qldpc_polar_decode_ssc_host(3, 1, NULL, 0, 31, 1, z, NULL, row, NULL, NULL) == QLDPC_ESIZE);
    CHECK(qldpc_polar_decode_ssc_host(3, 0, NULL, 0, 31, -1, z, NULL, row, NULL, NULL) == QLDPC_EINVAL);
    CHECK(qldpc_polar_decode_ssc_host(3, 0, NULL, 0, 31, 1, NULL, NULL, row, NULL, NULL) == QLDPC_EINVAL);
    CHECK(qldpc_polar_decode_ssc_host(3, 0, NULL, 0, 31, 0, NULL, NULL, NULL, NULL, NULL) == QLDPC_OK);
    CHECK(qldpc_polar_ssc_plan_host(0, 0, NULL, steps, &ns) == QLDPC_ESIZE && qldpc_polar_ssc_plan_host(21, 0, NULL, steps, &ns) == QLDPC_ESIZE);
    CHECK(qldpc_polar_ssc_plan_host(3, 2, p2, steps, &ns) == QLDPC_EINVAL && qldpc_polar_ssc_plan_host(3, 1, p8, steps, &ns) == QLDPC_ESIZE);
    CHECK(qldpc_polar_ssc_plan_host(3, 0, NULL, NULL, &ns) == QLDPC_EINVAL && qldpc_polar_ssc_plan_host(3, 0, NULL, steps, NULL) == QLDPC_EINVAL);
    CHECK(qldpc_polar_ssc_plan_host(3, 0, NULL, steps, &ns) == QLDPC_OK && ns == 1 && steps[1] == 3 && steps[2] == PL_SSC_MIXED);
    printf("polar ssc: sanitizer pass ok\n");
    return 0;
}
