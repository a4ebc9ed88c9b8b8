/* Sanitizer pass over the host side of the syndrome-weight QBER estimate (qldpc_qber_host.c over qldpc_qber_core.h, no HIP; linked with qldpc_graph.c):
 * tables, counts and argmax on buffers allocated at their exact sizes, the counts against a per-VN restatement of the rule.  Built with
 * -fsanitize=address,undefined by tests/test_qber_host.py */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "qldpc.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

static uint64_t rng_state = 0x13198a2e03707344ull;
static uint32_t rng32(void)
{
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return (uint32_t)((z ^ (z >> 31)) >> 16);
}

static int bit_of(const uint32_t *row, int v) { return row ? (int)((row[v >> 5] >> (31 - (v & 31))) & 1u) : 0; }

/* one code, one random frame with the inputs of `mask` present (1 class map + n_channel, 2 syndrome, 4 erase, 8 known + value) */
static int one_case(const qldpc_code *code, int mask)
{
    const int N = qldpc_code_n(code), M = qldpc_code_m(code), E = qldpc_code_e(code), D = qldpc_code_max_cn_degree(code);
    const size_t Wn = (size_t)(N + 31) / 32, Wm = (size_t)(M + 31) / 32;
    uint32_t *bits = malloc(4 * Wn), *erase = malloc(4 * Wn), *known = malloc(4 * Wn), *value = malloc(4 * Wn), *synd = malloc(4 * Wm);
    uint8_t *cls = malloc((size_t)N);
    int *var = malloc(sizeof(int) * (size_t)E), *chk = malloc(sizeof(int) * (size_t)E);
    uint32_t *got = malloc(sizeof(uint32_t) * 2 * (size_t)(D + 1)), *want = calloc(2 * (size_t)(D + 1), sizeof(uint32_t));
    int *d = calloc((size_t)M, sizeof(int)), *u = calloc((size_t)M, sizeof(int)), *dead = calloc((size_t)M, sizeof(int));
    for (size_t w = 0; w < Wn; w++) {      /* tail bits past N set at random on purpose */
        bits[w] = rng32() | (rng32() << 16);
        erase[w] = rng32() & rng32() & rng32() & (rng32() | (rng32() << 16));
        known[w] = rng32() & rng32() & (rng32() << 16 | rng32());
        value[w] = rng32() | (rng32() << 16);
    }
    for (size_t w = 0; w < Wm; w++) synd[w] = rng32() | (rng32() << 16);
    for (int v = 0; v < N; v++) cls[v] = (uint8_t)(rng32() % 6u < 4u ? 0 : (rng32() & 1u) + 1);
    const int nch = (mask & 1) ? (int)(rng32() % (uint32_t)(N + 1)) : N;
    CHECK(qldpc_code_export_edges(code, var, chk) == QLDPC_OK);
    for (int c = 0; c < M; c++) u[c] = (mask & 2) ? bit_of(synd, c) : 0;
    for (int e = 0; e < E; e++) {
        const int v = var[e], c = chk[e];
        const int kn = (mask & 8) ? bit_of(known, v) : 0, er = (mask & 4) ? bit_of(erase, v) : 0, cl = (mask & 1) ? cls[v] : 0;
        int state;      /* 0 exact, 1 erased, 2 noisy */
        if (kn) state = 0;
        else if (cl == 2 || er) state = 1;
        else if (cl == 1 || v >= nch) state = 0;
        else state = 2;
        if (state == 1) dead[c] = 1;
        if (state == 2) d[c]++;
        u[c] ^= kn ? bit_of(value, v) : bit_of(bits, v);
    }
    for (int c = 0; c < M; c++)
        if (!dead[c]) { want[2 * d[c]]++; want[2 * d[c] + 1] += (uint32_t)u[c]; }
    CHECK(qldpc_qber_counts_host(code, bits, (mask & 1) ? cls : NULL, nch, (mask & 2) ? synd : NULL, (mask & 4) ? erase : NULL, (mask & 8) ? known : NULL,
                                 (mask & 8) ? value : NULL, got) == QLDPC_OK);
    CHECK(memcmp(got, want, sizeof(uint32_t) * 2 * (size_t)(D + 1)) == 0);
    free(bits); free(erase); free(known); free(value); free(synd); free(cls); free(var); free(chk); free(got); free(want); free(d); free(u); free(dead);
    return 0;
}

static int tables_and_argmax(int D, int n_grid)
{
    const size_t cells = (size_t)(D + 1) * (size_t)n_grid;
    int32_t *L1 = malloc(sizeof(int32_t) * cells), *L0 = malloc(sizeof(int32_t) * cells);
    float *q = malloc(sizeof(float) * (size_t)n_grid), *llr = malloc(sizeof(float) * (size_t)n_grid);
    uint64_t *cnt = calloc(2 * (size_t)(D + 1), sizeof(uint64_t));
    int k = 7;
    CHECK(qldpc_qber_table_host(D, n_grid, 0.001f, 0.25f, L1, L0, q, llr) == QLDPC_OK);
    CHECK(qldpc_qber_table_host(D, n_grid, 0.001f, 0.25f, NULL, NULL, NULL, NULL) == QLDPC_OK);
    for (int i = 1; i < n_grid; i++) CHECK(q[i] > q[i - 1] && llr[i] < llr[i - 1]);
    for (int d = 1; d <= D; d++) CHECK(L1[(size_t)d * n_grid] < 0 && L0[(size_t)d * n_grid] < 0 && L1[(size_t)d * n_grid + n_grid - 1] > L1[(size_t)d * n_grid]);
    CHECK(qldpc_qber_argmax_host(cnt, D, n_grid, L1, L0, &k) == QLDPC_OK && k == -1);
    cnt[2 * D] = 1000;                               /* all satisfied */
    CHECK(qldpc_qber_argmax_host(cnt, D, n_grid, L1, L0, &k) == QLDPC_OK && k == 0);
    cnt[2 * D] = (1ull << 35) - 1; cnt[2 * D + 1] = (1ull << 34);      /* the largest score the bound admits: no signed overflow */
    CHECK(qldpc_qber_argmax_host(cnt, D, n_grid, L1, L0, &k) == QLDPC_OK && k > 0 && (D > 12 || k == n_grid - 1));      /* high degrees saturate at 1/2: ties, lowest k */
    cnt[2 * D] = 1ull << 35;
    CHECK(qldpc_qber_argmax_host(cnt, D, n_grid, L1, L0, &k) == QLDPC_EINVAL);
    for (int i = 0; i < 50; i++) {                   /* a peak inside the grid for every mix of degrees */
        uint64_t tot = 0;
        for (int d = 0; d <= D; d++) { cnt[2 * d] = rng32() % 5000u; cnt[2 * d + 1] = cnt[2 * d] * (rng32() % 30u) / 100u; if (d) tot += cnt[2 * d]; }
        CHECK(qldpc_qber_argmax_host(cnt, D, n_grid, L1, L0, &k) == QLDPC_OK && (tot ? (k >= 0 && k < n_grid) : k == -1));
    }
    CHECK(qldpc_qber_table_host(D, 1, 0.001f, 0.25f, L1, L0, q, llr) == QLDPC_EINVAL);
    CHECK(qldpc_qber_table_host(64, n_grid, 0.001f, 0.25f, NULL, NULL, NULL, NULL) == QLDPC_EUNSUPPORTED);
    free(L1); free(L0); free(q); free(llr); free(cnt);
    return 0;
}

int main(void)
{
    /* N = 45, M = 7 (N no multiple of 32), and a small IRA code */
    int var[46], chk[46], E = 0;
    for (int v = 0; v < 44; v++) { var[E] = v; chk[E++] = v % 7; }
    var[E] = 44; chk[E++] = 0; var[E] = 44; chk[E++] = 6;
    qldpc_code *toy = NULL, *ira = NULL;
    CHECK(qldpc_code_from_edges(45, 7, E, var, chk, &toy) == QLDPC_OK);
    CHECK(qldpc_code_ira(330, 257, 0.125f, 11, 3, 7, &ira) == QLDPC_OK);
    for (int mask = 0; mask < 16; mask++)
        for (int rep = 0; rep < 4; rep++)
            if (one_case(toy, mask) || one_case(ira, mask)) return 1;
    uint32_t few[2] = {0, 0}, out[18];
    CHECK(qldpc_qber_counts_host(toy, few, NULL, 45, NULL, NULL, few, NULL, out) == QLDPC_EINVAL);      /* known without value */
    CHECK(qldpc_qber_counts_host(NULL, few, NULL, 45, NULL, NULL, NULL, NULL, out) == QLDPC_EINVAL);
    if (tables_and_argmax(qldpc_code_max_cn_degree(toy), 2) || tables_and_argmax(qldpc_code_max_cn_degree(ira), 256) || tables_and_argmax(63, 1024)) return 1;
    qldpc_code_free(toy);
    qldpc_code_free(ira);
    printf("sanitizer pass ok\n");
    return 0;
}
