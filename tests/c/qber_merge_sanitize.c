/* Sanitizer pass over the merged form of the syndrome-weight QBER count (qldpc_qber_counts_merged_host and qldpc_qber_repeat_table_host in
 * qldpc_qber_host.c over qldpc_qber_core.h, no HIP; linked with qldpc_graph.c) on buffers allocated at their exact sizes, the counts against a per-VN
 * restatement of the rule.  Built with -fsanitize=address,undefined by tests/test_qber_merge_host.py */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "qldpc.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)
#define ROWS (QLDPC_QBER_MAX_DEGREE + 1)
#define MAX_RUN 16

static uint64_t rng_state = 0x243f6a8885a308d3ull;
static uint32_t rng32(void)
{
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return (uint32_t)((z ^ (z >> 31)) >> 16);
}

static int bit_of(const uint32_t *row, int v) { return row ? (int)((row[v >> 5] >> (31 - (v & 31))) & 1u) : 0; }
static void set_bit(uint32_t *row, int v, int b)
{
    row[v >> 5] &= ~(0x80000000u >> (v & 31));
    if (b) row[v >> 5] |= 0x80000000u >> (v & 31);
}

/* `shape` of the parity erasures: 0 - 3 every VN at 25 / 50 / 60 / 90 %, 4 the constructed cases: a run from check 0, runs of 16, 17 and 40 checks,
 * a known link inside a run, the last parity VN erased behind a link.  mask: 1 class map + n_channel, 2 syndrome, 8 known + value */
static int one_case(const qldpc_code *code, int mask, int shape)
{
    const int N = qldpc_code_n(code), M = qldpc_code_m(code), E = qldpc_code_e(code), K = N - M;
    const size_t Wn = (size_t)(N + 31) / 32, Wm = (size_t)(M + 31) / 32;
    uint32_t *bits = malloc(4 * Wn), *erase = malloc(4 * Wn), *known = malloc(4 * Wn), *value = malloc(4 * Wn), *synd = malloc(4 * Wm);
    uint8_t *cls = malloc((size_t)N);
    int *var = malloc(sizeof(int) * (size_t)E), *chk = malloc(sizeof(int) * (size_t)E), *ptr = calloc((size_t)M + 1, sizeof(int));
    int *state = malloc(sizeof(int) * (size_t)N), *val = malloc(sizeof(int) * (size_t)N), *mult = calloc((size_t)N, sizeof(int));
    uint32_t *got = malloc(sizeof(uint32_t) * 2 * ROWS), *want = calloc(2 * ROWS, sizeof(uint32_t));
    static const uint32_t dens[4] = {25, 50, 60, 90};
    for (size_t w = 0; w < Wn; w++) {      /* tail bits past N set at random on purpose */
        bits[w] = rng32() | (rng32() << 16);
        erase[w] = 0;
        known[w] = rng32() & rng32() & rng32() & (rng32() << 16 | rng32());
        value[w] = rng32() | (rng32() << 16);
    }
    erase[Wn - 1] = rng32();
    for (int v = 0; v < N; v++) set_bit(erase, v, v < K ? rng32() % 400u == 0 : (shape < 4 && rng32() % 100u < dens[shape]));
    if (shape == 4) {
        const int spans[5][2] = {{0, 3}, {8, 8 + 15}, {30, 30 + 16}, {60, 60 + 39}, {M - 3, M}};
        for (int s = 0; s < 5; s++)
            for (int c = spans[s][0]; c < spans[s][1] && c < M; c++) set_bit(erase, K + c, 1);
        set_bit(known, K + 1, 1);
        set_bit(known, K + 70, (mask & 8) != 0);
    }
    for (size_t w = 0; w < Wm; w++) synd[w] = rng32() | (rng32() << 16);
    for (int v = 0; v < N; v++) cls[v] = (uint8_t)(rng32() % 12u < 10u ? (v < K ? 0 : 1) : (rng32() & 1u) + 1);
    const int nch = (mask & 1) ? (int)(rng32() % (uint32_t)(N + 1)) : N;
    CHECK(qldpc_code_export_edges(code, var, chk) == QLDPC_OK);      /* check-major: the edges of check c are ptr[c] .. ptr[c + 1] - 1 */
    for (int e = 0; e < E; e++) ptr[chk[e] + 1]++;
    for (int c = 0; c < M; c++) ptr[c + 1] += ptr[c];
    for (int v = 0; v < N; v++) {      /* 0 exact, 1 erased, 2 noisy */
        const int kn = (mask & 8) ? bit_of(known, v) : 0, er = bit_of(erase, v), cl = (mask & 1) ? cls[v] : 0;
        state[v] = kn ? 0 : (cl == 2 || er) ? 1 : (cl == 1 || v >= nch) ? 0 : 2;
        val[v] = kn ? bit_of(value, v) : bit_of(bits, v);
    }
    for (int h = 0; h < M;) {
        int t = h;
        while (t < M - 1 && state[K + t] == 1) t++;
        int u = 0, d = 0, dead = t - h + 1 > MAX_RUN;
        for (int e = ptr[h]; e < ptr[t + 1]; e++) mult[var[e]]++;
        for (int c = h; c <= t; c++) u ^= (mask & 2) ? bit_of(synd, c) : 0;
        for (int e = ptr[h]; e < ptr[t + 1]; e++) {
            const int v = var[e], link = v >= K + h && v < K + t;
            if (!mult[v]) continue;      /* seen */
            if (!link) {
                if (state[v] == 1) dead = 1;
                if (state[v] == 2 && (mult[v] & 1)) d++;
                if (mult[v] & 1) u ^= val[v];
            } else CHECK(mult[v] == 2);
            mult[v] = 0;
        }
        if (!dead && d <= QLDPC_QBER_MAX_DEGREE) { want[2 * d]++; want[2 * d + 1] += (uint32_t)u; }
        h = t + 1;
    }
    CHECK(qldpc_qber_counts_merged_host(code, bits, (mask & 1) ? cls : NULL, nch, (mask & 2) ? synd : NULL, erase, (mask & 8) ? known : NULL,
                                        (mask & 8) ? value : NULL, got) == QLDPC_OK);
    CHECK(memcmp(got, want, sizeof(uint32_t) * 2 * ROWS) == 0);
    free(bits); free(erase); free(known); free(value); free(synd); free(cls); free(var); free(chk); free(ptr); free(state); free(val); free(mult);
    free(got); free(want);
    return 0;
}

int main(void)
{
    qldpc_code *small = NULL, *ira = NULL, *toy = NULL;
    CHECK(qldpc_code_ira(330, 257, 0.125f, 11, 3, 7, &small) == QLDPC_OK);      /* M = 73, K no multiple of 32 */
    CHECK(qldpc_code_ira(1280, 1024, 0.125f, 11, 3, 7, &ira) == QLDPC_OK);
    for (int mask = 0; mask < 16; mask++) {
        if (mask & 4) continue;
        for (int shape = 0; shape < 5; shape++)
            if ((shape < 4 && one_case(small, mask, shape)) || one_case(ira, mask, shape)) return 1;
    }
    /* the chain test on tables of its own: a chain of three checks, then each way of not being one */
    const int chain[3][3] = {{0, 1, 2}, {3, 3, 4}, {-1, 4, 5}};      /* tab[j][c]: N = 6, M = 3, K = 3; check 0 = {0, 3}, 1 = {1, 3, 4}, 2 = {2, 4, 5} */
    int tab[9];
    uint8_t rep[9];
    memcpy(tab, chain, sizeof(tab));
    CHECK(qldpc_qber_repeat_table_host(tab, 6, 3, 3, rep) == QLDPC_OK && rep[3 + 1] == 1 && rep[3 + 2] == 1 && rep[0] == 0 && rep[1] == 0);
    CHECK(qldpc_qber_repeat_table_host(tab, 6, 3, 3, NULL) == QLDPC_OK);
    tab[5] = 0;                                    /* check 2 lacks VN 4 */
    CHECK(qldpc_qber_repeat_table_host(tab, 6, 3, 3, rep) == QLDPC_EUNSUPPORTED);
    memcpy(tab, chain, sizeof(tab));
    tab[6] = 5;                                    /* check 0 holds the last parity VN */
    CHECK(qldpc_qber_repeat_table_host(tab, 6, 3, 3, rep) == QLDPC_EUNSUPPORTED);
    CHECK(qldpc_qber_repeat_table_host(tab, 2, 3, 3, rep) == QLDPC_EUNSUPPORTED);
    CHECK(qldpc_qber_repeat_table_host(NULL, 6, 3, 3, rep) == QLDPC_EINVAL);
    int var[46], chk[46], E = 0;
    for (int v = 0; v < 44; v++) { var[E] = v; chk[E++] = v % 7; }
    var[E] = 44; chk[E++] = 0; var[E] = 44; chk[E++] = 6;
    CHECK(qldpc_code_from_edges(45, 7, E, var, chk, &toy) == QLDPC_OK);
    uint32_t few[2] = {0, 0}, out[2 * ROWS];
    CHECK(qldpc_qber_counts_merged_host(toy, few, NULL, 45, NULL, NULL, NULL, NULL, out) == QLDPC_EUNSUPPORTED);
    CHECK(qldpc_qber_counts_merged_host(ira, few, NULL, 45, NULL, NULL, few, NULL, out) == QLDPC_EINVAL);      /* known without value */
    qldpc_code_free(small); qldpc_code_free(ira); qldpc_code_free(toy);
    printf("sanitizer pass ok\n");
    return 0;
}
