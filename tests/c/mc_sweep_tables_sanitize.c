/* Sanitizer pass over the host side of the sweep over table channels (qldpc_mc_sweep_tables_check_host in qldpc_mc_host.c and mc_soft_table_build of
 * qldpc_mc_core.h, no HIP): P tables of mixed level counts whose arrays are allocated with exactly levels - 1 and levels entries, so that a read past
 * either end is caught; every table built as qldpc_mc_sweep_tables builds it and its levels compared with the definition #{k : u >= cum[b][k]};
 * the check function over accepted configurations (P = 1, P = QLDPC_MC_SWEEP_MAX_POINTS, no order) and over every refusal with its code.
 * Built with -fsanitize=address,undefined by tests/test_mc_sweep_tables.py */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "qldpc.h"
#include "qldpc_mc_core.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)
#define TWO32 4294967296ull

static uint64_t state = 0x13198A2E03707344ull;
static uint64_t next(uint64_t below)
{
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (state >> 20) % below;
}

static int by_value(const void *a, const void *b) { const uint64_t x = *(const uint64_t *)a, y = *(const uint64_t *)b; return x < y ? -1 : x > y; }

/* a table of `levels` levels in arrays of exactly the sizes the definition reads; `ends`: the rows start with 0 and end with 2^32 */
static int make_table(qldpc_mc_table_point *pt, int levels, int ends)
{
    uint64_t *cum[2];
    for (int b = 0; b < 2; b++) {
        cum[b] = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)(levels - 1));
        CHECK(cum[b]);
        for (int k = 0; k < levels - 1; k++) cum[b][k] = next(TWO32 + 1);
        if (ends) { cum[b][0] = 0; cum[b][levels - 2] = TWO32; }
        if (levels > 8) cum[b][3] = cum[b][4] = cum[b][5];      /* a run of equal thresholds */
        qsort(cum[b], (size_t)(levels - 1), sizeof(uint64_t), by_value);
    }
    float *value = (float *)malloc(sizeof(float) * (size_t)levels);
    CHECK(value);
    for (int l = 0; l < levels; l++) value[l] = (float)l - 0.5f * (float)levels;
    memset(pt, 0, sizeof(*pt));
    pt->table.levels = levels; pt->table.cum[0] = cum[0]; pt->table.cum[1] = cum[1]; pt->table.value = value;
    return 0;
}

static void free_table(qldpc_mc_table_point *pt)
{
    free((void *)pt->table.cum[0]); free((void *)pt->table.cum[1]); free((void *)pt->table.value);
}

/* the built table against the definition, at the thresholds, next to them and at random words */
static int built_equals_definition(const qldpc_mc_table_point *pt)
{
    mc_soft_table *t = (mc_soft_table *)malloc(sizeof(*t));
    CHECK(t);
    const int L = pt->table.levels;
    CHECK(mc_soft_table_build(L, pt->table.cum[0], pt->table.cum[1], pt->table.value, t) == 0);
    CHECK(t->levels == (uint32_t)L);
    for (int b = 0; b < 2; b++) {
        uint32_t live = 0;
        for (int k = 0; k < L - 1; k++) live += pt->table.cum[b][k] < TWO32;
        CHECK(t->live[b] == live);
        for (int i = 0; i < 3 * (L - 1) + 64; i++) {
            const uint64_t c = i < 3 * (L - 1) ? pt->table.cum[b][i / 3] + (uint64_t)(i % 3) - 1u : next(TWO32);      /* cum - 1, cum, cum + 1 */
            if (c >= TWO32) continue;      /* also cum = 0 minus one */
            uint32_t level = 0;
            for (int k = 0; k < L - 1; k++) level += c >= pt->table.cum[b][k];
            CHECK(mc_soft_level(t->thr[b], t->live[b], (uint32_t)c) == level);
            CHECK(t->value[level] == pt->table.value[level]);
        }
    }
    for (int l = L; l < MC_SOFT_MAX_LEVELS; l++) CHECK(t->value[l] == 0.0f);
    free(t);
    return 0;
}

int main(void)
{
    enum { N = 1998, BATCH = 192, P = 9 };
    static const int levels[P] = {2, 64, 256, 3, 255, 17, 2, 128, 9};
    qldpc_mc_table_point pts[P];
    for (int q = 0; q < P; q++) {
        if (make_table(&pts[q], levels[q], q & 1) || built_equals_definition(&pts[q])) return 1;
        pts[q].label = 0.25 * q;
    }
    int order[60];
    for (int i = 0; i < 60; i++) order[i] = (N - 1) - 7 * i;      /* not ascending */
    for (int q = 0; q < P; q++) pts[q].n_punct = 60 * q / (P - 1);
    qldpc_mc_sweep_tables_cfg cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.points = pts; cfg.n_points = P; cfg.punct_order = order; cfg.n_order = 60; cfg.chunk = 32; cfg.max_frames = 150;
    CHECK(qldpc_mc_sweep_tables_check_host(N, BATCH, &cfg) == QLDPC_OK);
    cfg.chunk = 0; CHECK(qldpc_mc_sweep_tables_check_host(N, BATCH, &cfg) == QLDPC_OK);
    cfg.chunk = BATCH; CHECK(qldpc_mc_sweep_tables_check_host(N, BATCH, &cfg) == QLDPC_OK);
    cfg.n_points = 1; CHECK(qldpc_mc_sweep_tables_check_host(N, BATCH, &cfg) == QLDPC_OK);
    cfg.n_points = P;

    /* refusals, each undone before the next */
    cfg.chunk = BATCH + 1; CHECK(qldpc_mc_sweep_tables_check_host(N, BATCH, &cfg) == QLDPC_ESIZE);
    cfg.chunk = -1; CHECK(qldpc_mc_sweep_tables_check_host(N, BATCH, &cfg) == QLDPC_ESIZE);
    cfg.chunk = 32;
    cfg.max_frames = 0; CHECK(qldpc_mc_sweep_tables_check_host(N, BATCH, &cfg) == QLDPC_ESIZE && strstr(qldpc_last_error(), "max_frames=0"));
    cfg.max_frames = 150;
    cfg.n_points = 0; CHECK(qldpc_mc_sweep_tables_check_host(N, BATCH, &cfg) == QLDPC_ESIZE);
    cfg.n_points = QLDPC_MC_SWEEP_MAX_POINTS + 1; CHECK(qldpc_mc_sweep_tables_check_host(N, BATCH, &cfg) == QLDPC_ESIZE);      /* refused before a point is read */
    cfg.n_points = P;
    cfg.reserved[1] = 1; CHECK(qldpc_mc_sweep_tables_check_host(N, BATCH, &cfg) == QLDPC_EINVAL);
    cfg.reserved[1] = 0;
    pts[4].reserved = 1; CHECK(qldpc_mc_sweep_tables_check_host(N, BATCH, &cfg) == QLDPC_EINVAL);
    pts[4].reserved = 0;
    pts[4].table.reserved[0] = 1; CHECK(qldpc_mc_sweep_tables_check_host(N, BATCH, &cfg) == QLDPC_EINVAL);
    pts[4].table.reserved[0] = 0;
    pts[5].n_punct = 61; CHECK(qldpc_mc_sweep_tables_check_host(N, BATCH, &cfg) == QLDPC_ESIZE);
    pts[5].n_punct = -1; CHECK(qldpc_mc_sweep_tables_check_host(N, BATCH, &cfg) == QLDPC_ESIZE);
    pts[5].n_punct = 37;
    pts[3].table.levels = 1; CHECK(qldpc_mc_sweep_tables_check_host(N, BATCH, &cfg) == QLDPC_ESIZE);      /* the arrays are not read */
    pts[3].table.levels = 257; CHECK(qldpc_mc_sweep_tables_check_host(N, BATCH, &cfg) == QLDPC_ESIZE);
    pts[3].table.levels = 0; CHECK(qldpc_mc_sweep_tables_check_host(N, BATCH, &cfg) == QLDPC_ESIZE && strstr(qldpc_last_error(), "point 3"));
    pts[3].table.levels = 3;
    const float *value = pts[2].table.value;
    pts[2].table.value = NULL; CHECK(qldpc_mc_sweep_tables_check_host(N, BATCH, &cfg) == QLDPC_EINVAL);
    pts[2].table.value = value;
    const uint64_t *row = pts[2].table.cum[1];
    pts[2].table.cum[1] = NULL; CHECK(qldpc_mc_sweep_tables_check_host(N, BATCH, &cfg) == QLDPC_EINVAL);
    pts[2].table.cum[1] = row;
    uint64_t *w = (uint64_t *)pts[1].table.cum[0];
    const uint64_t was = w[10];
    w[10] = w[9] - 1; CHECK(w[9] > 0 && qldpc_mc_sweep_tables_check_host(N, BATCH, &cfg) == QLDPC_EINVAL);      /* a row that decreases */
    w[10] = was;
    const uint64_t last = w[62];
    w[62] = TWO32 + 1; CHECK(qldpc_mc_sweep_tables_check_host(N, BATCH, &cfg) == QLDPC_EINVAL);
    w[62] = last;
    order[59] = order[0]; CHECK(qldpc_mc_sweep_tables_check_host(N, BATCH, &cfg) == QLDPC_EINVAL);
    order[59] = N; CHECK(qldpc_mc_sweep_tables_check_host(N, BATCH, &cfg) == QLDPC_EINVAL);
    order[59] = -1; CHECK(qldpc_mc_sweep_tables_check_host(N, BATCH, &cfg) == QLDPC_EINVAL);
    order[59] = (N - 1) - 7 * 59;
    cfg.punct_order = NULL; CHECK(qldpc_mc_sweep_tables_check_host(N, BATCH, &cfg) == QLDPC_EINVAL);
    cfg.n_order = 0; CHECK(qldpc_mc_sweep_tables_check_host(N, BATCH, &cfg) == QLDPC_ESIZE);      /* no order: every n_punct must be 0 */
    for (int q = 0; q < P; q++) pts[q].n_punct = 0;
    CHECK(qldpc_mc_sweep_tables_check_host(N, BATCH, &cfg) == QLDPC_OK);
    cfg.points = NULL; CHECK(qldpc_mc_sweep_tables_check_host(N, BATCH, &cfg) == QLDPC_EINVAL);
    cfg.points = pts;
    CHECK(qldpc_mc_sweep_tables_check_host(N, BATCH, NULL) == QLDPC_EINVAL);
    CHECK(qldpc_mc_sweep_tables_check_host(1 << 20, 1 << 13, &cfg) == QLDPC_ESIZE && strstr(qldpc_last_error(), "2^31"));      /* 2^13 frames of 2^18 quads */
    CHECK(qldpc_mc_sweep_tables_check_host(1 << 20, (1 << 13) - 1, &cfg) == QLDPC_OK);
    CHECK(qldpc_mc_sweep_tables_check_host(N, BATCH, &cfg) == QLDPC_OK);      /* everything was undone */

    /* the largest sweep: QLDPC_MC_SWEEP_MAX_POINTS points that cycle through the P tables */
    qldpc_mc_table_point *many = (qldpc_mc_table_point *)malloc(sizeof(*many) * QLDPC_MC_SWEEP_MAX_POINTS);
    CHECK(many);
    for (int q = 0; q < QLDPC_MC_SWEEP_MAX_POINTS; q++) many[q] = pts[q % P];
    cfg.points = many; cfg.n_points = QLDPC_MC_SWEEP_MAX_POINTS;
    CHECK(qldpc_mc_sweep_tables_check_host(N, BATCH, &cfg) == QLDPC_OK);
    many[QLDPC_MC_SWEEP_MAX_POINTS - 1].table.levels = 300;
    CHECK(qldpc_mc_sweep_tables_check_host(N, BATCH, &cfg) == QLDPC_ESIZE);
    free(many);
    for (int q = 0; q < P; q++) free_table(&pts[q]);
    printf("sanitizer pass ok: %d tables\n", P);
    return 0;
}
