/* Sanitizer pass over the host side of the blind reconciliation rounds (qldpc_mc_blind_next_host and qldpc_mc_blind_efficiency_host in
 * qldpc_mc_host.c over qldpc_mc_core.h, no HIP): the schedule driven launch by launch to the end of made-up runs, as qldpc_mc_blind drives it,
 * over a pool vector of exactly max_rounds + 1 counts; at every launch the rule's invariants (the deepest full level first, input before the
 * flush, the flush from the lowest level and all of it, no pool at 2 batch), and at the end every pool empty and every frame accounted for.
 * Built with -fsanitize=address,undefined by tests/test_mc_blind.py */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "qldpc.h"
#include "qldpc_mc_core.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

static uint64_t state = 0x13198A2E03707344ull;
static uint32_t next(uint32_t below)
{
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(state >> 33) % below;
}

static int drive(int R, int batch, uint64_t input, unsigned open_percent)
{
    uint64_t *pool = malloc(sizeof(uint64_t) * (size_t)(R + 1));
    uint64_t left = input, drawn = 0, ended = 0, decodes = 0, launches = 0;
    memset(pool, 0, sizeof(uint64_t) * (size_t)(R + 1));
    pool[0] = 0xDEADBEEFull;      /* not read */
    for (;;) {
        int level = -1, n = -1;
        const int got = qldpc_mc_blind_next_host(R, batch, pool, left, &level, &n);
        CHECK(got == 0 || got == 1);
        if (!got) break;
        CHECK(++launches <= (input + 1) * (uint64_t)(R + 1));      /* every launch decodes at least one frame, a frame at most R + 1 times */
        CHECK(level >= 0 && level <= R && n >= 1 && n <= batch);
        int deepest_full = 0, lowest = 0;
        for (int r = R; r >= 1; r--) if (pool[r] >= (uint64_t)batch && !deepest_full) deepest_full = r;
        for (int r = 1; r <= R; r++) if (pool[r] && !lowest) lowest = r;
        if (deepest_full) CHECK(level == deepest_full && n == batch);
        else if (left) CHECK(level == 0 && (uint64_t)n == (left < (uint64_t)batch ? left : (uint64_t)batch));
        else CHECK(level == lowest && (uint64_t)n == pool[level]);
        uint64_t on = 0;
        for (int i = 0; i < n; i++) on += next(100) < open_percent;
        if (level == 0) { left -= (uint64_t)n; drawn += (uint64_t)n; } else pool[level] -= (uint64_t)n;
        if (level < R) { pool[level + 1] += on; CHECK(pool[level + 1] < 2 * (uint64_t)batch); ended += (uint64_t)n - on; }
        else ended += (uint64_t)n;
        decodes += (uint64_t)n;
    }
    for (int r = 1; r <= R; r++) CHECK(pool[r] == 0);
    CHECK(left == 0 && drawn == input && ended == input && decodes >= input && pool[0] == 0xDEADBEEFull);
    free(pool);
    return 0;
}

int main(void)
{
    int cases = 0;
    for (int i = 0; i < 400; i++, cases++)
        if (drive((int)next(9), 1 + (int)next(80), next(3000), next(101))) return 1;
    /* the sizes of the GPU suite, one round, the deepest pool vector, nothing closes, everything closes, input above 2^32 in one step */
    if (drive(3, 192, 192, 60) || drive(3, 64, 192, 60) || drive(3, 40, 192, 60) || drive(2, 5, 16, 100) || drive(0, 64, 500, 50)) return 1;
    if (drive(QLDPC_MC_BLIND_MAX_ROUNDS, 3, 200, 97) || drive(4, 4096, 20000, 100) || drive(4, 4096, 20000, 0)) return 1;
    cases += 8;
    {
        uint64_t pool[2] = {0, 0};
        int level = -1, n = -1;
        CHECK(qldpc_mc_blind_next_host(1, 4096, pool, 4294967296ull + 5, &level, &n) == 1 && level == 0 && n == 4096);
    }
    /* argument checks: nothing is written */
    uint64_t pool[3] = {0, 9, 9};
    int level = -7, n = -7;
    CHECK(qldpc_mc_blind_next_host(-1, 4, pool, 1, &level, &n) == QLDPC_ESIZE);
    CHECK(qldpc_mc_blind_next_host(QLDPC_MC_BLIND_MAX_ROUNDS + 1, 4, pool, 1, &level, &n) == QLDPC_ESIZE);
    CHECK(qldpc_mc_blind_next_host(2, 0, pool, 1, &level, &n) == QLDPC_ESIZE);
    CHECK(strstr(qldpc_last_error(), "batch=0") != NULL);
    CHECK(qldpc_mc_blind_next_host(2, 4, NULL, 1, &level, &n) == QLDPC_EINVAL);
    CHECK(qldpc_mc_blind_next_host(2, 4, pool, 1, NULL, &n) == QLDPC_EINVAL);
    CHECK(qldpc_mc_blind_next_host(2, 4, pool, 1, &level, NULL) == QLDPC_EINVAL);
    CHECK(level == -7 && n == -7);
    CHECK(qldpc_mc_blind_next_host(2, 4, pool, 1, &level, &n) == 1 && level == 2 && n == 4);
    double f = -1.0;
    CHECK(qldpc_mc_blind_efficiency_host(0, 0, 1, 0, 0.1, &f) == QLDPC_ESIZE);
    CHECK(qldpc_mc_blind_efficiency_host(8, -1, 1, 0, 0.1, &f) == QLDPC_ESIZE);
    CHECK(qldpc_mc_blind_efficiency_host(8, 0, 0, 0, 0.1, &f) == QLDPC_ESIZE);
    CHECK(qldpc_mc_blind_efficiency_host(8, 0, 1, 0, 0.5, &f) == QLDPC_ESIZE);
    CHECK(qldpc_mc_blind_efficiency_host(8, 0, 1, 0, 0.1, NULL) == QLDPC_EINVAL);
    CHECK(f == -1.0);
    CHECK(qldpc_mc_blind_efficiency_host(8, 4, 1, 0, 0.11002786443835955, &f) == QLDPC_OK && fabs(f - 1.0) < 1e-12);
    CHECK(qldpc_mc_blind_efficiency_host(8, 0, 2, 8, 0.11002786443835955, &f) == QLDPC_OK && fabs(f - 1.0) < 1e-12);
    printf("sanitizer pass ok: %d cases\n", cases);
    return 0;
}
