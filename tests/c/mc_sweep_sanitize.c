/* Sanitizer pass over the host side of the QBER sweep (qldpc_mc_sweep_deal_host in qldpc_mc_host.c over qldpc_mc_core.h, no HIP): the deal
 * driven round by round to termination over made-up failure tables, as qldpc_mc_sweep drives it, into arrays of exactly n_points entries; after
 * every round the definition's invariants (a closed point receives nothing, nobody more than it needs, the slots are used while anybody
 * needs one, two open points differ by at most one chunk unless need caps the lower one), and at the end every point closed.
 * Built with -fsanitize=address,undefined by tests/test_mc_sweep.py */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "qldpc.h"
#include "qldpc_mc_core.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

static uint64_t state = 0x243F6A8885A308D3ull;
static uint32_t next(uint32_t below)
{
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(state >> 33) % below;
}

static uint64_t need_of(uint64_t done, uint64_t fe, int C, uint64_t max_frames, uint64_t max_fe)
{
    if (done >= max_frames || (max_fe && fe >= max_fe)) return 0;
    return (max_frames - done) / (uint64_t)C + ((max_frames - done) % (uint64_t)C != 0);
}

static int drive(int P, int C, int S, uint64_t max_frames, uint64_t max_fe, uint64_t first_done, unsigned fail_percent)
{
    uint64_t *done = malloc(sizeof(uint64_t) * (size_t)P), *fe = malloc(sizeof(uint64_t) * (size_t)P);
    int *give = malloc(sizeof(int) * (size_t)P);
    for (int q = 0; q < P; q++) { done[q] = first_done; fe[q] = 0; }
    for (uint64_t round = 0;; round++) {
        CHECK(round <= (uint64_t)P * (max_frames - first_done) + 1);      /* every round decodes at least one frame */
        const int used = qldpc_mc_sweep_deal_host(P, C, S, max_frames, max_fe, done, fe, give);
        CHECK(used >= 0 && used <= S);
        uint64_t wanted = 0;
        int sum = 0;
        for (int q = 0; q < P; q++) {
            const uint64_t need = need_of(done[q], fe[q], C, max_frames, max_fe);
            CHECK(give[q] >= 0 && (uint64_t)give[q] <= need);
            wanted += need; sum += give[q];
            for (int r = 0; r < q && P <= 64; r++) {      /* ascending q is served first: a lower point is behind a higher one only where its need caps it */
                const uint64_t need_r = need_of(done[r], fe[r], C, max_frames, max_fe);
                if (need && need_r) CHECK(give[r] >= give[q] || (uint64_t)give[r] == need_r);
                if (need && need_r) CHECK(give[r] <= give[q] + 1 || (uint64_t)give[q] == need);
            }
        }
        CHECK(sum == used && (uint64_t)used == (wanted < (uint64_t)S ? wanted : (uint64_t)S));
        if (used == 0) break;
        for (int q = 0; q < P; q++) {
            uint64_t n = (uint64_t)give[q] * (uint64_t)C;
            if (n > max_frames - done[q]) n = max_frames - done[q];
            for (uint64_t k = 0; k < n; k++) fe[q] += next(100) < fail_percent * (unsigned)(q + 1) / (unsigned)P;
            done[q] += n;
        }
    }
    for (int q = 0; q < P; q++) CHECK(done[q] == max_frames || (max_fe && fe[q] >= max_fe));
    free(done); free(fe); free(give);
    return 0;
}

int main(void)
{
    int cases = 0;
    for (int i = 0; i < 300; i++, cases++) {
        const int P = 1 + (int)next(20), C = 1 + (int)next(24), S = 1 + (int)next(16);
        if (drive(P, C, S, 1 + next(600), next(30), 0, next(101))) return 1;
    }
    /* the sizes of the GPU suite, one open point among closed ones, one slot, and frame counts above 2^32 */
    if (drive(4, 16, 12, 250, 60, 0, 60) || drive(7, 8, 4, 100, 5, 0, 50) || drive(1, 192, 1, 500, 0, 0, 10) || drive(3, 1, 1, 7, 1, 0, 100)) return 1;
    if (drive(5, 64, 9, 4294967296ull + 1000, 3, 4294967296ull - 900, 40) || drive(QLDPC_MC_SWEEP_MAX_POINTS, 4, 64, 9, 0, 0, 0)) return 1;
    cases += 6;
    /* argument checks: give is not written */
    uint64_t z[2] = {0, 0};
    int give[2] = {-7, -7};
    CHECK(qldpc_mc_sweep_deal_host(0, 4, 4, 10, 0, z, z, give) == QLDPC_ESIZE);
    CHECK(qldpc_mc_sweep_deal_host(QLDPC_MC_SWEEP_MAX_POINTS + 1, 4, 4, 10, 0, z, z, give) == QLDPC_ESIZE);
    CHECK(qldpc_mc_sweep_deal_host(2, 0, 4, 10, 0, z, z, give) == QLDPC_ESIZE);
    CHECK(qldpc_mc_sweep_deal_host(2, 4, 0, 10, 0, z, z, give) == QLDPC_ESIZE);
    CHECK(qldpc_mc_sweep_deal_host(2, 4, 4, 0, 0, z, z, give) == QLDPC_ESIZE);
    CHECK(strstr(qldpc_last_error(), "max_frames=0") != NULL);
    CHECK(qldpc_mc_sweep_deal_host(2, 4, 4, 10, 0, NULL, z, give) == QLDPC_EINVAL);
    CHECK(qldpc_mc_sweep_deal_host(2, 4, 4, 10, 0, z, z, NULL) == QLDPC_EINVAL);
    CHECK(give[0] == -7 && give[1] == -7);
    CHECK(qldpc_mc_sweep_deal_host(2, 4, 3, 10, 0, z, z, give) == 3 && give[0] == 2 && give[1] == 1);
    printf("sanitizer pass ok: %d cases\n", cases);
    return 0;
}
