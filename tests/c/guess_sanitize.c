/* Sanitizer pass over the host side of the guessing rounds (qldpc_guess_trial_host and qldpc_guess_pick_host in qldpc_guess_host.c over
 * qldpc_guess_core.h; qldpc_mc_guess_next_host in qldpc_mc_host.c over qldpc_mc_core.h; no HIP): the mirrors over made-up rows held in buffers of
 * exactly ceil(N / 32) words against a restatement bit by bit, and the schedule driven launch by launch to the end of made-up runs, as
 * qldpc_mc_guess drives it, with the rule's invariants at every launch.  Built with -fsanitize=address,undefined by tests/test_guess_host.py */
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

static int bit(const uint32_t *row, int v) { return (int)((row[v >> 5] >> (31 - (v & 31))) & 1u); }
static void set(uint32_t *row, int v) { row[v >> 5] |= 0x80000000u >> (v & 31); }

/* one source of N VNs with `members` VNs in its guess set, the first of them at `from` or later */
static int rows(int N, int g, int members, int from)
{
    const int W = (N + 31) / 32, T = 1 << g;
    uint32_t *weak = calloc((size_t)W, 4), *hard = calloc((size_t)W, 4), *known = malloc((size_t)W * 4), *value = malloc((size_t)W * 4);
    uint32_t *trial_hard = malloc((size_t)T * (size_t)W * 4);
    int *ok = malloc((size_t)T * sizeof(int));
    for (int i = 0; i < members; i++) set(weak, from + (int)next((uint32_t)(N - from)));
    for (int v = 0; v < N; v++) if (next(2)) set(hard, v);
    for (int t = 0; t < T; t += 1 + (T > 64 ? (int)next(9) : 0)) {
        CHECK(qldpc_guess_trial_host(N, g, t, weak, hard, known, value) == QLDPC_OK);
        int rank = 0;
        for (int v = 0; v < N; v++) {
            CHECK(bit(known, v) == bit(weak, v));
            if (!bit(weak, v)) { CHECK(bit(value, v) == 0); continue; }
            CHECK(bit(value, v) == (bit(hard, v) ^ ((t >> rank) & 1)));
            rank++;
        }
    }
    /* the verdict: a few ok trials, some with another row, some with differences in the padding alone */
    const uint32_t pad = (N & 31) ? ~(0xffffffffu << (32 - (N & 31))) : 0u;
    int want_w = -1, want_n = 0, want_a = 0;
    for (int t = 0; t < T; t++) {
        memcpy(trial_hard + (size_t)t * W, hard, (size_t)W * 4);
        ok[t] = next(4) == 0;
        if (next(3) == 0) trial_hard[(size_t)t * W + (W - 1)] ^= next(0xffffffffu) & pad;
        if (next(5) == 0) trial_hard[(size_t)t * W + next((uint32_t)W)] ^= 0x80000000u >> (next(32));
    }
    for (int t = 0; t < T; t++) if (ok[t]) { if (want_w < 0) want_w = t; want_n++; }
    for (int t = 0; t < T && want_w >= 0; t++)
        for (int v = 0; v < N && ok[t]; v++) want_a |= bit(trial_hard + (size_t)t * W, v) != bit(trial_hard + (size_t)want_w * W, v);
    int w = -9, n = -9, a = -9;
    CHECK(qldpc_guess_pick_host(N, g, ok, trial_hard, &w, &n, &a) == QLDPC_OK);
    CHECK(w == want_w && n == want_n && a == want_a);
    free(weak); free(hard); free(known); free(value); free(trial_hard); free(ok);
    return 0;
}

static int drive(int g, int batch, uint64_t input, unsigned fail_percent)
{
    const uint64_t S = (uint64_t)batch >> g;
    uint64_t pool = 0, left = input, drawn = 0, tried = 0, failed = 0, launches = 0;
    for (;;) {
        int kind = -1, n = -1;
        const int got = qldpc_mc_guess_next_host(g, batch, pool, left, &kind, &n);
        CHECK(got == 0 || got == 1);
        if (!got) break;
        CHECK(++launches <= 2 * (input + 1));
        if (pool && pool >= S) CHECK(kind == QLDPC_MC_GUESS_TRIALS && (uint64_t)n == S);
        else if (left) CHECK(kind == QLDPC_MC_GUESS_FRESH && (uint64_t)n == (left < (uint64_t)batch ? left : (uint64_t)batch));
        else CHECK(kind == QLDPC_MC_GUESS_TRIALS && (uint64_t)n == pool);
        if (kind == QLDPC_MC_GUESS_FRESH) {
            uint64_t on = 0;
            for (int i = 0; i < n; i++) on += next(100) < fail_percent;
            left -= (uint64_t)n; drawn += (uint64_t)n; failed += on;
            if (g) pool += on;
            CHECK(pool < S + (uint64_t)batch && pool <= MC_GUESS_POOL_CAP(batch));
        } else {
            CHECK(n >= 1 && (uint64_t)n <= pool && ((uint64_t)n << g) <= (uint64_t)batch);
            pool -= (uint64_t)n; tried += (uint64_t)n;
        }
    }
    CHECK(pool == 0 && left == 0 && drawn == input && tried == (g ? failed : 0));
    return 0;
}

int main(void)
{
    int cases = 0;
    const int sizes[] = {1, 20, 32, 33, 1008, 2049, 8300};
    for (unsigned i = 0; i < sizeof sizes / sizeof *sizes; i++)
        for (int g = 0; g <= QLDPC_GUESS_MAX_BITS; g++, cases++) {
            const int N = sizes[i];
            if (rows(N, g, g, 0) || rows(N, g, g / 2, 0) || rows(N, g, g, N - 1 - (N - 1) % 32) || rows(N, g, 0, 0)) return 1;
            if (N > 2048 && rows(N, g, g, 2040)) return 1;
        }
    for (int i = 0; i < 400; i++, cases++) {
        const int g = (int)next(QLDPC_GUESS_MAX_BITS + 1);
        if (drive(g, (1 << g) + (int)next(5u << g), next(3000), next(101))) return 1;
    }
    /* the sizes of the GPU suite, g = 0, one source per launch, nothing fails, everything fails */
    if (drive(3, 192, 192, 60) || drive(3, 64, 192, 60) || drive(3, 40, 192, 60) || drive(0, 64, 500, 50) || drive(10, 1024, 5000, 30)) return 1;
    if (drive(8, 4096, 20000, 0) || drive(8, 4096, 20000, 100) || drive(1, 2, 100, 100)) return 1;
    cases += 8;
    /* argument checks: nothing is written */
    uint32_t row[2] = {0, 0}, out[2] = {77, 77};
    int ok[8] = {0}, kind = -7, n = -7, w = -7;
    CHECK(qldpc_guess_trial_host(0, 3, 0, row, row, out, out) == QLDPC_ESIZE);
    CHECK(qldpc_guess_trial_host(40, QLDPC_GUESS_MAX_BITS + 1, 0, row, row, out, out) == QLDPC_ESIZE);
    CHECK(qldpc_guess_trial_host(40, -1, 0, row, row, out, out) == QLDPC_ESIZE);
    CHECK(qldpc_guess_trial_host(40, 3, 8, row, row, out, out) == QLDPC_ESIZE && strstr(qldpc_last_error(), "trial 8") != NULL);
    CHECK(qldpc_guess_trial_host(40, 3, -1, row, row, out, out) == QLDPC_ESIZE);
    CHECK(qldpc_guess_trial_host(40, 3, 0, NULL, row, out, out) == QLDPC_EINVAL && qldpc_guess_trial_host(40, 3, 0, row, row, out, NULL) == QLDPC_EINVAL);
    CHECK(out[0] == 77 && out[1] == 77);
    CHECK(qldpc_guess_pick_host(40, 3, NULL, row, &w, &w, &w) == QLDPC_EINVAL && qldpc_guess_pick_host(40, 3, ok, row, &w, NULL, &w) == QLDPC_EINVAL);
    CHECK(qldpc_guess_pick_host(0, 3, ok, row, &w, &w, &w) == QLDPC_ESIZE && qldpc_guess_pick_host(40, 11, ok, row, &w, &w, &w) == QLDPC_ESIZE);
    CHECK(qldpc_mc_guess_next_host(-1, 8, 0, 1, &kind, &n) == QLDPC_ESIZE && qldpc_mc_guess_next_host(QLDPC_GUESS_MAX_BITS + 1, 4096, 0, 1, &kind, &n) == QLDPC_ESIZE);
    CHECK(qldpc_mc_guess_next_host(3, 7, 0, 1, &kind, &n) == QLDPC_ESIZE && qldpc_mc_guess_next_host(0, 0, 0, 1, &kind, &n) == QLDPC_ESIZE);
    CHECK(qldpc_mc_guess_next_host(3, 8, 0, 1, NULL, &n) == QLDPC_EINVAL && qldpc_mc_guess_next_host(3, 8, 0, 1, &kind, NULL) == QLDPC_EINVAL);
    CHECK(kind == -7 && n == -7 && w == -7);
    CHECK(qldpc_mc_guess_next_host(3, 8, 0, 4294967296ull + 5, &kind, &n) == 1 && kind == QLDPC_MC_GUESS_FRESH && n == 8);
    printf("sanitizer pass ok: %d cases\n", cases);
    return 0;
}
