/* Sanitizer pass over the host side of the Monte-Carlo frame definition (qldpc_mc_host.c over qldpc_mc_core.h, no HIP): qldpc_mc_frames_host
 * at the edge sizes into buffers of exactly the size the call may write, ranges against their parts, and every argument check.
 * Built with -fsanitize=address,undefined by tests/test_mc.py */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "qldpc.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

static int popcount_words(const uint32_t *w, size_t n)
{
    int c = 0;
    for (size_t i = 0; i < n; i++) c += __builtin_popcount(w[i]);
    return c;
}

int main(void)
{
    static const struct { uint32_t c[4], k[2], o[4]; } kat[3] = {
        {{0, 0, 0, 0}, {0, 0}, {0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u}},
        {{0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}, {0xffffffffu, 0xffffffffu}, {0x408f276du, 0x41c83b0eu, 0xa20bc7c6u, 0x6d5451fdu}},
        {{0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u}, {0xa4093822u, 0x299f31d0u}, {0xd16cfe09u, 0x94fdccebu, 0x5001e420u, 0x24126ea1u}}};
    for (int i = 0; i < 3; i++) {
        uint32_t o[4];
        CHECK(qldpc_mc_philox_host(kat[i].c, kat[i].k, o) == QLDPC_OK && !memcmp(o, kat[i].o, sizeof(o)));
    }
    CHECK(qldpc_mc_philox_host(NULL, kat[0].k, (uint32_t[4]){0}) == QLDPC_EINVAL);

    static const int sizes[][2] = {{1, 1}, {1, 32}, {31, 33}, {32, 64}, {33, 65}, {504, 1008}, {1590, 2000}};
    static const uint64_t firsts[] = {0, 4294967196ull /* 2^32 - 100 */, 18446744073709551615ull /* wraps */};
    int cases = 0;
    for (size_t s = 0; s < sizeof(sizes) / sizeof(*sizes); s++)
        for (size_t a = 0; a < sizeof(firsts) / sizeof(*firsts); a++) {
            const int K = sizes[s][0], N = sizes[s][1], Wk = (K + 31) / 32, Wn = (N + 31) / 32, n = 5;
            const uint64_t first = firsts[a];
            int *pos = malloc(sizeof(int) * (size_t)K);
            uint8_t *cls = malloc((size_t)N);
            for (int i = 0; i < K; i++) pos[i] = N - K + i;                       /* info bits last, as the IDENTITY encoder places them */
            for (int v = 0; v < N; v++) cls[v] = (uint8_t)(v % 3);
            uint32_t *info = malloc(4 * (size_t)n * Wk), *flips = malloc(4 * (size_t)n * Wn), *part_i = malloc(4 * (size_t)n * Wk), *part_f = malloc(4 * (size_t)n * Wn);
            CHECK(qldpc_mc_frames_host(K, N, pos, NULL, 7, 0.11, 0.0, first, n, info, flips) == QLDPC_OK);
            /* a range equals its parts, and either output alone */
            CHECK(qldpc_mc_frames_host(K, N, pos, NULL, 7, 0.11, 0.0, first, 2, part_i, part_f) == QLDPC_OK);
            CHECK(qldpc_mc_frames_host(K, N, pos, NULL, 7, 0.11, 0.0, first + 2, 3, part_i + 2 * Wk, NULL) == QLDPC_OK);
            CHECK(qldpc_mc_frames_host(K, N, pos, NULL, 7, 0.11, 0.0, first + 2, 3, NULL, part_f + 2 * Wn) == QLDPC_OK);
            CHECK(!memcmp(info, part_i, 4 * (size_t)n * Wk) && !memcmp(flips, part_f, 4 * (size_t)n * Wn));
            for (int f = 0; f < n; f++) {
                if (K % 32) CHECK((info[(size_t)f * Wk + Wk - 1] & ((1u << (32 - K % 32)) - 1u)) == 0);
                if (N % 32) CHECK((flips[(size_t)f * Wn + Wn - 1] & ((1u << (32 - N % 32)) - 1u)) == 0);
                for (int v = 0; v < N - K; v++) CHECK(!(flips[(size_t)f * Wn + v / 32] & (0x80000000u >> (v % 32))));      /* pinned, parity_ber = 0 */
            }
            /* no flips at qber = 0; a class map of its own; n = 0 writes nothing (the buffers may be NULL-sized) */
            CHECK(qldpc_mc_frames_host(K, N, pos, NULL, 7, 0.0, 0.0, first, n, NULL, flips) == QLDPC_OK && popcount_words(flips, (size_t)n * Wn) == 0);
            CHECK(qldpc_mc_frames_host(K, N, NULL, cls, 7, 0.3, 0.2, first, n, NULL, flips) == QLDPC_OK);
            for (int f = 0; f < n; f++)
                for (int v = 2; v < N; v += 3) CHECK(!(flips[(size_t)f * Wn + v / 32] & (0x80000000u >> (v % 32))));       /* punctured */
            CHECK(qldpc_mc_frames_host(K, N, pos, cls, 7, 0.3, 0.2, first, 0, info, flips) == QLDPC_OK);
            /* argument checks: nothing is written */
            memset(info, 0x5a, 4 * (size_t)n * Wk);
            memcpy(part_i, info, 4 * (size_t)n * Wk);
            CHECK(qldpc_mc_frames_host(K, N, pos, NULL, 7, -0.01, 0.0, first, n, info, flips) == QLDPC_ESIZE);
            CHECK(qldpc_mc_frames_host(K, N, pos, NULL, 7, 1.0, 0.0, first, n, info, flips) == QLDPC_ESIZE);
            CHECK(qldpc_mc_frames_host(K, N, pos, NULL, 7, NAN, 0.0, first, n, info, flips) == QLDPC_ESIZE);
            CHECK(qldpc_mc_frames_host(K, N, pos, NULL, 7, 0.1, 1.5, first, n, info, flips) == QLDPC_ESIZE);
            CHECK(qldpc_mc_frames_host(N + 1, N, pos, NULL, 7, 0.1, 0.0, first, n, info, flips) == QLDPC_ESIZE);
            CHECK(qldpc_mc_frames_host(0, N, pos, NULL, 7, 0.1, 0.0, first, n, info, flips) == QLDPC_ESIZE);
            CHECK(qldpc_mc_frames_host(K, 0, pos, NULL, 7, 0.1, 0.0, first, n, info, flips) == QLDPC_ESIZE);
            CHECK(qldpc_mc_frames_host(K, N, pos, NULL, 7, 0.1, 0.0, first, -1, info, flips) == QLDPC_EINVAL);
            CHECK(qldpc_mc_frames_host(K, N, pos, NULL, 7, 0.1, 0.0, first, n, NULL, NULL) == QLDPC_EINVAL);
            CHECK(!memcmp(info, part_i, 4 * (size_t)n * Wk));
            pos[K - 1] = N;                                                       /* outside [0, N) */
            CHECK(qldpc_mc_frames_host(K, N, pos, NULL, 7, 0.1, 0.0, first, n, NULL, flips) == QLDPC_EINVAL);
            pos[K - 1] = -1;
            CHECK(qldpc_mc_frames_host(K, N, pos, NULL, 7, 0.1, 0.0, first, n, NULL, flips) == QLDPC_EINVAL);
            if (K > 1) {
                pos[K - 1] = pos[0];                                              /* repeated */
                CHECK(qldpc_mc_frames_host(K, N, pos, NULL, 7, 0.1, 0.0, first, n, NULL, flips) == QLDPC_EINVAL);
            }
            cls[N - 1] = 3;
            CHECK(qldpc_mc_frames_host(K, N, NULL, cls, 7, 0.1, 0.0, first, n, NULL, flips) == QLDPC_EINVAL);
            free(pos); free(cls); free(info); free(flips); free(part_i); free(part_f);
            cases++;
        }
    printf("sanitizer pass ok: %d cases\n", cases);
    return 0;
}
