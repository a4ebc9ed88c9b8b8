/* Sanitizer pass over the host side of blind reconciliation (qldpc_blind_host.c over qldpc_weakest_core.h, no HIP): the select on rows and masks
 * allocated at their exact sizes, against an insertion sort over (key, v); Alice's answer against a bit loop.  Built with
 * -fsanitize=address,undefined by tests/test_blind.py */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../qcrypto-ldpc_amd/csrc/qldpc_blind_host.c"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #x); return 1; } } while (0)

static uint64_t rng_state = 0x243f6a8885a308d3ull;
static uint32_t rng32(void)
{
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return (uint32_t)((z ^ (z >> 31)) >> 16);
}

static int one_case(int N, int d, int style, int masked)
{
    const int W = (N + 31) / 32;
    float *post = malloc(sizeof(float) * (size_t)N);
    uint32_t *cand = malloc(4 * (size_t)W), *got = malloc(4 * (size_t)W), *want = calloc((size_t)W, 4);
    int *idx = malloc(sizeof(int) * (size_t)N);
    static const float mags[3] = {0.75f, 1.5f, 23.03f};
    for (int v = 0; v < N; v++) {
        const uint32_t r = rng32();
        const float m = style == 0 ? (float)(r & 0xffffu) / 97.0f : (style == 1 ? mags[r % 3u] : ((r & 3u) ? 0.0f : 2.5f));
        post[v] = (r & 0x10000u) ? -m : m;
    }
    for (int w = 0; w < W; w++) cand[w] = masked == 2 ? 0u : (rng32() | (rng32() << 16));      /* tail bits past N set at random on purpose */
    /* the reference: the candidates in (key, v) order by insertion */
    int n = 0;
    for (int v = 0; v < N; v++) {
        if (masked && !((cand[v >> 5] >> (31 - (v & 31))) & 1u)) continue;
        uint32_t kv;
        memcpy(&kv, &post[v], 4);
        kv &= 0x7fffffffu;
        int at = n++;
        while (at > 0) {
            uint32_t ku;
            memcpy(&ku, &post[idx[at - 1]], 4);
            if ((ku & 0x7fffffffu) <= kv) break;
            idx[at] = idx[at - 1]; at--;
        }
        idx[at] = v;
    }
    const int t = d < n ? d : n;
    for (int i = 0; i < t; i++) want[idx[i] >> 5] |= 0x80000000u >> (idx[i] & 31);
    int taken = -1;
    CHECK(qldpc_weakest_host(post, N, masked ? cand : NULL, d, got, &taken) == QLDPC_OK);
    CHECK(taken == t && memcmp(got, want, 4 * (size_t)W) == 0);
    free(post); free(cand); free(got); free(want); free(idx);
    return 0;
}

int main(void)
{
    static const int sizes[] = {1, 31, 32, 33, 1008, 2500};
    for (unsigned s = 0; s < sizeof sizes / sizeof sizes[0]; s++) {
        const int N = sizes[s], ds[] = {0, 1, N / 2, N, N + 5};
        for (int style = 0; style < 3; style++)
            for (int masked = 0; masked < 3; masked++)
                for (unsigned k = 0; k < 5; k++)
                    if (one_case(N, ds[k], style, masked)) return 1;
    }
    float p1[1] = {1.0f};
    uint32_t o1[1];
    CHECK(qldpc_weakest_host(p1, 1, NULL, -1, o1, NULL) == QLDPC_EINVAL && qldpc_weakest_host(p1, 0, NULL, 1, o1, NULL) == QLDPC_EINVAL);
    /* Alice's answer */
    for (int kb = 1; kb <= 70; kb += 23) {
        const int Wk = (kb + 31) / 32;
        uint32_t *key = malloc(4 * (size_t)Wk);
        int *pos = malloc(sizeof(int) * (size_t)kb);
        uint8_t *bit = malloc((size_t)kb);
        for (int w = 0; w < Wk; w++) key[w] = rng32() | (rng32() << 16);
        for (int i = 0; i < kb; i++) pos[i] = kb - 1 - i;
        CHECK(qldpc_recon_disclose_host(key, kb, pos, kb, bit) == QLDPC_OK);
        for (int i = 0; i < kb; i++) CHECK(bit[i] == ((key[pos[i] >> 5] >> (31 - (pos[i] & 31))) & 1u));
        pos[0] = kb;
        CHECK(qldpc_recon_disclose_host(key, kb, pos, kb, bit) == QLDPC_EINVAL);
        CHECK(qldpc_recon_disclose_host(key, kb, NULL, 0, NULL) == QLDPC_OK);
        free(key); free(pos); free(bit);
    }
    printf("sanitizer pass ok\n");
    return 0;
}
