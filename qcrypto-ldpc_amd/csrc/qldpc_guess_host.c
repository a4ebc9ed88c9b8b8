/*
 * qldpc_guess_host.c -- the host mirrors of the guessing round that need no device: the known and value rows of one trial (the functions the lanes of
 * qk_guess_expand run) and the winner, the count and the ambiguity flag of one source frame (those of qk_guess_pick), both on qldpc_guess_core.h.
 */
#include "../../include/qldpc.h"
#include "qldpc_graph.h"
#include "qldpc_guess_core.h"

static int guess_sizes(const char *who, int N, int g)
{
    if (N >= 1 && g >= 0 && g <= GS_MAX_BITS) return QLDPC_OK;
    qldpc_set_error("%s: N=%d (at least 1), guess bits=%d (0 .. %d)", who, N, g, GS_MAX_BITS);
    return QLDPC_ESIZE;
}

int qldpc_guess_trial_host(int N, int g, int t, const uint32_t *weak, const uint32_t *hard, uint32_t *known_out, uint32_t *value_out)
{
    if (!weak || !hard || !known_out || !value_out) return QLDPC_EINVAL;
    const int rc = guess_sizes("guess_trial_host", N, g);
    if (rc) return rc;
    if (t < 0 || t >= (1 << g)) { qldpc_set_error("guess_trial_host: trial %d outside 0 .. %d", t, (1 << g) - 1); return QLDPC_ESIZE; }
    const int W = (N + 31) / 32;
    unsigned rank = 0;
    for (int w = 0; w < W; w++) {
        known_out[w] = weak[w];
        value_out[w] = gs_value_word(weak[w], hard[w], (uint32_t)t, rank);
        rank += gs_popc(weak[w]);
    }
    return QLDPC_OK;
}

int qldpc_guess_pick_host(int N, int g, const int *ok, const uint32_t *trial_hard, int *winner, int *n_ok, int *ambiguous)
{
    if (!ok || !trial_hard || !winner || !n_ok || !ambiguous) return QLDPC_EINVAL;
    const int rc = guess_sizes("guess_pick_host", N, g);
    if (rc) return rc;
    const int W = (N + 31) / 32, T = 1 << g;
    int best = -1, count = 0, amb = 0;
    for (int t = 0; t < T; t++) { best = gs_better(best, t, ok[t] != 0); count += ok[t] != 0; }
    for (int t = 0; t < T && best >= 0; t++) {
        if (!ok[t] || t == best) continue;
        for (int w = 0; w < W; w++) amb |= gs_differs(trial_hard[(size_t)t * W + w], trial_hard[(size_t)best * W + w], w, N);
    }
    *winner = best; *n_ok = count; *ambiguous = amb;
    return QLDPC_OK;
}
