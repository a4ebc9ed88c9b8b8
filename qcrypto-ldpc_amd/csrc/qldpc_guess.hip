/*
 * qldpc_guess.hip -- the public calls of a guessing round (qldpc_guess_expand_dev, qldpc_guess_pick_dev): argument checks and the launches of the
 * kernels of qldpc_kernels_guess.h.  They take no decoder: device pointers and a stream, on the current device, as qldpc_privamp_dev does.
 */
#include <algorithm>

#include "qldpc_hip.h"
#include "qldpc_kernels_guess.h"

/* every size check of both calls */
static int guess_sizes(const char *who, int N, int g, int n_src)
{
    if (N < 1 || g < 0 || g > GS_MAX_BITS || n_src < 0) {
        qldpc_set_error("%s: N=%d (at least 1), guess bits=%d (0 .. %d), n_src=%d (not negative)", who, N, g, GS_MAX_BITS, n_src);
        return QLDPC_ESIZE;
    }
    if (((uint64_t)n_src << g) > GS_MAX_SLOTS) {
        qldpc_set_error("%s: %d sources of %d trials pass %u trial slots", who, n_src, 1 << g, GS_MAX_SLOTS);
        return QLDPC_ESIZE;
    }
    return QLDPC_OK;
}

extern "C" int qldpc_guess_expand_dev(int N, int g, int n_src, const uint32_t *d_weak, const uint32_t *d_hard, uint32_t *d_known_out, uint32_t *d_value_out,
                                      void *hip_stream)
{
    if (!d_weak || !d_hard || !d_known_out || !d_value_out) return QLDPC_EINVAL;
    const int rc = guess_sizes("guess_expand", N, g, n_src);
    if (rc) return rc;
    if (n_src == 0) return QLDPC_OK;
    const unsigned T = 1u << g, gy = std::min((T + GS_WAVES - 1u) / GS_WAVES, 64u);      /* up to 256 waves deal the trials of a source */
    hipLaunchKernelGGL(qk_guess_expand, dim3((unsigned)n_src, gy), dim3(GS_LANES), 0, (hipStream_t)hip_stream, d_weak, d_hard, d_known_out, d_value_out, (N + 31) / 32, g);
    LAUNCHCHK();
    return QLDPC_OK;
}

extern "C" int qldpc_guess_pick_dev(int N, int g, int n_src, const int *d_ok, const uint32_t *d_trial_hard, int *d_winner, int *d_n_ok, int *d_ambiguous,
                                    uint32_t *d_out_hard, void *hip_stream)
{
    if (!d_ok || !d_trial_hard || !d_winner || !d_n_ok || !d_ambiguous || !d_out_hard) return QLDPC_EINVAL;
    const int rc = guess_sizes("guess_pick", N, g, n_src);
    if (rc) return rc;
    if (n_src == 0) return QLDPC_OK;
    hipLaunchKernelGGL(qk_guess_pick, dim3((unsigned)n_src), dim3(GS_LANES), 0, (hipStream_t)hip_stream, d_ok, d_trial_hard, d_winner, d_n_ok, d_ambiguous, d_out_hard, N,
                       (N + 31) / 32, g);
    LAUNCHCHK();
    return QLDPC_OK;
}
