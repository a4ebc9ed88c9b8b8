/*
 * qldpc_kernels_giveup.h -- the early-exit run that also gives up on frames whose syndrome weight has stopped falling (cfg.giveup_patience > 0;
 * the rule is stated in qldpc_giveup_core.h).  With the option off none of these kernels is launched.
 *
 *   qk_syndrome_count   qk_syndrome with a count: besides the OR of the unsatisfied checks per frame it adds, per frame slot, their NUMBER into
 *                       weight[G][FG].  Same inputs and placement (one XCD per group from 8 groups on, round robin below).  Every check is counted,
 *                       so the pass is one launch: the gated second launch of qk_syndrome may skip checks once every verdict is known.
 *   qk_status_count     qk_status that reads the weights, runs the rule, keeps {last, best, since} per frame and a `gave` mask per (group, j), sets
 *                       done bits and iteration counts for frames given up as for converged ones, and clears the weights for the next pass.
 *   qk_status_init_count / qk_giveup_out    reset at the start of every run / results in the caller's frame order, generation by generation.
 *
 * The count is a vertical popcount: a lane holds one 64-bit word per check, bit = frame lane, and wanted are the 64 column sums.  A wave transposes
 * the 64 x 64 bit matrix of 64 consecutive checks across its lanes (qldpc_wave_transpose.h: six butterfly stages, exchange with lane ^ d, keep one half, shift the other in),
 * after which lane f holds the bits of frame lane f and ONE popcount gives its sum over those 64 checks.  That is 6 lane exchanges of a 64-bit word
 * and ~6 bit operations each per 64 checks and j; 64 ballots of bit f with a scalar count each, the alternative, cost ~4 instructions per frame lane,
 * about four times as many.  The waves of a workgroup add their sums in LDS (ds_add), then one no-return atomicAdd per frame slot and workgroup goes
 * to memory.  It is device (agent) scope, HIP's default: with fewer than 8 groups the workgroups of a group sit on several XCDs, as for unsat's
 * atomicOr; the status pass reads the sums in the next launch.
 */
#ifndef QLDPC_KERNELS_GIVEUP_H
#define QLDPC_KERNELS_GIVEUP_H

#include "qldpc_kernels.h"
#include "qldpc_giveup_core.h"
#include "qldpc_wave_transpose.h"

/* the give-up state of one generation as the kernels take it: weight [G][FG] (shared by all generations: cleared after every test), the per-frame
 * arrays [G][FG], the mask of frames given up [G][V], the frames given up since the decoder was created (qldpc_giveup_total).  best == NULL: the
 * option is off */
struct qk_giveup { int *weight, *last, *best, *since; u64 *gave; unsigned long long *total; int patience; };

template <int V>
__global__ __launch_bounds__(256) void qk_syndrome_count(const u64 *__restrict__ mask, const int *__restrict__ cn_var_t, int max_dc, int M, int N,
                                                         u64 *__restrict__ unsat, const u64 *__restrict__ done, const u64 *__restrict__ synd, int G, int bx,
                                                         int *__restrict__ weight)
{
    constexpr int FG = 64 * V;
    __shared__ int wsum[FG];
    const int id = blockIdx.x;
    const int g = G < 8 ? id % G : (id & 7) + 8 * ((id >> 3) / bx);      /* qk_syndrome says why */
    const int chunk = G < 8 ? id / G : (id >> 3) % bx;
    if (g >= G) return;
    if (qk_group_done<V>(done, g)) return;      /* both returns take the whole workgroup */
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (threadIdx.x < FG) wsum[threadIdx.x] = 0;
    __syncthreads();
    const u64 *mg = mask + (size_t)g * N * V;
    u64 acc[V];
    int cnt[V];
#pragma unroll
    for (int j = 0; j < V; j++) { acc[j] = 0; cnt[j] = 0; }
    /* 64 consecutive checks per wave and trip; past M a lane brings an all-zero word, the trip count is the wave's */
    for (int c0 = (chunk * 4 + wave) * 64; c0 < M; c0 += bx * 256) {
        const int c = c0 + lane;
        const bool live = c < M;
        u64 s[V];
#pragma unroll
        for (int j = 0; j < V; j++) s[j] = (live && synd) ? synd[((size_t)g * M + c) * V + j] : 0ull;
        constexpr int B = 10;
        for (int t0 = 0; t0 < max_dc; t0 += B) {
            int v[B];
#pragma unroll
            for (int t = 0; t < B; t++) v[t] = (live && t0 + t < max_dc) ? cn_var_t[(size_t)(t0 + t) * M + c] : -1;
#pragma unroll
            for (int t = 0; t < B; t++)
                if (v[t] >= 0) {
                    const u64 *p = mg + (size_t)v[t] * V;
#pragma unroll
                    for (int j = 0; j < V; j++) s[j] ^= p[j];
                }
        }
#pragma unroll
        for (int j = 0; j < V; j++) { acc[j] |= s[j]; cnt[j] += __popcll(qk_transpose64(s[j], lane)); }
    }
#pragma unroll
    for (int j = 0; j < V; j++) {
        u64 a = acc[j];
        for (int o = 32; o > 0; o >>= 1) a |= __shfl_xor(a, o);
        if (lane == 0 && a) atomicOr(&unsat[(size_t)g * V + j], a);
        if (cnt[j]) atomicAdd(&wsum[lane * V + j], cnt[j]);      /* slot of the group = lane * V + j */
    }
    __syncthreads();
    if (threadIdx.x < FG) {
        const int w = wsum[threadIdx.x];
        if (w) atomicAdd(&weight[(size_t)g * FG + threadIdx.x], w);
    }
}

template <int V>
__global__ void qk_status_count(u64 *__restrict__ unsat, u64 *__restrict__ done, int *__restrict__ depth, int *__restrict__ iters,
                                int G, int syndrome_depth, int ite_done, int *__restrict__ active_groups,
                                unsigned long long *__restrict__ work, volatile int *__restrict__ host_report, int seq, qk_giveup gu)
{
    constexpr int FG = 64 * V;
    const int g = blockIdx.x;
    const int lane = threadIdx.x;   /* 64 threads */
    bool all = true, was_all = true;
    int left = 0;
#pragma unroll
    for (int j = 0; j < V; j++) {
        const u64 u = unsat[(size_t)g * V + j];
        const u64 d = done[(size_t)g * V + j];
        was_all = was_all && (d == ~0ull);
        const int f = g * FG + lane * V + j;
        const bool was_done = (d >> lane) & 1ull;
        const bool zero = !((u >> lane) & 1ull);
        const int w = gu.weight[f];
        gu.weight[f] = 0;
        bool now = false, gave = false;
        if (!was_done) {
            int cur = depth[f], best = gu.best[f], since = gu.since[f];
            now = gu_converges(&cur, zero, syndrome_depth);
            gu_observe(&best, &since, w);
            gave = gu_gives_up(w, since, gu.patience, now);
            depth[f] = cur; gu.best[f] = best; gu.since[f] = since; gu.last[f] = w;
            if (now || gave) iters[f] = ite_done;
        }
        const u64 gm = __ballot(gave);
        const u64 nd = d | __ballot(now) | gm;
        all = all && (nd == ~0ull);
        left += __popcll(~nd);
        if (lane == 0) {
            done[(size_t)g * V + j] = nd; unsat[(size_t)g * V + j] = 0;
            if (gm) { gu.gave[(size_t)g * V + j] |= gm; atomicAdd(gu.total, (unsigned long long)__popcll(gm)); }
        }
    }
    if (lane == 0) qk_status_report(all, was_all, left, G, active_groups, work, host_report, seq);
}

template <int V>
__global__ void qk_status_init_count(u64 *__restrict__ unsat, u64 *__restrict__ done, int *__restrict__ depth, int *__restrict__ iters,
                                     int n_frames, int n_ite, unsigned long long *__restrict__ work, int *__restrict__ active_groups, qk_giveup gu)
{
    qk_status_init_body<V>(unsat, done, depth, iters, n_frames, n_ite, work, active_groups);
    constexpr int FG = 64 * V;
    const int g = blockIdx.x, lane = threadIdx.x;
#pragma unroll
    for (int j = 0; j < V; j++) {
        const int f = g * FG + lane * V + j;
        gu.weight[f] = 0; gu.last[f] = 0;
        gu_reset(&gu.best[f], &gu.since[f]);
        if (lane == 0) gu.gave[(size_t)g * V + j] = 0;
    }
}

/* gave / last weight / best weight of the frames whose result this generation holds, in the caller's order (qk_result_frame) */
template <int V>
__global__ void qk_giveup_out(qk_giveup gu, int *__restrict__ out_gave, int *__restrict__ out_last, int *__restrict__ out_best, int n_slots,
                              const int *__restrict__ origin, const u64 *__restrict__ final_mask)
{
    constexpr int FG = 64 * V;
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    const int o = qk_result_frame<V>(f, n_slots, origin, final_mask);
    if (o < 0) return;
    const int g = f / FG, r = f % FG, lane = r / V, j = r % V;
    if (out_gave) out_gave[o] = (int)((gu.gave[(size_t)g * V + j] >> lane) & 1ull);
    if (out_last) out_last[o] = gu.last[f];
    if (out_best) out_best[o] = gu.best[f];
}

#endif /* QLDPC_KERNELS_GIVEUP_H */
