/*
 * qldpc_kernels_weakest.h -- blind reconciliation on the FRAMES engine: the weakest-VN select over the frame-interleaved posterior rows
 * (qldpc_fetch_weakest_dev) and the known-bit loads (qldpc_load_known_dev).  The select is stated in qldpc_weakest_core.h; these lanes and the
 * host mirror call the same functions.
 *
 * qk_weakest: one workgroup per 64 consecutive frames of a group (blockIdx.x = which 64 of the FG frames of group blockIdx.y), lane = frame, so a
 * load of VN v is one coalesced 256-byte piece of row v: the rows are read in place, [G][N][FG] as the decoder keeps them, and nothing frame-major
 * is written but the result.  The WK_WAVES waves of the workgroup split the words of the row range into contiguous pieces.  Per 8-bit digit: the
 * histogram hist[256 bins][64 lanes] in LDS (64 KiB; a lane adds only to its own column, and the address of a lane's add falls into bank
 * lane % banks whatever the bin, so the adds of one instruction do not collide; waves meet in a column, hence ds_add), then wave 0 walks each
 * lane's column (wk_pick).  The last pass takes the keys below the threshold and the first `rem` equal to it in index order; only when some lane
 * takes a proper subset of its equal keys does a counting pass first give every wave the number of equal keys in the ranges before its own.
 * 4 + 1 (+ 1) passes over the rows of the group; a workgroup none of whose frames is taken returns at once.
 * Rows of frames that are not taken are not written: the caller clears the output first.
 */
#ifndef QLDPC_KERNELS_WEAKEST_H
#define QLDPC_KERNELS_WEAKEST_H

#include "qldpc_weakest_core.h"

#define WK_WAVES 16
#define WK_THREADS (64 * WK_WAVES)

/* post[G][N][FG] floats; cand[n_frames][Wn] or NULL; take[n_frames] or NULL; out[n_frames][Wn] */
static __global__ __launch_bounds__(WK_THREADS) void qk_weakest(const float *__restrict__ post, int N, int FG, int n_frames, const uint32_t *__restrict__ cand,
                                                                const int *__restrict__ take, uint32_t d, uint32_t *__restrict__ out, int Wn)
{
    __shared__ uint32_t hist[WK_BINS * 64];
    __shared__ uint32_t s_T[64], s_rem[64], s_eq[WK_WAVES][64];
    __shared__ int s_order;
    const int g = blockIdx.y, r0 = blockIdx.x * 64;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int f = g * FG + r0 + lane;
    const bool live = f < n_frames && (!take || take[f] != 0);
    if (!__syncthreads_or(live)) return;
    const uint32_t *row = reinterpret_cast<const uint32_t *>(post) + (size_t)g * N * FG + r0 + lane;      /* VN v of this lane's frame: row[v * FG] */
    const uint32_t *cand_row = (cand && live) ? cand + (size_t)f * Wn : nullptr;
    const int per = (Wn + WK_WAVES - 1) / WK_WAVES;
    const int w0 = wave * per, w1 = min(Wn, w0 + per);

    uint32_t T = 0, rem = 0;
    for (int p = 0; p < WK_DIGITS; p++) {
        for (int i = threadIdx.x; i < WK_BINS * 64; i += WK_THREADS) hist[i] = 0;
        if (threadIdx.x == 0) s_order = 0;
        __syncthreads();
        for (int w = w0; w < w1; w++) {
            const uint32_t c = live ? wk_cand_word(cand_row, w, N) : 0u;
            if (!__any(c != 0u)) continue;
            const int nb = min(32, N - w * 32);
            uint32_t key[32];
#pragma unroll
            for (int b = 0; b < 32; b++) key[b] = b < nb ? wk_key_of_bits(row[(size_t)(w * 32 + b) * FG]) : 0u;
#pragma unroll
            for (int b = 0; b < 32; b++)
                if (((c >> (31 - b)) & 1u) && wk_agrees(key[b], T, p)) atomicAdd(&hist[wk_digit(key[b], p) * 64 + lane], 1u);
        }
        __syncthreads();
        if (wave == 0) {
            if (p == 0) {
                uint32_t total = 0;
                for (int b = 0; b < WK_BINS; b++) total += hist[b * 64 + lane];
                rem = min(d, total);
            }
            uint32_t in_bin = 0;
            if (rem) T |= wk_pick(hist + lane, 64, &rem, &in_bin) << (24 - 8 * p);
            s_T[lane] = T; s_rem[lane] = rem;
            if (p == WK_DIGITS - 1 && rem < in_bin) s_order = 1;      /* a proper subset of the equal keys: index order decides */
        }
        __syncthreads();
        T = s_T[lane]; rem = s_rem[lane];
    }
    if (rem == 0) T = 0;
    uint32_t run = 0;
    if (s_order) {
        uint32_t eq = 0;
        for (int w = w0; w < w1; w++) {
            const uint32_t c = live ? wk_cand_word(cand_row, w, N) : 0u;
            if (!__any(c != 0u)) continue;
            const int nb = min(32, N - w * 32);
#pragma unroll
            for (int b = 0; b < 32; b++)
                if (b < nb && ((c >> (31 - b)) & 1u) && wk_key_of_bits(row[(size_t)(w * 32 + b) * FG]) == T) eq++;
        }
        s_eq[wave][lane] = eq;
        __syncthreads();
        for (int k = 0; k < wave; k++) run += s_eq[k][lane];
    } else if (rem) {
        rem = 0xffffffffu;      /* every key equal to T is taken: no order needed */
    }
    for (int w = w0; w < w1; w++) {
        const uint32_t c = live ? wk_cand_word(cand_row, w, N) : 0u;
        uint32_t o = 0;
        if (__any(c != 0u)) {
            const int nb = min(32, N - w * 32);
            uint32_t key[32];
#pragma unroll
            for (int b = 0; b < 32; b++) key[b] = b < nb ? wk_key_of_bits(row[(size_t)(w * 32 + b) * FG]) : 0u;
#pragma unroll
            for (int b = 0; b < 32; b++)
                if (((c >> (31 - b)) & 1u) && wk_taken(key[b], T, rem, &run)) o |= 0x80000000u >> b;
        }
        if (live) out[(size_t)f * Wn + w] = o;
    }
}

/*
 * Known bits for decoders that read an LLR array (the mirror of qk_erase_rows): known[n_frames][W] / value[n_frames][W] packed MSB-first, a set
 * known bit makes that VN's channel LLR of that frame `pos` (value bit 0) or `neg` (value bit 1).  T = float ([G][N][FG]) or uint8_t (the 8-bit form).
 */
template <int V, typename T>
__global__ __launch_bounds__(QK_THREADS) void qk_known_rows(const uint32_t *__restrict__ known, const uint32_t *__restrict__ value, T *__restrict__ llr, int N, int W, int n_frames, T pos, T neg)
{
    constexpr int FG = 64 * V;
    const int g = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (int w = blockIdx.x * QK_WAVES + wave; w < W; w += gridDim.x * QK_WAVES) {
        uint32_t word[V], val[V];
        bool any = false;
#pragma unroll
        for (int j = 0; j < V; j++) {
            const int f = g * FG + lane * V + j;
            word[j] = f < n_frames ? known[(size_t)f * W + w] : 0u;
            val[j] = f < n_frames ? value[(size_t)f * W + w] : 0u;
            any = any || word[j] != 0u;
        }
        if (!__any(any)) continue;
        for (int b = 0; b < 32; b++) {
            const int v = w * 32 + b;
            if (v >= N) break;
#pragma unroll
            for (int j = 0; j < V; j++)
                if ((word[j] >> (31 - b)) & 1u) llr[((size_t)g * N + v) * FG + lane * V + j] = ((val[j] >> (31 - b)) & 1u) ? neg : pos;
        }
    }
}

/* the coded channel LLRs (qk_coded_llr) written out as the LLR array they stand for: a frame set that gets known bits runs on explicit LLRs */
template <int V>
__global__ __launch_bounds__(QK_THREADS) void qk_decode_llr(qk_coded_llr coded, float *__restrict__ llr, int N)
{
    constexpr int FG = 64 * V;
    const int g = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float mg[V];
    int nc[V];
#pragma unroll
    for (int j = 0; j < V; j++) { mg[j] = coded.fmag[(size_t)g * FG + lane * V + j]; nc[j] = coded.fnch[(size_t)g * FG + lane * V + j]; }
    for (int v = blockIdx.x * QK_WAVES + wave; v < N; v += gridDim.x * QK_WAVES) {
        float y[V];
        qk_coded_y<V>(y, coded, g, v, N, lane, mg, nc);
        qk_store<V>(llr + ((size_t)g * N + v) * FG + lane * V, y);
    }
}

#endif /* QLDPC_KERNELS_WEAKEST_H */
