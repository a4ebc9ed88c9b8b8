/*
 * qldpc_kernels_qber.h -- the kernels of the syndrome-weight QBER estimate (qldpc_qber_estimate_dev), on the functions of qldpc_qber_core.h.
 *
 *   qk_qber_class_rows  once per call: the class map as two packed rows (pinned, punctured), so that a frame's state is word logic
 *   qk_qber_count       grid = check chunks x frames, a thread per check.  A workgroup first collapses the frame's packed inputs into value / noisy /
 *                       erased rows in LDS, coalesced over words (STAGED), or -- rows too long for the LDS -- resolves the same word function at every
 *                       gather from memory, where a frame's rows are L2-resident.  A thread walks its check through the transposed check table
 *                       tab[j][c] (-1 past the check's degree), a wavefront folds its checks by effective degree with ballots, one LDS atomic per
 *                       degree present, and the workgroup's histogram [D + 1][2] leaves in one no-return atomic per non-zero bin to the frame's row
 *                       and to the pool's.
 *   qk_qber_count_merged  the same with runs of checks across erased chain VNs merged into one observation each (qldpc_qber_set_merge): the passes find
 *                       the heads of the runs and queue them, a thread per queued head gathers its run
 *   qk_qber_argmax      a workgroup per frame, one more for the pool: threads stride over the grid, int64 scores, the reduction keeps the larger
 *                       score and among equals the lower index.
 */
#ifndef QLDPC_KERNELS_QBER_H
#define QLDPC_KERNELS_QBER_H

#include <hip/hip_runtime.h>

#include "qldpc_qber_core.h"

#define QBK_THREADS 256
#define QBK_AHEAD 4            /* slots of a check's row the merged count loads at a time */

struct qbk_frame_rows {
    const uint32_t *bits;      /* [n_frames][Wn] */
    const uint32_t *erase;     /* [n_frames][Wn] or NULL */
    const uint32_t *known;     /* [n_frames][Wn] or NULL */
    const uint32_t *value;     /* [n_frames][Wn], read where known is given */
    const uint32_t *synd;      /* [n_frames][Wm] or NULL */
    const int *n_channel;      /* [n_frames] or NULL = N */
    const uint32_t *cls_rows;  /* [2][Wn] pinned | punctured, or NULL = all channel */
};

static __global__ __launch_bounds__(QBK_THREADS) void qk_qber_class_rows(const uint8_t *__restrict__ vn_class, uint32_t *__restrict__ cls_rows, int N, int Wn)
{
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= Wn) return;
    uint32_t pi, pu;
    qb_class_word(vn_class, w, N, &pi, &pu);
    cls_rows[w] = pi;
    cls_rows[(size_t)Wn + w] = pu;
}

/* the collapsed words of word w of frame f */
__device__ static inline void qbk_word(const qbk_frame_rows &in, size_t row, int w, int Wn, int nch, uint32_t *val, uint32_t *noisy, uint32_t *erased)
{
    const uint32_t kn = in.known ? in.known[row + w] : 0u;
    qb_collapse_word(in.bits[row + w], in.erase ? in.erase[row + w] : 0u, kn, kn ? in.value[row + w] : 0u, in.cls_rows ? in.cls_rows[w] : 0u,
                     in.cls_rows ? in.cls_rows[(size_t)Wn + w] : 0u, qb_below_word(w, nch), val, noisy, erased);
}

/* the wavefront's observations (inf: this lane has one, of effective degree d and outcome u) into the workgroup's histogram, one degree at a time */
__device__ __forceinline__ static void qbk_fold(bool inf, int d, uint32_t u, int lane, uint32_t *hist)
{
    unsigned long long todo = __ballot(inf);
    while (todo) {
        const int lead = __ffsll(todo) - 1;
        const int dl = __shfl(d, lead);
        const unsigned long long same = __ballot(inf && d == dl), odd = __ballot(inf && d == dl && u);
        if (lane == lead) {
            atomicAdd(&hist[2 * dl], (uint32_t)__popcll(same));
            if (odd) atomicAdd(&hist[2 * dl + 1], (uint32_t)__popcll(odd));
        }
        todo &= ~same;
    }
}

/* the workgroup's histogram to the frame's row and to the pool's, one no-return atomic per non-zero bin */
__device__ __forceinline__ static void qbk_flush(const uint32_t *hist, int bins, int tid, int f, uint32_t *__restrict__ counts, unsigned long long *__restrict__ pool)
{
    for (int i = tid; i < bins; i += QBK_THREADS) {
        const uint32_t h = hist[i];
        if (!h) continue;
        if (counts) atomicAdd(&counts[(size_t)f * bins + i], h);
        if (pool) atomicAdd(&pool[i], (unsigned long long)h);
    }
}

template <bool STAGED>
__global__ __launch_bounds__(QBK_THREADS) void qk_qber_count(qbk_frame_rows in, const int *__restrict__ tab, int N, int M, int D, int Wn, int Wm, int cpb,
                                                            uint32_t *__restrict__ counts, unsigned long long *__restrict__ pool)
{
    extern __shared__ uint32_t s_qb[];      /* histogram [D + 1][2], then (STAGED) rows [3][Wn] */
    const int bins = 2 * (D + 1), tid = threadIdx.x, lane = tid & 63;
    const int f = blockIdx.y;
    const size_t row = (size_t)f * Wn;
    uint32_t *hist = s_qb, *s_val = s_qb + bins, *s_noisy = s_val + Wn, *s_erased = s_noisy + Wn;
    const int nch = in.n_channel ? in.n_channel[f] : N;
    for (int i = tid; i < bins; i += QBK_THREADS) hist[i] = 0;
    if (STAGED)
        for (int w = tid; w < Wn; w += QBK_THREADS) qbk_word(in, row, w, Wn, nch, &s_val[w], &s_noisy[w], &s_erased[w]);
    __syncthreads();
    const int c0 = blockIdx.x * cpb, c1 = min(M, c0 + cpb);
    for (int base = c0; base < c1; base += QBK_THREADS) {
        const int c = base + tid;
        uint32_t u = 0, er = 0;
        int d = 0;
        if (c < c1) {
            if (in.synd) u = qb_bit(in.synd + (size_t)f * Wm, c);
            for (int j = 0; j < D; j++) {
                const int v = tab[(size_t)j * M + c];
                if (v < 0) break;
                const int w = v >> 5, sh = 31 - (v & 31);
                uint32_t a, b, e;
                if (STAGED) { a = s_val[w]; b = s_noisy[w]; e = s_erased[w]; }
                else qbk_word(in, row, w, Wn, nch, &a, &b, &e);
                u ^= (a >> sh) & 1u;
                d += (int)((b >> sh) & 1u);
                er |= (e >> sh) & 1u;
            }
        }
        qbk_fold(c < c1 && !er, d, u, lane, hist);
    }
    __syncthreads();
    qbk_flush(hist, bins, tid, f, counts, pool);
}

/*
 * The merged count (qldpc_qber_core.h, MERGING).  A pass of 256 threads looks at 256 checks, a thread per check, and only finds the heads: one or two
 * erased words, no gather.  The heads go to a queue in LDS; whenever it holds 256 of them a thread per head walks the link bits after it and gathers the
 * checks of its run, which may reach past the chunk's last check (the staged rows hold the whole frame).  So the lanes that gather are dense however
 * many checks are no heads -- with half of the parity erased a thread per check would leave every other lane idle through a walk twice as long.  A VN
 * met before in the run is one byte of the repeat table per edge.  The histogram has QB_MAX_DEGREE + 1 rows whatever D.
 */
template <bool STAGED>
__global__ __launch_bounds__(QBK_THREADS) void qk_qber_count_merged(qbk_frame_rows in, const int *__restrict__ tab, const uint8_t *__restrict__ rep, int N, int M, int D,
                                                                   int Wn, int Wm, int cpb, uint32_t *__restrict__ counts, unsigned long long *__restrict__ pool)
{
    extern __shared__ uint32_t s_qb[];      /* histogram [QB_MAX_DEGREE + 1][2], then (STAGED) rows [3][Wn] */
    __shared__ int s_q[2 * QBK_THREADS];    /* the queue of heads: fewer than 256 left over plus at most 256 of a pass */
    __shared__ int s_wn[QBK_THREADS / 64];  /* heads per wavefront of a pass */
    const int bins = 2 * (QB_MAX_DEGREE + 1), tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int f = blockIdx.y, K = N - M;
    const size_t row = (size_t)f * Wn;
    uint32_t *hist = s_qb, *s_val = s_qb + bins, *s_noisy = s_val + Wn, *s_erased = s_noisy + Wn;
    const int nch = in.n_channel ? in.n_channel[f] : N;
    for (int i = tid; i < bins; i += QBK_THREADS) hist[i] = 0;
    if (STAGED)
        for (int w = tid; w < Wn; w += QBK_THREADS) qbk_word(in, row, w, Wn, nch, &s_val[w], &s_noisy[w], &s_erased[w]);
    __syncthreads();
    auto erased_word = [&](int w) -> uint32_t {
        if (w >= Wn) return 0u;
        if (STAGED) return s_erased[w];
        uint32_t a, b, e;
        qbk_word(in, row, w, Wn, nch, &a, &b, &e);
        return e;
    };
    /* the run of head h into the histogram; every lane of the workgroup calls it, on = this lane has a head */
    auto count_run = [&](int h, bool on) {
        uint32_t u = 0, er = 0;
        int d = 0;
        bool counted = false;
        if (on) {
            const int w0 = (K + h) >> 5;
            const int len = qb_run_checks(erased_word(w0), erased_word(w0 + 1), K, h, M), t = h + len - 1;
            counted = len <= QB_MAX_RUN;
            for (int c = h; counted && c <= t; c++) {
                if (in.synd) u ^= qb_bit(in.synd + (size_t)f * Wm, c);
                /* QBK_AHEAD slots of the row and their repeat bytes are loaded before the first of them is looked at: the walk waits for memory once
                 * per group, not twice per edge (a slot's VN decides whether the next one is read at all) */
                bool more = true;
                for (int j0 = 0; more && j0 < D; j0 += QBK_AHEAD) {
                    int vs[QBK_AHEAD];
                    uint8_t rs[QBK_AHEAD];
#pragma unroll
                    for (int i = 0; i < QBK_AHEAD; i++) {
                        const size_t at = (size_t)min(j0 + i, D - 1) * M + c;
                        vs[i] = j0 + i < D ? tab[at] : -1;
                        rs[i] = rep[at];
                    }
#pragma unroll
                    for (int i = 0; i < QBK_AHEAD; i++) {
                        const int v = vs[i];
                        if (v < 0) { more = false; break; }
                        if (qb_is_link(v, K, h, t)) continue;
                        const int w = v >> 5, sh = 31 - (v & 31);
                        uint32_t a, b, e;
                        if (STAGED) { a = s_val[w]; b = s_noisy[w]; e = s_erased[w]; }
                        else qbk_word(in, row, w, Wn, nch, &a, &b, &e);
                        u ^= (a >> sh) & 1u;
                        er |= (e >> sh) & 1u;
                        if ((b >> sh) & 1u) d += (qb_earlier_in_run(tab, rep, M, D, rs[i], c, v, h) & 1) ? -1 : 1;
                    }
                }
            }
        }
        qbk_fold(counted && !er && d <= QB_MAX_DEGREE, d, u, lane, hist);
    };
    const int c0 = blockIdx.x * cpb, c1 = min(M, c0 + cpb);
    int qn = 0;      /* heads in the queue, the same in every thread */
    for (int base = c0; base < c1; base += QBK_THREADS) {
        const int c = base + tid;
        bool head = false;
        if (c < c1 && c > 0) {      /* VN K + c - 1 no link */
            const int v = K + c - 1;
            head = !((erased_word(v >> 5) >> (31 - (v & 31))) & 1u);
        }
        else head = c < c1;
        const unsigned long long heads = __ballot(head);
        if (lane == 0) s_wn[wave] = __popcll(heads);
        __syncthreads();
        int at = qn;
        for (int w = 0; w < QBK_THREADS / 64; w++) {
            const int n = s_wn[w];
            if (w < wave) at += n;
            qn += n;
        }
        if (head) s_q[at + __popcll(heads & ((1ull << lane) - 1ull))] = c;
        __syncthreads();
        if (qn >= QBK_THREADS) {
            count_run(s_q[tid], true);
            const int rest = qn - QBK_THREADS, keep = tid < rest ? s_q[QBK_THREADS + tid] : 0;
            __syncthreads();
            if (tid < rest) s_q[tid] = keep;
            qn = rest;
        }
    }
    __syncthreads();
    count_run(tid < qn ? s_q[tid] : 0, tid < qn);
    __syncthreads();
    qbk_flush(hist, bins, tid, f, counts, pool);
}

/* block f < n_frames: the frame's counts; block n_frames (launched only when the pool is wanted): the pool's */
static __global__ __launch_bounds__(QBK_THREADS) void qk_qber_argmax(const uint32_t *__restrict__ counts, const unsigned long long *__restrict__ pool, int D, int n_grid,
                                                              const int32_t *__restrict__ L1, const int32_t *__restrict__ L0, const float *__restrict__ qgrid,
                                                              const float *__restrict__ llrgrid, int n_frames, int *__restrict__ index, float *__restrict__ qber,
                                                              float *__restrict__ llr_mag, int *__restrict__ pool_index)
{
    __shared__ uint64_t s_cnt[2 * (QB_MAX_DEGREE + 1)];
    __shared__ long long s_S[QBK_THREADS];
    __shared__ int s_k[QBK_THREADS];
    const int f = blockIdx.x, tid = threadIdx.x, bins = 2 * (D + 1);
    const bool is_pool = f == n_frames;
    for (int i = tid; i < bins; i += QBK_THREADS) s_cnt[i] = is_pool ? (uint64_t)pool[i] : (uint64_t)counts[(size_t)f * bins + i];
    __syncthreads();
    int64_t best_S = 0;
    int best_k = -1;
    if (qb_observations(s_cnt, D))
        for (int k = tid; k < n_grid; k += QBK_THREADS) {
            const int64_t S = qb_score(s_cnt, D, L1, L0, n_grid, k);
            if (qb_better(S, k, best_S, best_k)) { best_S = S; best_k = k; }
        }
    s_S[tid] = best_S; s_k[tid] = best_k;
    __syncthreads();
    for (int half = QBK_THREADS / 2; half > 0; half >>= 1) {
        if (tid < half && s_k[tid + half] >= 0 && qb_better(s_S[tid + half], s_k[tid + half], s_S[tid], s_k[tid])) { s_S[tid] = s_S[tid + half]; s_k[tid] = s_k[tid + half]; }
        __syncthreads();
    }
    if (tid) return;
    const int k = s_k[0];
    if (is_pool) { if (pool_index) *pool_index = k; return; }
    if (index) index[f] = k;
    if (qber) qber[f] = k < 0 ? 0.0f : qgrid[k];
    if (llr_mag) llr_mag[f] = k < 0 ? 0.0f : llrgrid[k];
}

#endif /* QLDPC_KERNELS_QBER_H */
