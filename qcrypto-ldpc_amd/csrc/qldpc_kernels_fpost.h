/*
 * qldpc_kernels_fpost.h -- the posterior form of a fixed-iteration flooding min-sum run (fp32, 64-frame groups, IRA codes).
 *
 * The flooding recursion (Decoder_LDPC_BP_flooding::_decode_single_ite / _initialize_var_to_chk) moves 4 E message rows per
 * iteration: var_to_chk written and read, chk_to_var written and read.  Three facts let a run move fewer rows and still compute
 * the very same floats:
 *
 *  1. var_to_chk[slot] = tmp - chk_to_var[slot] with tmp = Y + sum of the VN's messages in slot order.  The variable-node pass
 *     therefore only writes tmp (qk_vn_fpost below, one row per VN; qk_vn_flood in QK_VN_POST mode where the run closes, for degrees
 *     above QK_FPV_DMAX and with QLDPC_FLOOD_POST_VN=0); the check forms tmp - (its own previous message)
 *     itself: the same subtraction on the same operands.
 *  2. A check rebuilds its own previous messages from a compressed state, as the layered sweeps do (qldpc_kernels_cst.h).  For
 *     MS / OMS / NMS a tie min1 == min2 makes cst1 and cst2 the same float (qk_acc<QK_FAM_MS>::finish), so "which edges took
 *     cst1" shrinks to the index of ONE edge whose magnitude was min1: every other edge takes cst2, which on a tie is the same
 *     value.  Index (5 bits) and the dc sign bits share one word for dc <= 27: THREE 256-byte rows per check,
 *         {cst1, cst2, packed}[64]     packed: bit k = message of edge k is negative, bits 27..31 = the edge that took cst1.
 *     Nobody but the owner needs a check's state -- except:
 *  3. The accumulator chain of an IRA code: VN K + c sits on checks c and c + 1 only (VN K + M - 1 on check M - 1 only).  Its two
 *     messages belong to two adjacent checks, which adjacent wavefronts of one workgroup work on at the same time, so check c
 *     works out the totals of its two chain VNs from its own state and the states of checks c - 1 and c + 1 (cache hits, apart
 *     from the first and last wave of a workgroup).  The variable-node pass skips the chain VNs altogether: their posterior rows
 *     and their chk_to_var rows are never written or read.
 *
 * The state is read from one buffer and written to another (ping-pong by iteration parity): a neighbour may still be reading the
 * old one.  State loads are ordinary cached loads -- the neighbour's copy in the cache is the point.  The first iteration takes all
 * state as zero without reading it (every message +0.0), which gives (Y + 0) - 0 on every edge as qk_cn_flood<FIRST> does.
 *
 * After the last check pass qk_fpost_close gives the chain VNs their ballots (and posterior rows on request) from the final state.
 */
#ifndef QLDPC_KERNELS_FPOST_H
#define QLDPC_KERNELS_FPOST_H

#include "qldpc_kernels.h"

#define QK_FP_ROWS 3           /* {cst1, cst2, packed} */
#define QK_FP_DCMAX 27         /* sign bits 0..26, index in bits 27..31 */
#define QK_FP_NONE 0xffu       /* chain table: no such edge */
/* chain table, one word per check c (qldpc_code_chain_table): byte 0 = position of VN K + c - 1 in the row of check c, byte 1 = position of
 * VN K + c in it, byte 2 = position of VN K + c - 1 in the row of check c - 1, byte 3 = position of VN K + c in the row of check c + 1 */

/* the message of edge k for this lane's frame, rebuilt from a check's state: same magnitude bits, same sign bit (a -0.0 stays a -0.0) */
__device__ __forceinline__ float qk_fp_msg(uint32_t w, int k, float c1, float c2)
{
    return qk_withsign(((int)(w >> 27) == k) ? c1 : c2, (w >> k) << 31);
}

/*
 * The check pass.  One wavefront per check, indices prefetched with back-to-back scalar loads as in qk_cn_flood.
 *   info edge k:   x = post[v_k] - (own previous message k)
 *   chain edges:   tmp = Y + ((0.0f + m[slot 0]) + m[slot 1]) in the VN's slot order (ascending check: the lower check is slot 0),
 *                  exactly as qk_vn_flood sums; x = tmp - own.  The last VN has degree 1: tmp = Y + (0.0f + own).
 * then the fold of qk_acc<QK_FAM_MS>, the info edges' outputs CN-major as qk_cn_flood stores them, and the new state.
 *
 * Everything a wave reads is asked for before it waits for any of it.  The frame constants depend on g and lane only and go first.  The
 * first pass (coded) has no rows to gather, only channel words: lane k loads the VN index of edge k and then that VN's words by its own
 * address (qk_coded_fetch), two vector round trips for a check of any degree, and edge k's words reach every lane through readlane.  A
 * steady pass needs channel words for its two chain VNs only: their scalar loads are issued in front of the gathers and travel with them.
 * The posterior gathers and the state stores stay plain: non-temporal gathers, non-temporal state stores and both together were measured
 * and none stood clear of the run-to-run spread (DESIGN section 8 #1a); the gathers then fetch 1.08 x as many bytes.
 */
template <int DCMAX, bool FIRST, bool CODED>
__global__ __launch_bounds__(QK_THREADS) void qk_cn_fpost(const float *__restrict__ post, const float *__restrict__ llr, float *__restrict__ c2v,
                                                          const float *st_in, float *st_out,
                                                          const int *__restrict__ list, int n_list,
                                                          const int *__restrict__ cn_ptr, const int *__restrict__ cn_var, const uint32_t *__restrict__ chain,
                                                          size_t group_stride, const u64 *__restrict__ done, qk_rule rule, const u64 *__restrict__ synd, int M, int N,
                                                          qk_coded_llr coded)
{
    static_assert(DCMAX > 0 && DCMAX <= QK_FP_DCMAX, "sign bits and the index share one word");
    const int g = blockIdx.y;
    const int lane = threadIdx.x & 63;
    float mg = 0.0f;
    int nc = 0;
    if constexpr (CODED) { mg = coded.fmag[(size_t)g * 64 + lane]; nc = coded.fnch[(size_t)g * 64 + lane]; }
    if (qk_group_done<1>(done, g)) return;      /* a group of padding frames only */
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = blockIdx.x * QK_WAVES + wave;
    if (i >= n_list) return;
    const int c = list[i];
    const int b = cn_ptr[c];
    const int deg = cn_ptr[c + 1] - b;
    const uint32_t ch = chain[c];
    const int lpos = (int)(ch & 0xffu), rpos = (int)((ch >> 8) & 0xffu), lnb = (int)((ch >> 16) & 0xffu), rnb = (int)(ch >> 24);
    const float *pg = post + (size_t)g * N * 64 + lane;
    const float *yin = llr + (size_t)g * N * 64 + lane;
    const size_t srow = ((size_t)g * M + c) * (64 * QK_FP_ROWS) + lane;
    int vid[DCMAX];
    float x[DCMAX];
    float yl = 0.0f, yr = 0.0f;      /* Y of the chain VNs at positions lpos and rpos */
    /* own state, and the states of checks c - 1 and c + 1 where a chain VN is shared with them */
    float c1 = 0.0f, c2 = 0.0f, lc1 = 0.0f, lc2 = 0.0f, rc1 = 0.0f, rc2 = 0.0f;
    uint32_t w = 0u, lw = 0u, rw = 0u;
    if constexpr (FIRST) {      /* x[k] holds Y of edge k first */
        if constexpr (CODED) {
            /* lanes as edges: lane k holds the words of the VN of edge k (lanes past the degree repeat the last edge: no further cache line) */
            const int kl = lane < deg ? lane : (deg > 0 ? deg - 1 : 0);
            const int vlane = cn_var[b + kl];
            const qk_coded_w wl = qk_coded_fetch(coded, g, vlane, N);
#pragma unroll
            for (int k = 0; k < DCMAX; k++) {      /* no test of the degree: past it, the last edge again */
                vid[k] = __builtin_amdgcn_readlane(vlane, k);
                x[k] = qk_coded_y_of(qk_coded_w_of_lane(wl, k), vid[k], mg, nc);
            }
        } else {
#pragma unroll
            for (int k = 0; k < DCMAX; k++) vid[k] = cn_var[b + k];      /* padded by QK_IDX_PAD */
#pragma unroll
            for (int k = 0; k < DCMAX; k++)
                x[k] = (k < deg) ? yin[(size_t)vid[k] * 64] : 0.0f;      /* a row other checks gather too: cached */
        }
#pragma unroll
        for (int k = 0; k < DCMAX; k++) {
            yl = (k == lpos) ? x[k] : yl;
            yr = (k == rpos) ? x[k] : yr;
            x[k] = qk_first_v2c(x[k], (const float *)nullptr);
        }
    } else {
#pragma unroll
        for (int k = 0; k < DCMAX; k++) vid[k] = cn_var[b + k];      /* padded by QK_IDX_PAD */
        /* the two chain VNs (wave-uniform positions; a position DCMAX or beyond never matches; VN 0 stands in where there is none) */
        int vl = 0, vr = 0;
#pragma unroll
        for (int k = 0; k < DCMAX; k++) { vl = (k == lpos) ? vid[k] : vl; vr = (k == rpos) ? vid[k] : vr; }
        qk_coded_w wcl, wcr;
        if constexpr (CODED) { wcl = qk_coded_fetch(coded, g, vl, N); wcr = qk_coded_fetch(coded, g, vr, N); }
        else { yl = yin[(size_t)vl * 64]; yr = yin[(size_t)vr * 64]; }
#pragma unroll
        for (int k = 0; k < DCMAX; k++)
            if (k < deg && k != lpos && k != rpos) x[k] = pg[(size_t)vid[k] * 64];
        const float *s = st_in + srow;
        const uint32_t *sw = reinterpret_cast<const uint32_t *>(s);
        c1 = s[0]; c2 = s[64]; w = sw[128];
        if (lpos != (int)QK_FP_NONE && c > 0) { lc1 = s[-192]; lc2 = s[-128]; lw = sw[-64]; }         /* the rows of check c - 1 */
        if (rnb != (int)QK_FP_NONE && c + 1 < M) { rc1 = s[192]; rc2 = s[256]; rw = sw[320]; }        /* the rows of check c + 1 */
        if constexpr (CODED) { qk_coded_pin(wcl); qk_coded_pin(wcr); qk_pin_lane(mg, nc); yl = qk_coded_y_of(wcl, vl, mg, nc); yr = qk_coded_y_of(wcr, vr, mg, nc); }
#pragma unroll
        for (int k = 0; k < DCMAX; k++)
            if (k < deg && k != lpos && k != rpos) x[k] = x[k] - qk_fp_msg(w, k, c1, c2);
    }
    /* the chain edges: slot 0 is the lower check.  In the first pass every message is +0.0: (Y + 0) - 0 as on the other edges.  Both are worked out
     * whether the check has them or not (a position QK_FP_NONE matches no edge below, what it gives is dropped): under a branch of their own the
     * compiler moves the loads of yl and yr into that branch, behind the wait for the gathers */
    const int lp = lpos & 31, rp = rpos & 31;
    float xl, xr;
    {      /* VN K + c - 1: slot 0 = check c - 1, slot 1 = this check */
        const float own = qk_fp_msg(w, lp, c1, c2), nb = qk_fp_msg(lw, lnb & 31, lc1, lc2);
        const float tmp = yl + ((0.0f + nb) + own);
        xl = tmp - own;
    }
    {      /* VN K + c: slot 0 = this check, slot 1 = check c + 1 (none for the last VN) */
        const float own = qk_fp_msg(w, rp, c1, c2);
        const float sum0 = 0.0f + own;
        const float sum = (rnb != (int)QK_FP_NONE) ? sum0 + qk_fp_msg(rw, rnb & 31, rc1, rc2) : sum0;
        const float tmp = yr + sum;
        xr = tmp - own;
    }
    qk_acc<QK_FAM_MS> acc;
    acc.begin();
    if (synd) acc.sign = (uint32_t)((synd[(size_t)g * M + c] >> lane) & 1ull) << 31;
#pragma unroll
    for (int k = 0; k < DCMAX; k++)
        if (k < deg) {
            if (k == lpos) x[k] = xl;
            if (k == rpos) x[k] = xr;
            acc.in(x[k]);
        }
    acc.finish(rule);
    float *cout = c2v + (size_t)g * group_stride + lane;
    uint32_t nw = 0u, idx = 0u;
#pragma unroll
    for (int k = 0; k < DCMAX; k++)
        if (k < deg) {
            const float o = acc.out(x[k], rule);
            if (k != lpos && k != rpos) __builtin_nontemporal_store(o, cout + (size_t)(b + k) * 64);      /* CN-major, streamed: read once by the variable-node pass */
            nw |= (qk_bits(o) >> 31) << k;
        }
#pragma unroll
    for (int k = DCMAX - 1; k >= 0; k--)
        if (k < deg) idx = (fabsf(x[k]) == acc.min1) ? (uint32_t)k : idx;      /* descending k: the first edge at the minimum stays */
    float *so = st_out + srow;
    so[0] = acc.cst1; so[64] = acc.cst2; reinterpret_cast<uint32_t *>(so)[128] = nw | (idx << 27);
}

/*
 * The posterior pass between two iterations: tmp = Y + (((0.0f + m[0]) + m[1]) + ...) in slot order, exactly as qk_vn_flood sums, one
 * posterior row stored per information VN and nothing else (no ballots: nobody reads them before the run closes).
 *
 * The VNs come in classes of ONE degree each (fp_vn_class, qldpc_engine_int.h), and one launch covers up to QK_FPV_CLASSES of them: the
 * workgroups of class k are blk_end[k - 1] .. blk_end[k] - 1.  Class and degree are found by comparing blockIdx.x and one switch, all
 * wave-uniform, and each degree runs its own fully unrolled body without a per-row predicate.
 *
 * A wave learns everything in one scalar round trip: entry i of a class is one aligned record {v, row[0 .. D)} with
 * row[k] = vn_tr[vn_ptr[v] + k] (QK_FPV_STRIDE(D) ints: one dwordx4 for degree 3), asked for together with the group's `done` word.
 * Then the message rows (non-temporal: the check pass streamed them out, they are read once), the channel values behind them as in
 * qk_vn_flood, the sum, and a non-temporal store: the next check pass gathers a posterior row once per edge of its VN, but a pass of rows
 * later -- a plain store only parks the row in a cache it is evicted from before anybody asks (measured, DESIGN section 8 #1a).
 */
#define QK_FPV_DMAX 12         /* the degrees with a body (VN_CAPS of the engine: the register-resident buckets) */
#define QK_FPV_CLASSES 4       /* degree classes per launch */
#define QK_FPV_STRIDE(D) (((D) + 1 + 3) & ~3)      /* ints per record: {v, row[0 .. D)} padded to 16 bytes */
#define QK_FPV_UN(D) ((D) <= 4 ? 4 : 2)      /* VNs per wave: 12 rows in flight at degree 3, 22 at degree 11 */
struct qk_fpv_args {
    const int *rec[QK_FPV_CLASSES];
    int n[QK_FPV_CLASSES], deg[QK_FPV_CLASSES], blk_end[QK_FPV_CLASSES];      /* unused classes: n = 0, blk_end = the grid */
};
template <int D, int UN, bool CODED>
__device__ __forceinline__ void qk_vn_fpost_deg(const float *__restrict__ cin, const float *__restrict__ yin, float *__restrict__ pout,
                                                const int *__restrict__ rec, int n_list, int i0, int g, int lane, int N,
                                                const u64 *__restrict__ done, const qk_coded_llr &coded)
{
    constexpr int S = QK_FPV_STRIDE(D);
    if (i0 >= n_list) return;
    int w[UN][S];
#pragma unroll
    for (int u = 0; u < UN; u++) {
        const int i = (i0 + u < n_list) ? i0 + u : i0;      /* the tail repeats entry i0 (idempotent) */
        const int4 *r = reinterpret_cast<const int4 *>(rec) + (size_t)i * (S / 4);
#pragma unroll
        for (int q = 0; q < S / 4; q++) {
            const int4 t = r[q];
            w[u][4 * q] = t.x; w[u][4 * q + 1] = t.y; w[u][4 * q + 2] = t.z; w[u][4 * q + 3] = t.w;
        }
    }
    if (qk_group_done<1>(done, g)) return;      /* a group of padding frames only */
    float m[UN][D > 0 ? D : 1];
#pragma unroll
    for (int u = 0; u < UN; u++) {
#pragma unroll
        for (int k = 0; k < D; k++) m[u][k] = __builtin_nontemporal_load(cin + (size_t)w[u][1 + k] * 64);
    }
    float y[UN];
    if constexpr (CODED) {
        const float mg[1] = {coded.fmag[(size_t)g * 64 + lane]};
        const int nc[1] = {coded.fnch[(size_t)g * 64 + lane]};
#pragma unroll
        for (int u = 0; u < UN; u++) {
            float t[1];
            qk_coded_y<1>(t, coded, g, w[u][0], N, lane, mg, nc);
            y[u] = t[0];
        }
    } else {
#pragma unroll
        for (int u = 0; u < UN; u++) y[u] = __builtin_nontemporal_load(yin + (size_t)w[u][0] * 64);
    }
#pragma unroll
    for (int u = 0; u < UN; u++) {
        float sum = 0.0f;
#pragma unroll
        for (int k = 0; k < D; k++) sum += m[u][k];
        __builtin_nontemporal_store(y[u] + sum, pout + (size_t)w[u][0] * 64);
    }
}

template <bool CODED>
__global__ __launch_bounds__(QK_THREADS) void qk_vn_fpost(const float *__restrict__ c2v, const float *__restrict__ llr, float *__restrict__ post, qk_fpv_args a,
                                                          int N, size_t group_stride, const u64 *__restrict__ done, qk_coded_llr coded)
{
    const int g = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const float *cin = c2v + (size_t)g * group_stride + lane;
    const float *yin = llr + (size_t)g * N * 64 + lane;
    float *pout = post + (size_t)g * N * 64 + lane;
    const int blk = (int)blockIdx.x;
    const int *rec = a.rec[0];
    int n = a.n[0], deg = a.deg[0], blk0 = 0;
#pragma unroll
    for (int k = 1; k < QK_FPV_CLASSES; k++)
        if (blk >= a.blk_end[k - 1]) { rec = a.rec[k]; n = a.n[k]; deg = a.deg[k]; blk0 = a.blk_end[k - 1]; }
    const int wi = (blk - blk0) * QK_WAVES + wave;      /* this wave within its class */
#define QK_FPV_CASE(D) case D: qk_vn_fpost_deg<D, QK_FPV_UN(D), CODED>(cin, yin, pout, rec, n, wi * QK_FPV_UN(D), g, lane, N, done, coded); break;
    switch (deg) {
        QK_FPV_CASE(0) QK_FPV_CASE(1) QK_FPV_CASE(2) QK_FPV_CASE(3) QK_FPV_CASE(4) QK_FPV_CASE(5) QK_FPV_CASE(6)
        QK_FPV_CASE(7) QK_FPV_CASE(8) QK_FPV_CASE(9) QK_FPV_CASE(10) QK_FPV_CASE(11) QK_FPV_CASE(12)
    default: break;
    }
#undef QK_FPV_CASE
}

/*
 * _compute_post of the chain VNs after the last check pass: tmp from the final state of checks c and c + 1, the sgn / hard ballots
 * qk_vn_flood leaves (padding frames keep the bits they had) and, on request, the posterior row.  One wavefront per chain VN.
 * The state rows stay cached loads (the wave of check c - 1 reads the rows of check c too); the rows of check c + 1 are asked for
 * whenever it exists, not only once the chain word has said that it shares the VN, so that no row load waits for a scalar one.
 */
template <bool CODED>
__global__ __launch_bounds__(QK_THREADS) void qk_fpost_close(const float *__restrict__ st, const float *__restrict__ llr, const uint32_t *__restrict__ chain,
                                                             u64 *__restrict__ sgn, u64 *__restrict__ hard, float *__restrict__ post_out,
                                                             int M, int N, int K, const u64 *__restrict__ done, qk_coded_llr coded)
{
    const int g = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int c = blockIdx.x * QK_WAVES + wave;
    if (c >= M) return;
    const int v = K + c;
    /* the channel words, the two chain words and both checks' rows are asked for together: none of the addresses waits for another load */
    qk_coded_w wc;
    float y = 0.0f, mg = 0.0f;
    int nc = 0;
    if constexpr (CODED) { mg = coded.fmag[(size_t)g * 64 + lane]; nc = coded.fnch[(size_t)g * 64 + lane]; wc = qk_coded_fetch(coded, g, v, N); }
    else y = llr[((size_t)g * N + v) * 64 + lane];
    const bool more = c + 1 < M;      /* the last chain VN has degree 1 */
    const uint32_t ch0 = chain[c], ch1 = chain[more ? c + 1 : c];
    const float *s = st + ((size_t)g * M + c) * (64 * QK_FP_ROWS) + lane;
    const uint32_t *sw = reinterpret_cast<const uint32_t *>(s);
    const float c1 = s[0], c2 = s[64];
    const uint32_t w = sw[128];
    float n1 = 0.0f, n2 = 0.0f;
    uint32_t nw = 0u;
    if (more) { n1 = s[192]; n2 = s[256]; nw = sw[320]; }
    const int rpos = (int)((ch0 >> 8) & 0xffu);
    const int npos = more ? (int)(ch1 & 0xffu) : (int)QK_FP_NONE;
    float sum = 0.0f + qk_fp_msg(w, rpos, c1, c2);
    if (npos != (int)QK_FP_NONE) sum = sum + qk_fp_msg(nw, npos, n1, n2);
    if constexpr (CODED) y = qk_coded_y_of(wc, v, mg, nc);
    const float tmp = y + sum;
    u64 sb = __ballot((qk_bits(tmp) >> 31) != 0);
    u64 hb = __ballot(!(tmp >= 0.0f));
    const size_t bi = (size_t)g * N + v;
    const u64 dm = done[g];
    if (dm) { sb = (sb & ~dm) | (sgn[bi] & dm); hb = (hb & ~dm) | (hard[bi] & dm); }
    if (lane == 0) { sgn[bi] = sb; hard[bi] = hb; }
    if (post_out) post_out[((size_t)g * N + v) * 64 + lane] = tmp;
}

#endif /* QLDPC_KERNELS_FPOST_H */
