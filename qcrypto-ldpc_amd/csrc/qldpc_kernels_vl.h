/*
 * qldpc_kernels_vl.h -- the vertical-layered schedule (Decoder_LDPC_BP_vertical_layered, VAR/main.cpp (alist-v1.0.1):240-256) on the
 * FRAMES engine's layout: post [G][N][FG], msg [G][E][FG] CN-major, lane = frame, V frames per lane.
 *
 * One sweep visits the VNs in the code's vlayer order (qldpc_graph.c: build_vlayers); for VN v and each of its checks c, in slot order:
 *   in[i]  = var_nodes[v_i] - messages[c, i]     for ALL i of check c (v's own position p included)
 *   out    = the rule's fold over in[.]           qk_acc<FAM>, the horizontal sweep's arithmetic in the same operation order
 *   messages[c, p] = out[p]; var_nodes[v] = in[p] + out[p]      only v's own edge and posterior are written
 * i.e. the horizontal recursion per (v, c) pair with the write set cut down to v.  AFF3CT's source is not in the reference tree: this is a
 * restatement, parity unpinned against AFF3CT; bit-exact means against tests/vlayered_ref.py, whose horizontal branch is pinned to the oracle.
 *
 * One launch per class of mutually check-disjoint VNs, one wavefront per VN: every row a wave reads besides its own belongs to a VN of
 * another class, so nothing it reads is written during the launch.  The VN's posterior stays in registers between its checks.  A check's
 * rows are asked for eight at a time (16 V registers in flight, any degree); only the own input survives the fold, so there is no
 * degree-sized register array and no degree bucket.  Message rows are re-read by every other VN of their check within the sweep: cached
 * loads and stores, not the streaming forms of the flooding passes.  Compiled with -ffp-contract=off like every exact kernel here.
 */
#ifndef QLDPC_KERNELS_VL_H
#define QLDPC_KERNELS_VL_H

#include "qldpc_kernels.h"

#define QK_VL_CHUNK 8

template <int V, int FAM>
__global__ __launch_bounds__(QK_THREADS) void qk_vn_vlayer(float *__restrict__ post, float *__restrict__ msg,
                                                           const int *__restrict__ list, int n_list,
                                                           const int *__restrict__ vn_ptr, const int *__restrict__ vn_chk, const int *__restrict__ vn_tr,
                                                           const int *__restrict__ cn_ptr, const int *__restrict__ cn_var /* padded by QK_IDX_PAD */,
                                                           int N, size_t group_stride, const u64 *__restrict__ done, qk_rule rule, int freeze,
                                                           const u64 *__restrict__ synd, int M)
{
    constexpr int FG = 64 * V;
    const int g = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int i = blockIdx.x * QK_WAVES + wave;
    if (i >= n_list) return;
    if (qk_group_done<V>(done, g)) return;
    const int v = list[i];
    const int s0 = vn_ptr[v], s1 = vn_ptr[v + 1];
    bool frozen[V];
    const bool any_frozen = qk_frozen<V>(done, g, lane, frozen) && freeze;
    float *pg = post + (size_t)g * N * FG + lane * V;
    float *mg = msg + (size_t)g * group_stride + lane * V;

    float own[V];
    qk_load<V>(own, pg + (size_t)v * FG);
    for (int s = s0; s < s1; s++) {
        const int c = vn_chk[s];
        const int k = vn_tr[s];              /* CN-major edge of (v, c) */
        const int b = cn_ptr[c];
        const int deg = cn_ptr[c + 1] - b;
        const int p = k - b;
        qk_acc<FAM> acc[V];
#pragma unroll
        for (int j = 0; j < V; j++) {
            acc[j].begin();
            /* syndrome form: the check must come out with parity s_c, i.e. its sign product starts at (-1)^s_c */
            if (synd) acc[j].sign = (uint32_t)((synd[((size_t)g * M + c) * V + j] >> lane) & 1ull) << 31;
        }
        float xp[V];
#pragma unroll
        for (int j = 0; j < V; j++) xp[j] = 0.0f;
        for (int k0 = 0; k0 < deg; k0 += QK_VL_CHUNK) {
            int vn[QK_VL_CHUNK];
#pragma unroll
            for (int u = 0; u < QK_VL_CHUNK; u++) vn[u] = cn_var[b + k0 + u];      /* past the check's end: the next check's VNs or the padding, never used */
            float x[QK_VL_CHUNK][V], m[QK_VL_CHUNK][V];
#pragma unroll
            for (int u = 0; u < QK_VL_CHUNK; u++)
                if (k0 + u < deg) {
                    if (k0 + u != p) qk_load<V>(x[u], pg + (size_t)vn[u] * FG);
                    qk_load<V>(m[u], mg + (size_t)(b + k0 + u) * FG);
                }
#pragma unroll
            for (int u = 0; u < QK_VL_CHUNK; u++)
                if (k0 + u < deg) {
                    const bool mine = k0 + u == p;      /* wave-uniform */
#pragma unroll
                    for (int j = 0; j < V; j++) {
                        const float in = (mine ? own[j] : x[u][j]) - m[u][j];
                        if (mine) xp[j] = in;
                        qk_acc_in<FAM>(acc[j], qk_prep<FAM>(in), rule);
                    }
                }
        }
        float o[V];
#pragma unroll
        for (int j = 0; j < V; j++) {
            acc[j].finish(rule);
            o[j] = acc[j].out(qk_prep<FAM>(xp[j]), rule);
            own[j] = xp[j] + o[j];
        }
        qk_store_masked<V>(mg + (size_t)k * FG, o, frozen, any_frozen);
    }
    qk_store_masked<V>(pg + (size_t)v * FG, own, frozen, any_frozen);
}

#endif /* QLDPC_KERNELS_VL_H */
