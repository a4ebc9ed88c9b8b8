/*
 * qldpc_kernels_gang.h -- one colour step of SEVERAL horizontal-layered decoders as one launch (decoder gangs, qldpc.h "decoder gangs").
 *
 * A layered sweep of one decoder is a launch per layer and degree bucket (qk_cn_layer / qk_cn_layer_cst); with a handful of codes in
 * flight -- the rate groups of a reconciliation call -- the device sees that many under-filled launches side by side.  The gang kernels
 * below run the SAME per-check code (qk_cn_layer_body / qk_cn_layer_cst_body: the solo kernels call the very same functions) for up to
 * QK_GANG_SLOTS decoders ("members") whose step falls into the same kernel class (degree cap, rule family, explicit messages / compressed
 * check state), in one 1-D grid:
 *
 *     blocks of member m = ceil(n_m / QK_WAVES) * G_m      (n_m checks in its bucket, G_m groups that hold frames)
 *     grid = sum over the members present; prefix[] = the running sum, passed by value
 *
 * A workgroup finds (member, local block) with qk_gang_locate -- an unrolled compare-and-count over the prefix, no indexing of the kernel
 * arguments by a runtime value (that would put them into scratch) -- then g = local / bx_m, i = (local % bx_m) * QK_WAVES + wave.  What the
 * solo kernels get as arguments comes by scalar loads from the member's qk_gang_entry, which the host wrote once per (decoder, layer, bucket)
 * when the decoder first joined a gang; the kernel arguments carry only what changes between loads and sweeps (target syndromes, the
 * "sweep 0: messages are zero" bit).  Everything a wave addresses its rows with stays wave-uniform, as in the solo kernels.
 *
 * Only 64-frame groups (V = 1), no REMAP instances (a gang member does not compact), fp32.  Members share nothing; steps are ordered by the
 * stream.  The cost against separate streams is unmeasured until tools/gang_cost.py has run on the device.
 */
#ifndef QLDPC_KERNELS_GANG_H
#define QLDPC_KERNELS_GANG_H

#include "qldpc_kernels.h"
#include "qldpc_kernels_cst.h"

#define QK_GANG_SLOTS 8      /* members one launch covers */

/* A pointer read from memory is a generic one to the compiler: rows would move by flat loads and stores and the records by vector loads.  The entry
 * therefore says where its pointers point, in the device's view of it (same layout): device memory a lane writes (global), or data nothing writes
 * while the kernel runs (constant: the graph, the lists and records, and the done words, which only other launches write).  That gives the global
 * row accesses and the scalar loads the solo kernels get from their arguments. */
#if defined(__HIP_DEVICE_COMPILE__)
#define QK_GANG_GLOBAL __attribute__((address_space(1)))
#define QK_GANG_CONST __attribute__((address_space(4)))
#else
#define QK_GANG_GLOBAL
#define QK_GANG_CONST
#endif

/* what a solo layer launch passes as arguments, for one (decoder, layer, bucket); lives in device memory next to the bucket it describes */
struct qk_gang_entry {
    QK_GANG_GLOBAL float *post, *msg;      /* d_a, d_b: posteriors, messages / check state */
    const QK_GANG_CONST u64 *done;
    const QK_GANG_CONST int *list, *rec;   /* bucket::d_list, bucket::d_rec (NULL: walk list -> cn_ptr -> cn_var) */
    const QK_GANG_CONST int *cn_ptr, *cn_var;
    size_t group_stride;
    int n, rec_stride, N, M;
    qk_rule rule;
    int freeze, pad;
};

/* host side: store a device pointer into a field of the two structs (the device pass of the compiler sees the host code too, with the fields' address spaces) */
template <typename D, typename S> static inline void qk_gang_set(D &dst, S *src) { dst = (D)(uintptr_t)src; }

struct qk_gang_args {
    const QK_GANG_CONST qk_gang_entry *entry[QK_GANG_SLOTS];
    const QK_GANG_CONST u64 *synd[QK_GANG_SLOTS];  /* target syndromes of the syndrome form (NULL: H x = 0): set by the member's loads */
    int prefix[QK_GANG_SLOTS + 1];   /* prefix[k] = first block of slot k; slots past the last one in use repeat the total */
    unsigned first;                  /* bit k: sweep 0 of slot k, its messages are taken as zero */
};

/* block -> (slot, block within the slot's range): the slot whose half-open range [prefix[k], prefix[k + 1]) holds the block.  Slots of zero
 * blocks are passed over (their range is empty); a block at or past prefix[QK_GANG_SLOTS] gives slot QK_GANG_SLOTS.  The same code on the
 * host (qldpc_gang_locate_host) and in the kernels. */
__host__ __device__ inline void qk_gang_locate(const int (&prefix)[QK_GANG_SLOTS + 1], int block, int *slot, int *local)
{
    int k = 0, base = 0;
#pragma unroll
    for (int j = 1; j <= QK_GANG_SLOTS; j++) {
        const bool past = block >= prefix[j];
        k += past ? 1 : 0;
        base = past ? prefix[j] : base;
    }
    *slot = k;
    *local = block - base;
}

#define QK_GANG_PICK(dst, arr, slot) \
    _Pragma("unroll") for (int j_ = 1; j_ < QK_GANG_SLOTS; j_++) dst = (slot) == j_ ? (arr)[j_] : dst

template <int DCMAX, int FAM>
__global__ __launch_bounds__(QK_THREADS) void qk_cn_layer_gang(const qk_gang_args a)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int slot, local;
    qk_gang_locate(a.prefix, (int)blockIdx.x, &slot, &local);
    if (slot >= QK_GANG_SLOTS) return;
    const QK_GANG_CONST qk_gang_entry *e = a.entry[0];
    const QK_GANG_CONST u64 *synd = a.synd[0];
    QK_GANG_PICK(e, a.entry, slot);
    QK_GANG_PICK(synd, a.synd, slot);
    const int first = (int)((a.first >> slot) & 1u);
    const int n = e->n;
    /* what the record and done loads need comes with n, not in a round trip of its own behind the bounds test below */
    asm volatile("" ::"s"(n), "s"(e->rec), "s"(e->rec_stride), "s"(e->done), "s"(e->post));
    const unsigned bx = (unsigned)(n + QK_WAVES - 1) / QK_WAVES;
    /* the quotient comes out of the vector unit (there is no scalar divide): brought back into an SGPR, or the record loads behind it turn into vector loads */
    const int g = __builtin_amdgcn_readfirstlane((int)((unsigned)local / bx));
    const int i = (local - g * (int)bx) * QK_WAVES + wave;
    if (i >= n) return;
    qk_cn_layer_body<1, DCMAX, FAM, false>(g, lane, i, (float *)e->post, (float *)e->msg, (const int *)e->list, (const int *)e->cn_ptr, (const int *)e->cn_var, e->N,
                                           e->group_stride, (const u64 *)e->done, e->rule, e->freeze, (const u64 *)synd, e->M, first, (const int *)e->rec, e->rec_stride,
                                           qk_layer_remap<false>{});
}

template <int DCMAX, int FAM>
__global__ __launch_bounds__(QK_THREADS) void qk_cn_layer_cst_gang(const qk_gang_args a)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int slot, local;
    qk_gang_locate(a.prefix, (int)blockIdx.x, &slot, &local);
    if (slot >= QK_GANG_SLOTS) return;
    const QK_GANG_CONST qk_gang_entry *e = a.entry[0];
    const QK_GANG_CONST u64 *synd = a.synd[0];
    QK_GANG_PICK(e, a.entry, slot);
    QK_GANG_PICK(synd, a.synd, slot);
    const int first = (int)((a.first >> slot) & 1u);
    const int n = e->n;
    /* what the record and done loads need comes with n, not in a round trip of its own behind the bounds test below */
    asm volatile("" ::"s"(n), "s"(e->rec), "s"(e->rec_stride), "s"(e->done), "s"(e->post));
    const unsigned bx = (unsigned)(n + QK_WAVES - 1) / QK_WAVES;
    /* the quotient comes out of the vector unit (there is no scalar divide): brought back into an SGPR, or the record loads behind it turn into vector loads */
    const int g = __builtin_amdgcn_readfirstlane((int)((unsigned)local / bx));
    const int i = (local - g * (int)bx) * QK_WAVES + wave;
    if (i >= n) return;
    qk_cn_layer_cst_body<DCMAX, FAM, false>(g, lane, i, (float *)e->post, (float *)e->msg, (const int *)e->list, (const int *)e->cn_ptr, (const int *)e->cn_var, e->N,
                                            e->group_stride, (const u64 *)e->done, e->rule, (const u64 *)synd, e->M, first, (const int *)e->rec, e->rec_stride,
                                            qk_layer_remap<false>{});
}

#endif /* QLDPC_KERNELS_GANG_H */
