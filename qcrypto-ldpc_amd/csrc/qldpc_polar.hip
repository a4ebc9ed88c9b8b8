/*
 * qldpc_polar.hip -- the context and the launches of qldpc_polar_*: a batched polar encoder and successive-cancellation decoder.  The rules are
 * qldpc_polar_core.h's, the kernels and the layout of the scratch qldpc_kernels_polar.h's, the host mirrors qldpc_polar_host.c's.
 *
 * A context owns everything a call touches: the frozen mask and info_pos on the device, the belief scratch of ceil(max_frames / 64) groups and
 * their u and x rows.  A call allocates nothing and waits for nothing: its two or three kernels go onto the context's stream in order.
 */
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "qldpc_hip.h"
#include "qldpc_kernels_polar.h"
#include "qldpc_polar_core.h"

struct qldpc_polar {
    int n, n_info, messages, maxq, max_frames, device;
    size_t groups, W;
    hipStream_t stream;
    uint32_t *d_fmask;             /* W words: 1 = frozen */
    int *d_info_pos;
    void *d_B;                     /* groups x pl_group_elems(n) int8 or float; NULL for n <= 5 */
    uint32_t *d_U, *d_X;           /* groups x W x 64 each */
    size_t dev_bytes;
};

extern "C" void qldpc_polar_free(qldpc_polar *p)
{
    if (!p) return;
    (void)hipSetDevice(p->device);
    (void)hipStreamSynchronize(p->stream);                       /* the last call may still read the scratch */
    if (p->d_fmask) (void)hipFree(p->d_fmask);
    if (p->d_info_pos) (void)hipFree(p->d_info_pos);
    if (p->d_B) (void)hipFree(p->d_B);
    if (p->d_U) (void)hipFree(p->d_U);
    if (p->d_X) (void)hipFree(p->d_X);
    delete p;
}

extern "C" int qldpc_polar_create(int log2_n, int n_info, const int *info_pos, int messages, int maxq, int max_frames, int device, qldpc_polar **out)
{
    if (!out) return QLDPC_EINVAL;
    *out = nullptr;
    /* every argument check before the first HIP call */
    if (pl_check_size(log2_n)) { qldpc_set_error("polar_create: log2_n=%d (1 .. %d)", log2_n, PL_MAX_LOG2N); return QLDPC_ESIZE; }
    if (messages != QLDPC_POLAR_I8 && messages != QLDPC_POLAR_F32) { qldpc_set_error("polar_create: messages=%d (QLDPC_POLAR_I8 or QLDPC_POLAR_F32)", messages); return QLDPC_EINVAL; }
    if (pl_check_maxq(messages, maxq)) {
        qldpc_set_error("polar_create: maxq=%d (1 .. %d: f is not saturated and gives maxq + 1, which an int8 holds up to 127; use maxq <= %d)", maxq, PL_MAX_MAXQ, PL_MAX_MAXQ);
        return QLDPC_ESIZE;
    }
    if (max_frames < 1 || max_frames > (1 << 24)) { qldpc_set_error("polar_create: max_frames=%d (1 .. %d)", max_frames, 1 << 24); return QLDPC_EINVAL; }
    const size_t W = (size_t)pl_words(log2_n);
    std::vector<uint32_t> mask(W, 0u);
    const int bad = pl_mark_info(log2_n, n_info, info_pos, mask.data());
    if (bad) {
        if (bad == PL_EINVAL) qldpc_set_error("polar_create: info_pos names a position twice (positions must be distinct)");
        else qldpc_set_error("polar_create: n_info=%d positions, each in 0 .. N - 1, are required (0 <= n_info <= N = %ld)", n_info, 1l << log2_n);
        return bad;
    }
    const uint32_t valid = pl_row_mask(log2_n);
    for (size_t w = 0; w < W; w++) mask[w] = ~mask[w] & valid;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { qldpc_set_error("no HIP device visible: libqldpc has no CPU fallback"); return QLDPC_ENODEV; }
    if (device < 0 || device >= ndev) { qldpc_set_error("device %d out of range", device); return QLDPC_ENODEV; }
    HIPCHK(hipSetDevice(device));
    qldpc_polar *p = new (std::nothrow) qldpc_polar();
    if (!p) return QLDPC_ENOMEM;
    p->n = log2_n; p->n_info = n_info; p->messages = messages; p->maxq = maxq; p->max_frames = max_frames; p->device = device;
    p->W = W; p->groups = ((size_t)max_frames + PL_GROUP - 1) / PL_GROUP;
    const size_t esz = messages == QLDPC_POLAR_I8 ? 1 : sizeof(float);
    int rc = QLDPC_OK;
    auto alloc = [&](void **q, size_t bytes) {
        if (!bytes || rc) return;
        if (hipMalloc(q, bytes) != hipSuccess) { (void)hipGetLastError(); rc = QLDPC_ENOMEM; } else p->dev_bytes += bytes;
    };
    alloc((void **)&p->d_fmask, sizeof(uint32_t) * W);
    alloc((void **)&p->d_info_pos, sizeof(int) * (size_t)(n_info > 0 ? n_info : 1));
    alloc(&p->d_B, esz * p->groups * pl_group_elems(log2_n));
    alloc((void **)&p->d_U, sizeof(uint32_t) * p->groups * W * PL_GROUP);
    alloc((void **)&p->d_X, sizeof(uint32_t) * p->groups * W * PL_GROUP);
    if (rc) {
        qldpc_set_error("polar_create: device allocation failed (about %zu MiB for max_frames=%d at N = 2^%d: lower max_frames)",
                        (esz * p->groups * pl_group_elems(log2_n) + 8 * p->groups * W * PL_GROUP) >> 20, max_frames, log2_n);
        qldpc_polar_free(p);
        return rc;
    }
    hipError_t he = hipMemcpy(p->d_fmask, mask.data(), sizeof(uint32_t) * W, hipMemcpyHostToDevice);
    if (he == hipSuccess && n_info > 0) he = hipMemcpy(p->d_info_pos, info_pos, sizeof(int) * (size_t)n_info, hipMemcpyHostToDevice);
    if (he != hipSuccess) { qldpc_set_error("polar_create: %s", hipGetErrorString(he)); qldpc_polar_free(p); return QLDPC_EHIP; }
    *out = p;
    return QLDPC_OK;
}

extern "C" size_t qldpc_polar_device_bytes(const qldpc_polar *p) { return p ? p->dev_bytes : 0; }

extern "C" int qldpc_polar_set_stream(qldpc_polar *p, void *hip_stream)
{
    if (!p) return QLDPC_EINVAL;
    p->stream = (hipStream_t)hip_stream;
    return QLDPC_OK;
}

static int pl_check_frames(const qldpc_polar *p, int n_frames, const char *who)
{
    if (!p) return QLDPC_EINVAL;
    if (n_frames < 0) { qldpc_set_error("%s: n_frames=%d is negative", who, n_frames); return QLDPC_EINVAL; }
    if (n_frames > p->max_frames) { qldpc_set_error("%s: n_frames=%d exceeds the context's max_frames=%d: create it larger or split the call", who, n_frames, p->max_frames); return QLDPC_ESIZE; }
    return QLDPC_OK;
}

extern "C" int qldpc_polar_encode_dev(qldpc_polar *p, int n_frames, const uint32_t *d_u, uint32_t *d_x)
{
    const int rc = pl_check_frames(p, n_frames, "polar_encode_dev");
    if (rc || n_frames == 0) return rc;
    if (!d_u || !d_x) { qldpc_set_error("polar_encode_dev: NULL device pointer"); return QLDPC_EINVAL; }
    HIPCHK(hipSetDevice(p->device));
    const size_t tiles = p->W > PL_ENC_TILE ? p->W / PL_ENC_TILE : 1;
    hipLaunchKernelGGL(pl_encode_tiles, dim3((unsigned)((size_t)n_frames * tiles)), dim3(PL_ENC_LANES), 0, p->stream, p->n, d_u, d_x);
    LAUNCHCHK();
    if (tiles > 1) {
        const size_t threads = (size_t)n_frames * PL_ENC_TILE;
        hipLaunchKernelGGL(pl_encode_columns, dim3((unsigned)(threads / PL_ENC_LANES)), dim3(PL_ENC_LANES), 0, p->stream, p->n, n_frames, d_x);
        LAUNCHCHK();
    }
    return QLDPC_OK;
}

template <class M, int SL, bool TOP>
static void pl_launch_decode(const qldpc_polar *p, M m, int n_frames, unsigned groups, const void *d_llr, const uint32_t *d_frozen_u, void *d_leaf)
{
    typedef typename M::mem mem;
    hipLaunchKernelGGL((pl_decode<M, SL, TOP>), dim3(groups), dim3(PL_GROUP), 0, p->stream, m, p->n, n_frames, (const mem *)d_llr, (const uint32_t *)p->d_fmask,
                       d_frozen_u, (mem *)p->d_B, p->d_U, p->d_X, (mem *)d_leaf);
}

template <class M>
static int pl_run_decode(const qldpc_polar *p, M m, int n_frames, const void *d_llr, const uint32_t *d_frozen_u, void *d_leaf)
{
    typedef typename M::mem mem;
    const unsigned groups = (unsigned)(((size_t)n_frames + PL_GROUP - 1) / PL_GROUP);
    if (p->n > PL_SUB_LOG) {
        const size_t tiles = ((size_t)1 << p->n) / 64u;
        hipLaunchKernelGGL(pl_load<M>, dim3((unsigned)(groups * tiles)), dim3(256), 0, p->stream, m, p->n, n_frames, (const mem *)d_llr, (mem *)p->d_B);
        LAUNCHCHK();
    }
    switch (p->n) {
    case 1: pl_launch_decode<M, 1, true>(p, m, n_frames, groups, d_llr, d_frozen_u, d_leaf); break;
    case 2: pl_launch_decode<M, 2, true>(p, m, n_frames, groups, d_llr, d_frozen_u, d_leaf); break;
    case 3: pl_launch_decode<M, 3, true>(p, m, n_frames, groups, d_llr, d_frozen_u, d_leaf); break;
    case 4: pl_launch_decode<M, 4, true>(p, m, n_frames, groups, d_llr, d_frozen_u, d_leaf); break;
    case 5: pl_launch_decode<M, 5, true>(p, m, n_frames, groups, d_llr, d_frozen_u, d_leaf); break;
    default: pl_launch_decode<M, 5, false>(p, m, n_frames, groups, d_llr, d_frozen_u, d_leaf); break;
    }
    LAUNCHCHK();
    return QLDPC_OK;
}

extern "C" int qldpc_polar_decode_dev(qldpc_polar *p, int n_frames, const void *d_llr, const uint32_t *d_frozen_u, uint32_t *d_u, uint32_t *d_info,
                                      uint32_t *d_x, void *d_leaf)
{
    int rc = pl_check_frames(p, n_frames, "polar_decode_dev");
    if (rc || n_frames == 0) return rc;
    if (!d_llr) { qldpc_set_error("polar_decode_dev: d_llr is NULL"); return QLDPC_EINVAL; }
    HIPCHK(hipSetDevice(p->device));
    if (p->messages == QLDPC_POLAR_I8) rc = pl_run_decode(p, pl_msg_i8{p->maxq}, n_frames, d_llr, d_frozen_u, d_leaf);
    else rc = pl_run_decode(p, pl_msg_f32{}, n_frames, d_llr, d_frozen_u, d_leaf);
    if (rc) return rc;
    if (d_u || d_info || d_x) {
        const size_t groups = ((size_t)n_frames + PL_GROUP - 1) / PL_GROUP, threads = groups * p->W * PL_GROUP;
        hipLaunchKernelGGL(pl_outputs, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, p->stream, p->n, n_frames, p->n_info, (const int *)p->d_info_pos,
                           (const uint32_t *)p->d_U, (const uint32_t *)p->d_X, d_u, d_info, d_x);
        LAUNCHCHK();
    }
    return QLDPC_OK;
}
