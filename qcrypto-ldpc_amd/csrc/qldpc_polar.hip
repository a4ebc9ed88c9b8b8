/*
 * qldpc_polar.hip -- the context and the launches of qldpc_polar_*: a batched polar encoder and successive-cancellation decoder.  The rules are
 * qldpc_polar_core.h's, the kernels and the layout of the scratch qldpc_kernels_polar.h's, the host mirrors qldpc_polar_host.c's.
 *
 * A context owns everything a call touches: the frozen mask and info_pos on the device, the belief scratch of ceil(max_frames / 64) groups and
 * their u and x rows.  A call allocates nothing and waits for nothing: its two or three kernels go onto the context's stream in order.
 *
 * A context of the WIDE form (qldpc_polar_create_form, QLDPC_POLAR_WIDE) decodes with a workgroup per frame (qldpc_kernels_polar_wide.h, one
 * kernel a call) and owns the scratch of qldpc_polar_wide_core.h instead: max_frames x plw_scratch_elems beliefs and two rows a frame.  Frames of
 * n <= 5 are one leaf block and go the lanes' way in either form.  QLDPC_POLAR_WIDE_CHIP (6 .. 13), QLDPC_POLAR_WIDE_LANES (64, 256, 512, 1024)
 * and QLDPC_POLAR_WIDE_LEAF (1 or 32) in the environment replace the chip level, the workgroup size and the lanes of a leaf block of the
 * contexts created after: what tools/polar_wide_cost.py measures the alternatives with.
 */
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "qldpc_hip.h"
#include "qldpc_kernels_polar.h"
#include "qldpc_kernels_polar_wide.h"
#include "qldpc_polar_core.h"
#include "qldpc_polar_wide_core.h"

struct qldpc_polar {
    int n, n_info, messages, maxq, max_frames, device;
    bool wide;                     /* the wide form at work: QLDPC_POLAR_WIDE and n > 5 */
    int chip, lanes, leaf_lanes;   /* wide: the chip level asked for, the workgroup, and the lanes of a leaf block (32, or 0: one) */
    size_t groups, W;
    hipStream_t stream;
    uint32_t *d_fmask;             /* W words: 1 = frozen */
    int *d_info_pos;
    void *d_B;                     /* groups x pl_group_elems(n) int8 or float, NULL for n <= 5; wide: max_frames x plw_scratch_elems(n, chip) */
    uint32_t *d_U, *d_X;           /* groups x W x 64 each; wide: max_frames x W each */
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

/* the workgroup of a wide context: a size plw_launch has an instance of */
static bool plw_lanes_ok(int lanes) { return lanes == 64 || lanes == 256 || lanes == 512 || lanes == 1024; }

static int pl_create(int log2_n, int n_info, const int *info_pos, int messages, int maxq, int max_frames, int form, int device, qldpc_polar **out)
{
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
    p->wide = form == QLDPC_POLAR_WIDE && log2_n > PL_SUB_LOG;
    p->chip = PLW_CHIP_LOG; p->lanes = PLW_LANES; p->leaf_lanes = PLW_LEAF_LANES;
    if (p->wide) {
        if (const char *e = getenv("QLDPC_POLAR_WIDE_CHIP")) { const int c = atoi(e); if (c >= PLW_CHIP_MIN && c <= PLW_CHIP_MAX) p->chip = c; }
        if (const char *e = getenv("QLDPC_POLAR_WIDE_LANES")) { const int l = atoi(e); if (plw_lanes_ok(l)) p->lanes = l; }
        if (const char *e = getenv("QLDPC_POLAR_WIDE_LEAF")) { const int l = atoi(e); if (l == 1 || l == 32) p->leaf_lanes = l == 32 ? 32 : 0; }
    }
    const size_t esz = messages == QLDPC_POLAR_I8 ? 1 : sizeof(float);
    if (p->wide && esz * plw_lds_elems(log2_n, p->chip) + 4 * sizeof(uint32_t) * PLW_WIN > 65536) {      /* float messages at chip level 13: past what a launch gets unasked */
        const int bytes = (int)(esz * plw_lds_elems(log2_n, p->chip));
        const void *fn = p->lanes == 64 ? (const void *)plw_decode<pl_msg_f32, 64> : p->lanes == 512 ? (const void *)plw_decode<pl_msg_f32, 512>
                       : p->lanes == 1024 ? (const void *)plw_decode<pl_msg_f32, 1024> : (const void *)plw_decode<pl_msg_f32, 256>;
        (void)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);      /* a launch that this did not make room for reports its own error */
        (void)hipGetLastError();
    }
    /* beliefs and words of each of the two rows: by groups of 64 frames, or by frames */
    const size_t beliefs = p->wide ? (size_t)max_frames * plw_scratch_elems(log2_n, p->chip) : p->groups * pl_group_elems(log2_n);
    const size_t row_words = p->wide ? (size_t)max_frames * W : p->groups * W * PL_GROUP;
    int rc = QLDPC_OK;
    auto alloc = [&](void **q, size_t bytes) {
        if (!bytes || rc) return;
        if (hipMalloc(q, bytes) != hipSuccess) { (void)hipGetLastError(); rc = QLDPC_ENOMEM; } else p->dev_bytes += bytes;
    };
    alloc((void **)&p->d_fmask, sizeof(uint32_t) * W);
    alloc((void **)&p->d_info_pos, sizeof(int) * (size_t)(n_info > 0 ? n_info : 1));
    alloc(&p->d_B, esz * beliefs);
    alloc((void **)&p->d_U, sizeof(uint32_t) * row_words);
    alloc((void **)&p->d_X, sizeof(uint32_t) * row_words);
    if (rc) {
        qldpc_set_error("polar_create: device allocation failed (about %zu MiB for max_frames=%d at N = 2^%d: lower max_frames)",
                        (esz * beliefs + 8 * row_words) >> 20, max_frames, log2_n);
        qldpc_polar_free(p);
        return rc;
    }
    hipError_t he = hipMemcpy(p->d_fmask, mask.data(), sizeof(uint32_t) * W, hipMemcpyHostToDevice);
    if (he == hipSuccess && n_info > 0) he = hipMemcpy(p->d_info_pos, info_pos, sizeof(int) * (size_t)n_info, hipMemcpyHostToDevice);
    if (he != hipSuccess) { qldpc_set_error("polar_create: %s", hipGetErrorString(he)); qldpc_polar_free(p); return QLDPC_EHIP; }
    *out = p;
    return QLDPC_OK;
}

extern "C" int qldpc_polar_create(int log2_n, int n_info, const int *info_pos, int messages, int maxq, int max_frames, int device, qldpc_polar **out)
{
    if (!out) return QLDPC_EINVAL;
    *out = nullptr;
    return pl_create(log2_n, n_info, info_pos, messages, maxq, max_frames, QLDPC_POLAR_LANES, device, out);
}

extern "C" int qldpc_polar_create_form(int log2_n, int n_info, const int *info_pos, int messages, int maxq, int max_frames, int form, int device,
                                       qldpc_polar **out)
{
    if (!out) return QLDPC_EINVAL;
    *out = nullptr;
    if (form != QLDPC_POLAR_LANES && form != QLDPC_POLAR_WIDE) {
        qldpc_set_error("polar_create_form: form=%d (QLDPC_POLAR_LANES = %d or QLDPC_POLAR_WIDE = %d)", form, QLDPC_POLAR_LANES, QLDPC_POLAR_WIDE);
        return QLDPC_EINVAL;
    }
    return pl_create(log2_n, n_info, info_pos, messages, maxq, max_frames, form, device, out);
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

/* the wide form: one kernel, a workgroup per frame, which writes every output the caller asked for */
template <class M, int LANES>
static void plw_launch(const qldpc_polar *p, M m, int n_frames, const void *d_llr, const uint32_t *d_frozen_u, uint32_t *d_u, uint32_t *d_info,
                       uint32_t *d_x, void *d_leaf)
{
    typedef typename M::mem mem;
    const size_t lds = sizeof(mem) * plw_lds_elems(p->n, p->chip);
    hipLaunchKernelGGL((plw_decode<M, LANES>), dim3((unsigned)n_frames), dim3(LANES), lds, p->stream, m, p->n, plw_chip(p->n, p->chip), p->leaf_lanes, (const mem *)d_llr,
                       (const uint32_t *)p->d_fmask, d_frozen_u, (mem *)p->d_B, p->d_U, p->d_X, d_u, d_x, d_info, p->n_info, (const int *)p->d_info_pos,
                       (mem *)d_leaf);
}

template <class M>
static int plw_run_decode(const qldpc_polar *p, M m, int n_frames, const void *d_llr, const uint32_t *d_frozen_u, uint32_t *d_u, uint32_t *d_info,
                          uint32_t *d_x, void *d_leaf)
{
    switch (p->lanes) {
    case 64: plw_launch<M, 64>(p, m, n_frames, d_llr, d_frozen_u, d_u, d_info, d_x, d_leaf); break;
    case 512: plw_launch<M, 512>(p, m, n_frames, d_llr, d_frozen_u, d_u, d_info, d_x, d_leaf); break;
    case 1024: plw_launch<M, 1024>(p, m, n_frames, d_llr, d_frozen_u, d_u, d_info, d_x, d_leaf); break;
    default: plw_launch<M, 256>(p, m, n_frames, d_llr, d_frozen_u, d_u, d_info, d_x, d_leaf); break;
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
    if (p->wide) {
        if (p->messages == QLDPC_POLAR_I8) return plw_run_decode(p, pl_msg_i8{p->maxq}, n_frames, d_llr, d_frozen_u, d_u, d_info, d_x, d_leaf);
        return plw_run_decode(p, pl_msg_f32{}, n_frames, d_llr, d_frozen_u, d_u, d_info, d_x, d_leaf);
    }
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
