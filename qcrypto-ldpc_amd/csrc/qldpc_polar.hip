/*
 * qldpc_polar.hip -- the context and the launches of qldpc_polar_*: a batched polar encoder and successive-cancellation decoder.  The rules are
 * qldpc_polar_core.h's, the kernels and the layout of the scratch qldpc_kernels_polar.h's, the host mirrors qldpc_polar_host.c's, and what a
 * context shares with the list decoder's qldpc_polar_ctx.h's.
 *
 * A context owns everything a call touches: the frozen mask and info_pos on the device, the belief scratch of ceil(max_frames / 64) groups and
 * their u and x rows.  A call allocates nothing and waits for nothing: its two or three kernels go onto the context's stream in order.
 *
 * A context of the WIDE form (qldpc_polar_create_form, QLDPC_POLAR_WIDE) decodes with a workgroup per frame (qldpc_kernels_polar_wide.h, one
 * kernel a call) and owns the scratch of qldpc_polar_wide_core.h instead: max_frames x plw_scratch_elems beliefs and two rows a frame.  Frames of
 * n <= 5 are one leaf block and go the lanes' way in either form.  QLDPC_POLAR_WIDE_CHIP (6 .. 13), QLDPC_POLAR_WIDE_LANES (64, 256, 512, 1024)
 * and QLDPC_POLAR_WIDE_LEAF (1 or 32) in the environment replace the chip level, the workgroup size and the lanes of a leaf block of the
 * contexts created after: what tools/polar_wide_cost.py measures the alternatives with.
 *
 * A context of the SSC rule (qldpc_polar_create_rule, QLDPC_POLAR_SSC; the rule and the plan are qldpc_polar_ssc_core.h's) is a lanes context that
 * also owns the plan of its code on the device and decodes with pl_ssc_decode (qldpc_kernels_polar_ssc.h) in pl_decode's place; everything else,
 * the tally included, is the lanes form's.
 *
 * qldpc_polar_tally_dev (the genie-aided construction, qldpc_polar_tally_core.h) is the lanes' decode in its tally form
 * (qldpc_kernels_polar_tally.h): pl_load, then pl_tally on the same scratch, into an accumulator that is the caller's.
 *
 * qldpc_polar_decode_rows_dev is the lanes' SC decode with a frozen set per frame (qldpc_kernels_polar_rows.h): pl_load, pl_decode_rows in
 * pl_decode's place on the same scratch, pl_outputs.
 */
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <new>
#include <type_traits>

#include "qldpc_kernels_polar_rows.h"
#include "qldpc_kernels_polar_ssc.h"
#include "qldpc_kernels_polar_tally.h"
#include "qldpc_kernels_polar_wide.h"
#include "qldpc_polar_ctx.h"

struct qldpc_polar {
    pl_ctx c;
    bool wide;                     /* the wide form at work: QLDPC_POLAR_WIDE and n > 5 */
    int chip, lanes, leaf_lanes;   /* wide: the chip level asked for, the workgroup, and the lanes of a leaf block (32, or 0: one) */
    void *d_B;                     /* groups x pl_group_elems(n) int8 or float, NULL for n <= 5; wide: max_frames x plw_scratch_elems(n, chip) */
    uint32_t *d_U, *d_X;           /* groups x W x 64 each; wide: max_frames x W each */
    int rule;                      /* QLDPC_POLAR_SC or QLDPC_POLAR_SSC */
    int *d_steps;                  /* SSC: the plan of the code, n_steps x PL_SSC_STEP ints; NULL otherwise */
    int n_steps;
};

const pl_ctx *pl_ctx_of_sc(const qldpc_polar *p) { return &p->c; }
bool pl_sc_is_wide(const qldpc_polar *p) { return p->wide; }
int pl_sc_rule(const qldpc_polar *p) { return p->rule; }

extern "C" void qldpc_polar_free(qldpc_polar *p)
{
    if (!p) return;
    pl_ctx_free(&p->c);
    delete p;
}

/* fn(an integral_constant of the workgroup size) for the sizes plw_decode has an instance of; any other: the default */
template <class Fn> static auto plw_with_lanes(int lanes, Fn fn)
{
    switch (lanes) {
    case 64: return fn(std::integral_constant<int, 64>{});
    case 512: return fn(std::integral_constant<int, 512>{});
    case 1024: return fn(std::integral_constant<int, 1024>{});
    default: return fn(std::integral_constant<int, PLW_LANES>{});
    }
}

/* the plan of an SSC context, built from the code and sent up; the context's ledger owns it */
static int pl_upload_plan(qldpc_polar *p, const int *info_pos)
{
    uint32_t *mask = nullptr;
    int rc = pl_args_frozen_mask("polar_create", p->c.n, p->c.n_info, info_pos, &mask);
    if (rc) return rc;
    int *steps = (int *)malloc(sizeof(int) * PL_SSC_STEP * (size_t)pl_ssc_max_steps(p->c.n));
    if (!steps) { free(mask); return QLDPC_ENOMEM; }
    p->n_steps = (int)pl_ssc_plan(p->c.n, mask, steps);
    free(mask);
    pl_ctx_alloc(&p->c, &p->d_steps, sizeof(int) * PL_SSC_STEP * (size_t)p->n_steps);
    hipError_t e = hipSuccess;
    if (!p->c.alloc_failed) e = hipMemcpy(p->d_steps, steps, sizeof(int) * PL_SSC_STEP * (size_t)p->n_steps, hipMemcpyHostToDevice);
    free(steps);
    HIPCHK(e);
    return QLDPC_OK;
}

static int pl_create(int log2_n, int n_info, const int *info_pos, int messages, int maxq, int max_frames, int form, int rule, int device, qldpc_polar **out)
{
    qldpc_polar *p = new (std::nothrow) qldpc_polar();
    if (!p) return QLDPC_ENOMEM;
    const int rc = pl_ctx_create(&p->c, "polar_create", log2_n, PL_MAX_LOG2N, n_info, info_pos, messages, maxq, max_frames, device, [&](int stage) {
        if (stage == 0 && rule == QLDPC_POLAR_SSC && form == QLDPC_POLAR_WIDE && log2_n > PL_SUB_LOG) {
            qldpc_set_error("polar_create: the SSC rule has no wide form at log2_n=%d (> %d): create a QLDPC_POLAR_LANES context for it", log2_n, PL_SUB_LOG);
            return (int)QLDPC_EUNSUPPORTED;
        }
        return (int)QLDPC_OK;
    });
    if (rc) { qldpc_polar_free(p); return rc; }
    p->rule = rule;
    p->wide = form == QLDPC_POLAR_WIDE && log2_n > PL_SUB_LOG;
    p->chip = PLW_CHIP_LOG; p->lanes = PLW_LANES; p->leaf_lanes = PLW_LEAF_LANES;
    if (p->wide) {
        if (const char *e = getenv("QLDPC_POLAR_WIDE_CHIP")) { const int c = atoi(e); if (c >= PLW_CHIP_MIN && c <= PLW_CHIP_MAX) p->chip = c; }
        if (const char *e = getenv("QLDPC_POLAR_WIDE_LANES")) { const int l = atoi(e); if (l == 64 || l == 256 || l == 512 || l == 1024) p->lanes = l; }
        if (const char *e = getenv("QLDPC_POLAR_WIDE_LEAF")) { const int l = atoi(e); if (l == 1 || l == 32) p->leaf_lanes = l == 32 ? 32 : 0; }
    }
    const size_t esz = messages == QLDPC_POLAR_I8 ? 1 : sizeof(float), W = p->c.W;
    if (p->wide && esz * plw_lds_elems(log2_n, p->chip) + 4 * sizeof(uint32_t) * PLW_WIN > 65536) {      /* float messages at chip level 13: past what a launch gets unasked */
        const int bytes = (int)(esz * plw_lds_elems(log2_n, p->chip));
        (void)plw_with_lanes(p->lanes, [&](auto lanes) {      /* a launch that this did not make room for reports its own error */
            return hipFuncSetAttribute((const void *)plw_decode<pl_msg_f32, decltype(lanes)::value>, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        });
        (void)hipGetLastError();
    }
    /* beliefs and words of each of the two rows: by groups of 64 frames, or by frames */
    const size_t beliefs = p->wide ? (size_t)max_frames * plw_scratch_elems(log2_n, p->chip) : p->c.groups * pl_group_elems(log2_n);
    const size_t row_words = p->wide ? (size_t)max_frames * W : p->c.groups * W * PL_GROUP;
    pl_ctx_alloc(&p->c, &p->d_B, esz * beliefs);
    pl_ctx_alloc(&p->c, &p->d_U, sizeof(uint32_t) * row_words);
    pl_ctx_alloc(&p->c, &p->d_X, sizeof(uint32_t) * row_words);
    if (rule == QLDPC_POLAR_SSC && !p->c.alloc_failed)
        if (const int prc = pl_upload_plan(p, info_pos)) { qldpc_polar_free(p); return prc; }
    if (p->c.alloc_failed) {
        qldpc_set_error("polar_create: device allocation failed (about %zu MiB for max_frames=%d at N = 2^%d: lower max_frames)",
                        (esz * beliefs + 8 * row_words) >> 20, max_frames, log2_n);
        qldpc_polar_free(p);
        return QLDPC_ENOMEM;
    }
    *out = p;
    return QLDPC_OK;
}

extern "C" int qldpc_polar_create(int log2_n, int n_info, const int *info_pos, int messages, int maxq, int max_frames, int device, qldpc_polar **out)
{
    if (!out) return QLDPC_EINVAL;
    *out = nullptr;
    return pl_create(log2_n, n_info, info_pos, messages, maxq, max_frames, QLDPC_POLAR_LANES, QLDPC_POLAR_SC, device, out);
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
    return pl_create(log2_n, n_info, info_pos, messages, maxq, max_frames, form, QLDPC_POLAR_SC, device, out);
}

extern "C" int qldpc_polar_create_rule(int log2_n, int n_info, const int *info_pos, int messages, int maxq, int max_frames, int form, int rule, int device,
                                       qldpc_polar **out)
{
    if (!out) return QLDPC_EINVAL;
    *out = nullptr;
    if (rule != QLDPC_POLAR_SC && rule != QLDPC_POLAR_SSC) {
        qldpc_set_error("polar_create_rule: rule=%d (QLDPC_POLAR_SC = %d or QLDPC_POLAR_SSC = %d)", rule, QLDPC_POLAR_SC, QLDPC_POLAR_SSC);
        return QLDPC_EINVAL;
    }
    if (form != QLDPC_POLAR_LANES && form != QLDPC_POLAR_WIDE) {
        qldpc_set_error("polar_create_rule: form=%d (QLDPC_POLAR_LANES = %d or QLDPC_POLAR_WIDE = %d)", form, QLDPC_POLAR_LANES, QLDPC_POLAR_WIDE);
        return QLDPC_EINVAL;
    }
    return pl_create(log2_n, n_info, info_pos, messages, maxq, max_frames, form, rule, device, out);
}

extern "C" size_t qldpc_polar_device_bytes(const qldpc_polar *p) { return pl_ctx_device_bytes(PL_CTX(p)); }

extern "C" int qldpc_polar_set_stream(qldpc_polar *p, void *hip_stream) { return pl_ctx_set_stream(PL_CTX(p), hip_stream); }

extern "C" int qldpc_polar_encode_dev(qldpc_polar *p, int n_frames, const uint32_t *d_u, uint32_t *d_x)
{
    const int rc = pl_ctx_check_frames(PL_CTX(p), n_frames, "polar_encode_dev");
    if (rc || n_frames == 0) return rc;
    if (!d_u || !d_x) { qldpc_set_error("polar_encode_dev: NULL device pointer"); return QLDPC_EINVAL; }
    HIPCHK(hipSetDevice(p->c.device));
    return pl_launch_encode(p->c.stream, p->c.n, (size_t)n_frames, d_u, d_x);
}

template <class M, int SL, bool TOP>
static void pl_launch_decode(const qldpc_polar *p, M m, int n_frames, unsigned groups, const void *d_llr, const uint32_t *d_frozen_u, void *d_leaf)
{
    typedef typename M::mem mem;
    hipLaunchKernelGGL((pl_decode<M, SL, TOP>), dim3(groups), dim3(PL_GROUP), 0, p->c.stream, m, p->c.n, n_frames, (const mem *)d_llr, (const uint32_t *)p->c.d_fmask,
                       d_frozen_u, (mem *)p->d_B, p->d_U, p->d_X, (mem *)d_leaf);
}

template <class M, int SL, bool TOP>
static void pl_launch_ssc(const qldpc_polar *p, M m, int n_frames, unsigned groups, const void *d_llr, const uint32_t *d_frozen_u, bool want_u)
{
    typedef typename M::mem mem;
    hipLaunchKernelGGL((pl_ssc_decode<M, SL, TOP>), dim3(groups), dim3(PL_GROUP), 0, p->c.stream, m, p->c.n, n_frames, (const mem *)d_llr, (const uint32_t *)p->c.d_fmask,
                       d_frozen_u, (const int *)p->d_steps, p->n_steps, want_u, (mem *)p->d_B, p->d_U, p->d_X);
}

/* d_leaf: SC only (an SSC call with one was refused); want_u: SSC only */
template <class M>
static int pl_run_decode(const qldpc_polar *p, M m, int n_frames, const void *d_llr, const uint32_t *d_frozen_u, void *d_leaf, bool want_u)
{
    typedef typename M::mem mem;
    const int n = p->c.n;
    const unsigned groups = (unsigned)(((size_t)n_frames + PL_GROUP - 1) / PL_GROUP);
    if (n > PL_SUB_LOG) {
        const size_t tiles = ((size_t)1 << n) / 64u;
        hipLaunchKernelGGL(pl_load<M>, dim3((unsigned)(groups * tiles)), dim3(256), 0, p->c.stream, m, n, n_frames, (const mem *)d_llr, (mem *)p->d_B);
        LAUNCHCHK();
    }
    if (p->rule == QLDPC_POLAR_SSC) {
        switch (n) {
        case 1: pl_launch_ssc<M, 1, true>(p, m, n_frames, groups, d_llr, d_frozen_u, want_u); break;
        case 2: pl_launch_ssc<M, 2, true>(p, m, n_frames, groups, d_llr, d_frozen_u, want_u); break;
        case 3: pl_launch_ssc<M, 3, true>(p, m, n_frames, groups, d_llr, d_frozen_u, want_u); break;
        case 4: pl_launch_ssc<M, 4, true>(p, m, n_frames, groups, d_llr, d_frozen_u, want_u); break;
        case 5: pl_launch_ssc<M, 5, true>(p, m, n_frames, groups, d_llr, d_frozen_u, want_u); break;
        default: pl_launch_ssc<M, 5, false>(p, m, n_frames, groups, d_llr, d_frozen_u, want_u); break;
        }
        LAUNCHCHK();
        return QLDPC_OK;
    }
    switch (n) {
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
template <class M>
static int plw_run_decode(const qldpc_polar *p, M m, int n_frames, const void *d_llr, const uint32_t *d_frozen_u, uint32_t *d_u, uint32_t *d_info,
                          uint32_t *d_x, void *d_leaf)
{
    typedef typename M::mem mem;
    const int n = p->c.n;
    const size_t lds = sizeof(mem) * plw_lds_elems(n, p->chip);
    plw_with_lanes(p->lanes, [&](auto lanes) {
        hipLaunchKernelGGL((plw_decode<M, decltype(lanes)::value>), dim3((unsigned)n_frames), dim3(decltype(lanes)::value), lds, p->c.stream, m, n, plw_chip(n, p->chip),
                           p->leaf_lanes, (const mem *)d_llr, (const uint32_t *)p->c.d_fmask, d_frozen_u, (mem *)p->d_B, p->d_U, p->d_X, d_u, d_x, d_info, p->c.n_info,
                           (const int *)p->c.d_info_pos, (mem *)d_leaf);
    });
    LAUNCHCHK();
    return QLDPC_OK;
}

/* the rows the caller asked for of a lanes decode, from the scratch */
static int pl_run_outputs(const qldpc_polar *p, int n_frames, uint32_t *d_u, uint32_t *d_info, uint32_t *d_x)
{
    if (d_u || d_info || d_x) {
        const size_t groups = ((size_t)n_frames + PL_GROUP - 1) / PL_GROUP, threads = groups * p->c.W * PL_GROUP;
        hipLaunchKernelGGL(pl_outputs, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, p->c.stream, p->c.n, n_frames, p->c.n_info, (const int *)p->c.d_info_pos,
                           (const uint32_t *)p->d_U, (const uint32_t *)p->d_X, d_u, d_info, d_x);
        LAUNCHCHK();
    }
    return QLDPC_OK;
}

extern "C" int qldpc_polar_decode_dev(qldpc_polar *p, int n_frames, const void *d_llr, const uint32_t *d_frozen_u, uint32_t *d_u, uint32_t *d_info,
                                      uint32_t *d_x, void *d_leaf)
{
    int rc = pl_ctx_check_frames(PL_CTX(p), n_frames, "polar_decode_dev");
    if (rc || n_frames == 0) return rc;
    if (!d_llr) { qldpc_set_error("polar_decode_dev: d_llr is NULL"); return QLDPC_EINVAL; }
    if (p->rule == QLDPC_POLAR_SSC && d_leaf) {
        qldpc_set_error("polar_decode_dev: the SSC rule has no leaf output (a pruned node never forms its leaf beliefs): create a QLDPC_POLAR_SC context for it");
        return QLDPC_EUNSUPPORTED;
    }
    HIPCHK(hipSetDevice(p->c.device));
    if (p->wide) return pl_with_messages(&p->c, [&](auto m) { return plw_run_decode(p, m, n_frames, d_llr, d_frozen_u, d_u, d_info, d_x, d_leaf); });
    rc = pl_with_messages(&p->c, [&](auto m) { return pl_run_decode(p, m, n_frames, d_llr, d_frozen_u, d_leaf, d_u || d_info); });
    if (rc) return rc;
    return pl_run_outputs(p, n_frames, d_u, d_info, d_x);
}

template <class M, int SL, bool TOP>
static void pl_launch_rows(const qldpc_polar *p, M m, int n_frames, unsigned groups, const void *d_llr, const uint32_t *d_frozen_u, const uint32_t *d_frozen_rows,
                           void *d_leaf)
{
    typedef typename M::mem mem;
    hipLaunchKernelGGL((pl_decode_rows<M, SL, TOP>), dim3(groups), dim3(PL_GROUP), 0, p->c.stream, m, p->c.n, n_frames, (const mem *)d_llr,
                       (const uint32_t *)p->c.d_fmask, d_frozen_u, d_frozen_rows, (mem *)p->d_B, p->d_U, p->d_X, (mem *)d_leaf);
}

template <class M>
static int pl_run_rows(const qldpc_polar *p, M m, int n_frames, const void *d_llr, const uint32_t *d_frozen_u, const uint32_t *d_frozen_rows, void *d_leaf)
{
    typedef typename M::mem mem;
    const int n = p->c.n;
    const unsigned groups = (unsigned)(((size_t)n_frames + PL_GROUP - 1) / PL_GROUP);
    if (n > PL_SUB_LOG) {
        const size_t tiles = ((size_t)1 << n) / 64u;
        hipLaunchKernelGGL(pl_load<M>, dim3((unsigned)(groups * tiles)), dim3(256), 0, p->c.stream, m, n, n_frames, (const mem *)d_llr, (mem *)p->d_B);
        LAUNCHCHK();
    }
    switch (n) {
    case 1: pl_launch_rows<M, 1, true>(p, m, n_frames, groups, d_llr, d_frozen_u, d_frozen_rows, d_leaf); break;
    case 2: pl_launch_rows<M, 2, true>(p, m, n_frames, groups, d_llr, d_frozen_u, d_frozen_rows, d_leaf); break;
    case 3: pl_launch_rows<M, 3, true>(p, m, n_frames, groups, d_llr, d_frozen_u, d_frozen_rows, d_leaf); break;
    case 4: pl_launch_rows<M, 4, true>(p, m, n_frames, groups, d_llr, d_frozen_u, d_frozen_rows, d_leaf); break;
    case 5: pl_launch_rows<M, 5, true>(p, m, n_frames, groups, d_llr, d_frozen_u, d_frozen_rows, d_leaf); break;
    default: pl_launch_rows<M, 5, false>(p, m, n_frames, groups, d_llr, d_frozen_u, d_frozen_rows, d_leaf); break;
    }
    LAUNCHCHK();
    return QLDPC_OK;
}

extern "C" int qldpc_polar_decode_rows_dev(qldpc_polar *p, int n_frames, const void *d_llr, const uint32_t *d_frozen_u, const uint32_t *d_frozen_rows,
                                           uint32_t *d_u, uint32_t *d_info, uint32_t *d_x, void *d_leaf)
{
    int rc = pl_ctx_check_frames(PL_CTX(p), n_frames, "polar_decode_rows_dev");
    if (rc) return rc;
    if (p->wide) {
        qldpc_set_error("polar_decode_rows_dev: the rows decode has no wide form: create a QLDPC_POLAR_LANES context of the same size and messages for it");
        return QLDPC_EUNSUPPORTED;
    }
    if (p->rule == QLDPC_POLAR_SSC) {
        qldpc_set_error("polar_decode_rows_dev: the rows decode has no SSC rule (the plan of pruned nodes belongs to the code, not to a frame): create a QLDPC_POLAR_SC context for it");
        return QLDPC_EUNSUPPORTED;
    }
    if (n_frames == 0) return QLDPC_OK;
    if (!d_llr || !d_frozen_rows) { qldpc_set_error("polar_decode_rows_dev: NULL device pointer (d_llr and d_frozen_rows are required)"); return QLDPC_EINVAL; }
    HIPCHK(hipSetDevice(p->c.device));
    rc = pl_with_messages(&p->c, [&](auto m) { return pl_run_rows(p, m, n_frames, d_llr, d_frozen_u, d_frozen_rows, d_leaf); });
    if (rc) return rc;
    return pl_run_outputs(p, n_frames, d_u, d_info, d_x);
}

template <class M, int SL, bool TOP>
static void pl_launch_tally(const qldpc_polar *p, M m, int n_frames, unsigned groups, const void *d_llr, const uint32_t *d_u_true, uint64_t *d_tally)
{
    typedef typename M::mem mem;
    hipLaunchKernelGGL((pl_tally<M, SL, TOP>), dim3(groups), dim3(PL_GROUP), 0, p->c.stream, m, p->c.n, n_frames, (const mem *)d_llr, d_u_true, (mem *)p->d_B, p->d_X,
                       (unsigned long long *)d_tally);
}

template <class M>
static int pl_run_tally(const qldpc_polar *p, M m, int n_frames, const void *d_llr, const uint32_t *d_u_true, uint64_t *d_tally)
{
    typedef typename M::mem mem;
    const int n = p->c.n;
    const unsigned groups = (unsigned)(((size_t)n_frames + PL_GROUP - 1) / PL_GROUP);
    if (n > PL_SUB_LOG) {
        const size_t tiles = ((size_t)1 << n) / 64u;
        hipLaunchKernelGGL(pl_load<M>, dim3((unsigned)(groups * tiles)), dim3(256), 0, p->c.stream, m, n, n_frames, (const mem *)d_llr, (mem *)p->d_B);
        LAUNCHCHK();
    }
    switch (n) {
    case 1: pl_launch_tally<M, 1, true>(p, m, n_frames, groups, d_llr, d_u_true, d_tally); break;
    case 2: pl_launch_tally<M, 2, true>(p, m, n_frames, groups, d_llr, d_u_true, d_tally); break;
    case 3: pl_launch_tally<M, 3, true>(p, m, n_frames, groups, d_llr, d_u_true, d_tally); break;
    case 4: pl_launch_tally<M, 4, true>(p, m, n_frames, groups, d_llr, d_u_true, d_tally); break;
    case 5: pl_launch_tally<M, 5, true>(p, m, n_frames, groups, d_llr, d_u_true, d_tally); break;
    default: pl_launch_tally<M, 5, false>(p, m, n_frames, groups, d_llr, d_u_true, d_tally); break;
    }
    LAUNCHCHK();
    return QLDPC_OK;
}

extern "C" int qldpc_polar_tally_dev(qldpc_polar *p, int n_frames, const void *d_llr, const uint32_t *d_u_true, uint64_t *d_tally)
{
    const int rc = pl_ctx_check_frames(PL_CTX(p), n_frames, "polar_tally_dev");
    if (rc) return rc;
    if (p->wide) {
        qldpc_set_error("polar_tally_dev: the tally has no wide form: create a QLDPC_POLAR_LANES context of the same size and messages for it");
        return QLDPC_EUNSUPPORTED;
    }
    if (n_frames == 0) return QLDPC_OK;
    if (!d_llr || !d_u_true || !d_tally) { qldpc_set_error("polar_tally_dev: NULL device pointer (d_llr, d_u_true and d_tally are required)"); return QLDPC_EINVAL; }
    HIPCHK(hipSetDevice(p->c.device));
    return pl_with_messages(&p->c, [&](auto m) { return pl_run_tally(p, m, n_frames, d_llr, d_u_true, d_tally); });
}
