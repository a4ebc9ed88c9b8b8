/*
 * qldpc_polar_ctx.h -- what the device contexts of the polar subsystem (qldpc_polar and qldpc_polar_list embed one pl_ctx) have in common, HIP
 * host code: the code and where it lives on the device, the ledger of what a context allocated (qldpc_devmem.h), the checks of a call, the encode launch and the
 * choice of the message type.  A context owns everything a call touches; a call allocates nothing and waits for nothing.
 */
#ifndef QLDPC_POLAR_CTX_H
#define QLDPC_POLAR_CTX_H

#include <hip/hip_runtime.h>

#include <cstdlib>

#include "qldpc_hip.h"
#include "qldpc_devmem.h"
#include "qldpc_kernels_polar.h"
#include "qldpc_polar_int.h"

struct pl_ctx {
    int n, n_info, messages, maxq, max_frames, device;
    size_t W, groups;              /* words of a row, and ceil(max_frames / 64) */
    hipStream_t stream;
    uint32_t *d_fmask;             /* W words: 1 = frozen */
    int *d_info_pos;
    dm_ledger mem;                 /* every device allocation of the context, its owner's included */
    bool alloc_failed;             /* an allocation failed; the ones after it are not tried, and the owner reports it once */
};
#define PL_CTX(p) ((p) ? &(p)->c : nullptr)

/* for the Monte-Carlo loop (qldpc_polar_mc.hip) and the sessions (qldpc_polar_recon.hip), which run around a context they do not own: the
   context's pl_ctx, whether an SC context decodes in the wide form, its rule, and a list decoder's CRC.  Defined beside the two structs, in
   qldpc_polar.hip and qldpc_polar_list.hip */
const pl_ctx *pl_ctx_of_sc(const qldpc_polar *p);
bool pl_sc_is_wide(const qldpc_polar *p);
int pl_sc_rule(const qldpc_polar *p);
const pl_ctx *pl_ctx_of_list(const qldpc_polar_list *p, int *crc_len, uint32_t *crc_poly);

/* the only allocation of a context: `bytes` at *q (left NULL for 0 bytes), in the ledger; alloc_failed around dm_alloc */
template <class T> static inline void pl_ctx_alloc(pl_ctx *c, T **q, size_t bytes)
{
    unsigned char *d = nullptr;
    if (c->alloc_failed) return;
    if (dm_alloc(&c->mem, &d, bytes)) c->alloc_failed = true;
    else if (d) *q = (T *)d;
}

static inline void pl_ctx_free(pl_ctx *c)
{
    if (c->mem.blocks.empty()) return;                           /* pl_ctx_create refused before it allocated anything */
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);                       /* the last call may still read the scratch */
    dm_free_all(&c->mem);
}

/* the device checked, then the frozen mask and info_pos of the code (n, n_info, W set) allocated and sent up */
static inline int pl_ctx_upload(pl_ctx *c, int device, const uint32_t *mask, const int *info_pos)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { qldpc_set_error("no HIP device visible: libqldpc has no CPU fallback"); return QLDPC_ENODEV; }
    if (device < 0 || device >= ndev) { qldpc_set_error("device %d out of range", device); return QLDPC_ENODEV; }
    HIPCHK(hipSetDevice(device));
    c->device = device;
    pl_ctx_alloc(c, &c->d_fmask, sizeof(uint32_t) * c->W);
    pl_ctx_alloc(c, &c->d_info_pos, sizeof(int) * (size_t)(c->n_info > 0 ? c->n_info : 1));
    if (c->alloc_failed) return QLDPC_OK;
    HIPCHK(hipMemcpy(c->d_fmask, mask, sizeof(uint32_t) * c->W, hipMemcpyHostToDevice));
    if (c->n_info > 0) HIPCHK(hipMemcpy(c->d_info_pos, info_pos, sizeof(int) * (size_t)c->n_info, hipMemcpyHostToDevice));
    return QLDPC_OK;
}

/* The create step.  Every argument check comes before the first HIP call: the code's scalars (qldpc_polar_int.h), more(0), max_frames, the
   frozen mask, more(1); more() makes the owner's own checks, where they have always stood.  Then pl_ctx_upload.  An allocation that fails sets
   alloc_failed and nothing else: the owner allocates what it needs next and reports both in its own words.  pl_ctx_free also frees a context
   that failed half way. */
template <class More>
static inline int pl_ctx_create(pl_ctx *c, const char *who, int log2_n, int max_log2_n, int n_info, const int *info_pos, int messages, int maxq, int max_frames,
                                int device, More more)
{
    uint32_t *mask = nullptr;
    int rc = pl_args_scalars(who, log2_n, max_log2_n, messages, maxq);
    if (!rc) rc = more(0);
    if (rc) return rc;
    if (max_frames < 1 || max_frames > (1 << 24)) { qldpc_set_error("%s: max_frames=%d (1 .. %d)", who, max_frames, 1 << 24); return QLDPC_EINVAL; }
    rc = pl_args_frozen_mask(who, log2_n, n_info, info_pos, &mask);
    if (rc) return rc;
    rc = more(1);
    if (!rc) {
        c->n = log2_n; c->n_info = n_info; c->messages = messages; c->maxq = maxq; c->max_frames = max_frames;
        c->W = (size_t)pl_words(log2_n); c->groups = ((size_t)max_frames + PL_GROUP - 1) / PL_GROUP;
        rc = pl_ctx_upload(c, device, mask, info_pos);
    }
    free(mask);
    return rc;
}

static inline size_t pl_ctx_device_bytes(const pl_ctx *c) { return c ? c->mem.dev_bytes : 0; }

static inline int pl_ctx_set_stream(pl_ctx *c, void *hip_stream)
{
    if (!c) return QLDPC_EINVAL;
    HIPCHK(hipSetDevice(c->device));
    return qldpc_stream_switch(&c->stream, hip_stream);
}

static inline int pl_ctx_check_frames(const pl_ctx *c, int n_frames, const char *who)
{
    if (!c) return QLDPC_EINVAL;
    if (n_frames < 0) { qldpc_set_error("%s: n_frames=%d is negative", who, n_frames); return QLDPC_EINVAL; }
    if (n_frames > c->max_frames) { qldpc_set_error("%s: n_frames=%d exceeds the context's max_frames=%d: create it larger or split the call", who, n_frames, c->max_frames); return QLDPC_ESIZE; }
    return QLDPC_OK;
}

/* x = encode(u) of `rows` rows of 2^n bits, in place allowed: the stages inside a tile, then those above it where a row has more than one */
static inline int pl_launch_encode(hipStream_t stream, int n, size_t rows, const uint32_t *d_u, uint32_t *d_x)
{
    const size_t W = (size_t)pl_words(n), tiles = W > PL_ENC_TILE ? W / PL_ENC_TILE : 1;
    hipLaunchKernelGGL(pl_encode_tiles, dim3((unsigned)(rows * tiles)), dim3(PL_ENC_LANES), 0, stream, n, d_u, d_x);
    LAUNCHCHK();
    if (tiles > 1) {
        hipLaunchKernelGGL(pl_encode_columns, dim3((unsigned)(rows * PL_ENC_TILE / PL_ENC_LANES)), dim3(PL_ENC_LANES), 0, stream, n, (int)rows, d_x);
        LAUNCHCHK();
    }
    return QLDPC_OK;
}

/* fn(m), m the context's message type: pl_msg_i8 with its maxq, or pl_msg_f32 */
template <class Fn> static inline int pl_with_messages(const pl_ctx *c, Fn fn)
{
    return c->messages == QLDPC_POLAR_I8 ? fn(pl_msg_i8{c->maxq}) : fn(pl_msg_f32{});
}

#endif /* QLDPC_POLAR_CTX_H */
