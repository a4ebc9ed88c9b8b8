/*
 * qldpc_hashbatch.h -- the staging of a batch context of the privacy-amplification hashes (qldpc_privamp_ctx and qldpc_toeplitz_ctx embed one)
 * and the two forms of a call, HIP host code over the layout of qldpc_hashbatch_core.h.  A call writes `head` words of its own at the front
 * of h_in (descriptor rows: the layout's rows[] turned into what its kernel reads) and, in the host form, the packed rows of its blocks behind.
 *
 * THE REUSE RULE.  h_in, d_in and rows[] belong to one call at a time.  `done` is recorded behind everything a call queued, on the stream it
 * queued it on (the context's for the host form, the caller's for the device form), and hb_begin waits for it before the next call writes
 * a word: a device-form call returns while its kernels still read d_in.  A call that fails at its launch records nothing, so `done` still
 * stands for the call before it.
 */
#ifndef QLDPC_HASHBATCH_H
#define QLDPC_HASHBATCH_H

#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

#include "qldpc_hashbatch_core.h"
#include "qldpc_hip.h"
#include "qldpc_devmem.h"

struct hb_stage {
    int device;
    hb_limits lim;
    size_t in_words;               /* head and packed payload of a full call */
    uint32_t *h_in, *d_in, *h_out, *d_out;
    hb_row *rows;                  /* max_blocks: the layout of the call being made */
    hipStream_t stream;            /* of the host form */
    hipEvent_t done;               /* the reuse rule */
    dm_ledger mem;                 /* the staging and what else the context allocates (qldpc_devmem.h) */
};

static inline void hb_free(hb_stage *st)
{
    if (!st->lim.max_blocks) return;                             /* hb_create refused before it allocated anything */
    (void)hipSetDevice(st->device);
    if (st->done) { (void)hipEventSynchronize(st->done); (void)hipEventDestroy(st->done); }
    if (st->stream) (void)hipStreamDestroy(st->stream);
    dm_free_all(&st->mem);
    free(st->rows);
}

/* limits and device checked, then everything allocated; head_words, extra_words: of one block of the largest sizes.  hb_free also frees a stage that failed half way */
static inline int hb_create(hb_stage *st, int device, const hb_limits *lim, size_t head_words, size_t extra_words, const char *who, const hb_names *nm)
{
    int rc = hb_limits_check(lim, extra_words, who, nm), ndev = 0;
    if (rc) return rc;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { qldpc_set_error("no HIP device visible: libqldpc has no CPU fallback"); return QLDPC_ENODEV; }
    if (device < 0 || device >= ndev) return QLDPC_ENODEV;
    st->device = device; st->lim = *lim;
    HIPCHK(hipSetDevice(device));
    const size_t blocks = (size_t)lim->max_blocks, out_cap = blocks * hb_words(lim->max_out_bits), out_words = out_cap ? out_cap : 1;
    st->in_words = blocks * (head_words + hb_words(lim->max_key_bits) + extra_words);
    st->rows = (hb_row *)malloc(sizeof(hb_row) * blocks);
    if (!st->rows) return QLDPC_ENOMEM;
    if ((rc = dm_alloc_pinned(&st->mem, &st->h_in, st->in_words)) || (rc = dm_alloc_pinned(&st->mem, &st->h_out, out_words)) ||
        (rc = dm_alloc(&st->mem, &st->d_in, st->in_words)) || (rc = dm_alloc(&st->mem, &st->d_out, out_words))) return rc;
    HIPCHK(hipStreamCreateWithFlags(&st->stream, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&st->done, hipEventDisableTiming));
    HIPCHK(hipEventRecord(st->done, st->stream));
    return QLDPC_OK;
}

/* the first step of a call that has passed its checks: from here on the staging is this call's */
static inline int hb_begin(hb_stage *st)
{
    HIPCHK(hipSetDevice(st->device));
    HIPCHK(hipEventSynchronize(st->done));
    return QLDPC_OK;
}

/* host form: the key rows packed at `keys` (in h_in), up_words up, launch(stream), down_words down, all waited for, the output rows back to the caller */
template <class Launch>
static inline int hb_run_host(hb_stage *st, int n, const uint32_t *const *key_words, uint32_t *keys, size_t up_words, size_t down_words, uint32_t *const *out_words, Launch launch)
{
    const hb_row *r = st->rows;
    for (int i = 0; i < n; i++) memcpy(keys + r[i].key_off, key_words[i], 4 * (size_t)r[i].key_words);
    HIPCHK(hipMemcpyAsync(st->d_in, st->h_in, 4 * up_words, hipMemcpyHostToDevice, st->stream));
    const int rc = launch(st->stream);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(st->h_out, st->d_out, 4 * down_words, hipMemcpyDeviceToHost, st->stream));
    HIPCHK(hipEventRecord(st->done, st->stream));
    HIPCHK(hipStreamSynchronize(st->stream));
    for (int i = 0; i < n; i++)
        if (r[i].out_words) memcpy(out_words[i], st->h_out + r[i].out_off, 4 * (size_t)r[i].out_words);
    return QLDPC_OK;
}

/* device form on the caller's stream; head_words 0: the launch uploads what its kernels read itself */
template <class Launch>
static inline int hb_run_dev(hb_stage *st, size_t head_words, hipStream_t s, Launch launch)
{
    if (head_words) HIPCHK(hipMemcpyAsync(st->d_in, st->h_in, 4 * head_words, hipMemcpyHostToDevice, s));
    const int rc = launch(s);
    if (rc) return rc;
    HIPCHK(hipEventRecord(st->done, s));
    return QLDPC_OK;
}

#endif /* QLDPC_HASHBATCH_H */
