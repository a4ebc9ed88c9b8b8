/*
 * qldpc_polar_recon.hip -- the session object and the launches of qldpc_polar_recon_*: polar reconciliation around an existing qldpc_polar context
 * (any form, any rule) or an existing qldpc_polar_list context with a CRC.
 *
 *     Alice   mask -> the context's encode launch -> syndrome and crc
 *     Bob     prior and frozen row -> the context's own decode -> verdict
 *
 * The rule is qldpc_polar_recon_core.h's, the kernels qldpc_kernels_polar_recon.h's, the mirrors and the shared argument checks
 * qldpc_polar_recon_host.c's.  Everything is queued on the context's stream; nothing crosses the host and no call waits for anything.
 *
 * The session owns, in a ledger of its own, the rows of a call (LLRs, frozen, x, info, pick) and the two tables the context does not have (the
 * frozen positions in order and the prefix popcounts of the frozen mask), all allocated by create: no call allocates anything.  The frozen mask
 * and info_pos are the context's, which is not owned and must outlive the session.
 *
 * A session made by qldpc_polar_recon_create_ladder (SC contexts of the lanes form) also owns a ladder (qldpc_polar_ladder_core.h): its positions
 * and their rank table, the added-flag rows of a round, two open lists and their two counters.  qldpc_polar_recon_decode_rounds runs
 *
 *     entry -> per round: read the open count back | slot prior -> the rows form of the SC decode -> slot verdict and the next round's list
 *
 * with the kernels of qldpc_kernels_polar_ladder.h.  The grid of a round needs the open count on the host: one 4-byte read-back per round, queued
 * on the context's stream and waited for on that stream alone.
 *
 * A session made by qldpc_polar_recon_create_flip is a ladder session (n_extra = 0 is the common case) that also owns the scratch of SC-Flip trials
 * (qldpc_polar_flip_core.h): the leaf rows of a chunk's probe and the flip positions of its trials.  qldpc_polar_recon_decode_flip runs
 *
 *     first pass (or the entry of a resumed call) -> read the open count back | per chunk of C = max_blocks / T open blocks:
 *     slot prior -> probe (rows decode with the leaf output) -> select -> trial prior on C T slots -> rows decode -> settle
 *
 * with the kernels of qldpc_kernels_polar_flip.h.  The trials live in the rows a call's blocks live in (LLR, frozen, flags, info, x), which is why
 * a chunk holds max_blocks / T blocks.  One 4-byte read-back, the call's only wait; after it everything is queued.  These two are the calls of a
 * session that wait.
 */
#include <hip/hip_runtime.h>

#include <cstdint>
#include <new>
#include <vector>

#include "qldpc_kernels_polar_flip.h"
#include "qldpc_kernels_polar_ladder.h"
#include "qldpc_kernels_polar_recon.h"
#include "qldpc_polar_ctx.h"
#include "qldpc_polar_recon_int.h"

struct qldpc_polar_recon {
    qldpc_polar *sc;
    qldpc_polar_list *list;
    const pl_ctx *c;               /* of the one that is given */
    int crc_len, n_frozen, max_blocks;
    uint32_t crc_poly;
    int prior_i, pin_i;            /* the levels: the integers of an int8 context, the floats of a float one */
    float prior_f, pin_f;
    size_t Wf, Wi;                 /* words of a syndrome row and of an info row */
    int *d_fpos, *d_fprefix;
    uint32_t *d_frozen, *d_x, *d_info;
    int32_t *d_pick;
    void *d_llr;
    bool has_ladder;               /* made by _create_ladder: what follows is set */
    int n_extra;
    size_t We;                     /* words of Alice's extra row */
    int *d_extra_pos, *d_rank;     /* the ladder [n_extra] and its rank table [N] */
    uint32_t *d_flags;             /* the added frozen flags of a round's slots, max_blocks x W */
    int *d_open, *d_count;         /* two open lists of max_blocks blocks and their two counters: round t fills those of round t + 1 */
    int h_open;                    /* where a round's count is read back to */
    int max_flips;                 /* made by _create_flip (0 otherwise): what follows is set */
    void *d_leaf;                  /* the leaf rows of a chunk's probe, max_blocks x N: a chunk of n_flips = 1 holds max_blocks blocks */
    int *d_pos;                    /* the flips of a chunk's trials, (max_blocks / T) x T <= max_blocks entries */
    dm_ledger mem;                 /* everything create allocates (qldpc_devmem.h) */
};

extern "C" void qldpc_polar_recon_free(qldpc_polar_recon *r)
{
    if (!r) return;
    if (!r->mem.blocks.empty()) {
        (void)hipSetDevice(r->c->device);
        (void)hipStreamSynchronize(r->c->stream);                /* the last call may still read the rows */
    }
    dm_free_all(&r->mem);
    delete r;
}

template <class T> static int prc_alloc(qldpc_polar_recon *r, T **q, size_t count)
{
    if (count == 0) count = 1;                                   /* an empty array still gets one element */
    const int rc = dm_alloc(&r->mem, q, count);
    if (rc) qldpc_set_error("polar_recon_create: device allocation of %zu bytes failed: lower max_blocks", sizeof(T) * count);
    return rc;
}

static int prc_build(qldpc_polar_recon *r)
{
    const pl_ctx *c = r->c;
    const size_t B = (size_t)r->max_blocks, N = (size_t)1 << c->n, esz = c->messages == QLDPC_POLAR_I8 ? 1 : sizeof(float);
    int rc;
    HIPCHK(hipSetDevice(c->device));
    if ((rc = prc_alloc(r, &r->d_fpos, (size_t)r->n_frozen)) || (rc = prc_alloc(r, &r->d_fprefix, c->W)) || (rc = prc_alloc(r, (uint8_t **)&r->d_llr, esz * B * N)) ||
        (rc = prc_alloc(r, &r->d_frozen, B * c->W)) || (rc = prc_alloc(r, &r->d_x, B * c->W)) || (rc = prc_alloc(r, &r->d_info, B * r->Wi)) ||
        (rc = prc_alloc(r, &r->d_pick, B)))
        return rc;
    /* the two tables from the context's own frozen mask */
    std::vector<uint32_t> mask(c->W);
    std::vector<int> fpos((size_t)r->n_frozen + 1), prefix(c->W);
    HIPCHK(hipMemcpy(mask.data(), c->d_fmask, sizeof(uint32_t) * c->W, hipMemcpyDeviceToHost));
    if (prc_tables(c->n, mask.data(), prefix.data(), fpos.data()) != r->n_frozen) { qldpc_set_error("polar_recon_create: the context's frozen mask does not hold N - K positions"); return QLDPC_ESTATE; }
    HIPCHK(hipMemcpy(r->d_fprefix, prefix.data(), sizeof(int) * c->W, hipMemcpyHostToDevice));
    if (r->n_frozen) HIPCHK(hipMemcpy(r->d_fpos, fpos.data(), sizeof(int) * (size_t)r->n_frozen, hipMemcpyHostToDevice));
    return QLDPC_OK;
}

extern "C" int qldpc_polar_recon_create(qldpc_polar *sc, qldpc_polar_list *list, int crc_len, uint32_t crc_poly, double prior, double pin, int max_blocks,
                                        qldpc_polar_recon **out)
{
    const char *who = "polar_recon_create";
    if (!out) return QLDPC_EINVAL;
    *out = nullptr;
    if ((sc != nullptr) == (list != nullptr)) { qldpc_set_error("%s: exactly one of an SC context and a list context is required", who); return QLDPC_EINVAL; }
    int list_len = 0, rc;
    uint32_t list_poly = 0u;
    const pl_ctx *c = sc ? pl_ctx_of_sc(sc) : pl_ctx_of_list(list, &list_len, &list_poly);
    if (list) {
        if (crc_len || crc_poly) { qldpc_set_error("%s: with a list context the CRC is the context's: crc_len and crc_poly must be 0", who); return QLDPC_EINVAL; }
        if (list_len == 0) { qldpc_set_error("%s: the list context has no CRC: a session has no verdict without one", who); return QLDPC_EINVAL; }
        crc_len = list_len; crc_poly = list_poly;
    } else if ((rc = prc_args_crc(who, crc_len, crc_poly, c->n_info)))
        return rc;
    if (max_blocks < 0 || max_blocks > c->max_frames) {
        qldpc_set_error("%s: max_blocks=%d (0: the context's max_frames = %d, or 1 .. that)", who, max_blocks, c->max_frames);
        return max_blocks < 0 ? QLDPC_EINVAL : QLDPC_ESIZE;
    }
    if (max_blocks == 0) max_blocks = c->max_frames;
    qldpc_polar_recon *r = new (std::nothrow) qldpc_polar_recon();
    if (!r) return QLDPC_ENOMEM;
    if ((rc = prc_args_levels(who, c->messages, c->maxq, prior, pin, &r->prior_i, &r->pin_i, &r->prior_f, &r->pin_f))) { delete r; return rc; }
    r->sc = sc; r->list = list; r->c = c;
    r->crc_len = crc_len; r->crc_poly = crc_poly; r->max_blocks = max_blocks;
    r->n_frozen = (1 << c->n) - c->n_info; r->Wf = pmc_words(r->n_frozen); r->Wi = pmc_words(c->n_info);
    if ((rc = prc_build(r))) { qldpc_polar_recon_free(r); return rc; }
    *out = r;
    return QLDPC_OK;
}

extern "C" size_t qldpc_polar_recon_device_bytes(const qldpc_polar_recon *r) { return r ? r->mem.dev_bytes : 0; }
extern "C" int qldpc_polar_recon_syndrome_words(const qldpc_polar_recon *r) { return r ? (int)r->Wf : QLDPC_EINVAL; }
extern "C" int qldpc_polar_recon_leaked_bits(const qldpc_polar_recon *r) { return r ? r->n_frozen + r->crc_len : QLDPC_EINVAL; }

static unsigned prc_grid(size_t lanes, unsigned per) { return (unsigned)((lanes + per - 1) / per); }

static int prc_check_blocks(const qldpc_polar_recon *r, int n_blocks, const char *who)
{
    if (!r) return QLDPC_EINVAL;
    const int rc = prc_args_count(who, n_blocks);
    if (rc) return rc;
    if (n_blocks > r->max_blocks) { qldpc_set_error("%s: n_blocks=%d exceeds the session's max_blocks=%d: create it larger or split the call", who, n_blocks, r->max_blocks); return QLDPC_ESIZE; }
    return QLDPC_OK;
}

extern "C" int qldpc_polar_recon_encode_dev(qldpc_polar_recon *r, int n_blocks, const uint32_t *d_keys, const int *d_key_bits, uint32_t *d_syndrome, uint32_t *d_crc)
{
    const char *who = "polar_recon_encode_dev";
    int rc = prc_check_blocks(r, n_blocks, who);
    if (rc || n_blocks == 0) return rc;
    if (!d_keys || !d_crc || (r->n_frozen && !d_syndrome)) { qldpc_set_error("%s: NULL device pointer", who); return QLDPC_EINVAL; }
    const pl_ctx *c = r->c;
    const hipStream_t s = c->stream;
    const size_t nb = (size_t)n_blocks, total = nb * c->W;
    HIPCHK(hipSetDevice(c->device));
    hipLaunchKernelGGL(prc_mask, dim3(prc_grid(total, PRC_LANES)), dim3(PRC_LANES), 0, s, d_keys, d_key_bits, r->d_x, total, c->n, (unsigned)pl_ctz((long)c->W));
    LAUNCHCHK();
    if ((rc = pl_launch_encode(s, c->n, nb, r->d_x, r->d_x))) return rc;      /* the launch of qldpc_polar_encode_dev, in place: u */
    hipLaunchKernelGGL(prc_syndrome, dim3(prc_grid(nb, PRC_SYN_BLOCKS)), dim3(PRC_SYN_LANES), 0, s, (const uint32_t *)r->d_x, (const int *)r->d_fpos,
                       (const int *)c->d_info_pos, r->d_info, d_syndrome, d_crc, (unsigned)n_blocks, (unsigned)c->W, (unsigned)r->n_frozen, (unsigned)c->n_info, r->crc_len,
                       r->crc_poly);
    LAUNCHCHK();
    return QLDPC_OK;
}

/* the launch of the prior kernel: the caller has checked everything and set the device */
static int prc_launch_prior(hipStream_t s, int log2_n, int n_frozen, const uint32_t *d_fmask, const int *d_fprefix, bool i8, int pi, int qi, float pf, float qf,
                            int n_blocks, const uint32_t *d_keys, const int *d_key_bits, const uint32_t *d_syndrome, void *d_llr, uint32_t *d_frozen)
{
    const size_t total = (size_t)n_blocks * pmc_quads(log2_n);
    const unsigned W = (unsigned)pl_words(log2_n), Wf = pmc_words(n_frozen);
    if (i8)
        hipLaunchKernelGGL(prc_prior<int>, dim3(prc_grid(total, PRC_LANES)), dim3(PRC_LANES), 0, s, d_keys, d_key_bits, d_syndrome, d_fmask, d_fprefix, d_llr, d_frozen, total,
                           log2_n, W, Wf, pi, qi);
    else
        hipLaunchKernelGGL(prc_prior<float>, dim3(prc_grid(total, PRC_LANES)), dim3(PRC_LANES), 0, s, d_keys, d_key_bits, d_syndrome, d_fmask, d_fprefix, d_llr, d_frozen, total,
                           log2_n, W, Wf, pf, qf);
    LAUNCHCHK();
    return QLDPC_OK;
}

static int prc_launch_verdict(hipStream_t s, int log2_n, int n_info, int crc_len, uint32_t crc_poly, int n_blocks, const uint32_t *d_info, const uint32_t *d_x,
                              const int32_t *d_pick, uint32_t *d_keys, const int *d_key_bits, const uint32_t *d_crc, int *d_status, int *d_corrected)
{
    hipLaunchKernelGGL(prc_verdict, dim3(prc_grid((size_t)n_blocks, PRC_LANES)), dim3(PRC_LANES), 0, s, d_info, d_x, d_pick, d_keys, d_key_bits, d_crc, d_status, d_corrected,
                       (unsigned)n_blocks, log2_n, n_info, crc_len, crc_poly);
    LAUNCHCHK();
    return QLDPC_OK;
}

extern "C" int qldpc_polar_recon_decode_dev(qldpc_polar_recon *r, int n_blocks, uint32_t *d_keys, const int *d_key_bits, const uint32_t *d_syndrome,
                                            const uint32_t *d_crc, int *d_status, int *d_corrected, int32_t *d_pick)
{
    const char *who = "polar_recon_decode_dev";
    int rc = prc_check_blocks(r, n_blocks, who);
    if (rc) return rc;
    if (d_pick && !r->list) { qldpc_set_error("%s: d_pick is the list decoder's: this session wraps an SC context", who); return QLDPC_EINVAL; }
    if (n_blocks == 0) return QLDPC_OK;
    if (!d_keys || !d_crc || !d_status || (r->n_frozen && !d_syndrome)) { qldpc_set_error("%s: NULL device pointer", who); return QLDPC_EINVAL; }
    const pl_ctx *c = r->c;
    const hipStream_t s = c->stream;
    HIPCHK(hipSetDevice(c->device));
    if ((rc = prc_launch_prior(s, c->n, r->n_frozen, c->d_fmask, r->d_fprefix, c->messages == QLDPC_POLAR_I8, r->prior_i, r->pin_i, r->prior_f, r->pin_f, n_blocks, d_keys,
                               d_key_bits, d_syndrome, r->d_llr, r->d_frozen)))
        return rc;
    int32_t *pick = r->list ? (d_pick ? d_pick : r->d_pick) : nullptr;
    if (r->sc) rc = qldpc_polar_decode_dev(r->sc, n_blocks, r->d_llr, r->d_frozen, nullptr, r->d_info, r->d_x, nullptr);
    else rc = qldpc_polar_list_decode_dev(r->list, n_blocks, r->d_llr, r->d_frozen, d_crc, nullptr, r->d_info, r->d_x, pick, nullptr, nullptr);
    if (rc) return rc;
    return prc_launch_verdict(s, c->n, c->n_info, r->crc_len, r->crc_poly, n_blocks, r->d_info, r->d_x, pick, d_keys, d_key_bits, d_crc, d_status, d_corrected);
}

/* ---- the building blocks on their own: a stream and the code as device tables, no session; the current device is the caller's ---- */

extern "C" int qldpc_polar_recon_prior_dev(void *hip_stream, int log2_n, int n_frozen, const uint32_t *d_frozen_mask, const int *d_frozen_prefix, int messages, int maxq,
                                           double prior, double pin, int n_blocks, const uint32_t *d_keys, const int *d_key_bits, const uint32_t *d_syndrome, void *d_llr,
                                           uint32_t *d_frozen)
{
    const char *who = "polar_recon_prior_dev";
    int pi, qi;
    float pf, qf;
    int rc = pl_args_scalars(who, log2_n, PL_MAX_LOG2N, messages, maxq);
    if (!rc) rc = prc_args_levels(who, messages, maxq, prior, pin, &pi, &qi, &pf, &qf);
    if (!rc) rc = prc_args_count(who, n_blocks);
    if (rc) return rc;
    if (n_frozen < 0 || n_frozen > (1 << log2_n)) { qldpc_set_error("%s: n_frozen=%d (0 .. N = %d)", who, n_frozen, 1 << log2_n); return QLDPC_ESIZE; }
    if (n_blocks == 0) return QLDPC_OK;
    if (!d_frozen_mask || !d_frozen_prefix || !d_keys || !d_llr || !d_frozen || (n_frozen && !d_syndrome)) { qldpc_set_error("%s: NULL device pointer", who); return QLDPC_EINVAL; }
    return prc_launch_prior((hipStream_t)hip_stream, log2_n, n_frozen, d_frozen_mask, d_frozen_prefix, messages == QLDPC_POLAR_I8, pi, qi, pf, qf, n_blocks, d_keys, d_key_bits,
                            d_syndrome, d_llr, d_frozen);
}

extern "C" int qldpc_polar_recon_verdict_dev(void *hip_stream, int log2_n, int n_info, int crc_len, uint32_t crc_poly, int n_blocks, const uint32_t *d_info,
                                             const uint32_t *d_x, const int32_t *d_pick, uint32_t *d_keys, const int *d_key_bits, const uint32_t *d_crc, int *d_status,
                                             int *d_corrected)
{
    const int rc = prc_args_verdict("polar_recon_verdict_dev", log2_n, n_info, crc_len, crc_poly, n_blocks, d_info, d_x, d_pick, d_keys, d_crc, d_status);
    if (rc || n_blocks == 0) return rc;
    return prc_launch_verdict((hipStream_t)hip_stream, log2_n, n_info, crc_len, crc_poly, n_blocks, d_info, d_x, d_pick, d_keys, d_key_bits, d_crc, d_status, d_corrected);
}

/* ---- incremental freezing: a session with a ladder (qldpc_polar_ladder_core.h) ---- */

extern "C" int qldpc_polar_recon_create_ladder(qldpc_polar *sc, int crc_len, uint32_t crc_poly, double prior, double pin, int max_blocks, int n_extra,
                                               const int *extra_pos, qldpc_polar_recon **out)
{
    const char *who = "polar_recon_create_ladder";
    if (!out) return QLDPC_EINVAL;
    *out = nullptr;
    if (!sc) { qldpc_set_error("%s: an SC context is required (the list decoder has no rows form)", who); return QLDPC_EINVAL; }
    if (pl_sc_is_wide(sc) || pl_sc_rule(sc) != QLDPC_POLAR_SC) {
        qldpc_set_error("%s: the rows decode of a ladder session has neither a wide form nor an SSC rule (the SSC plan belongs to the code, not to a block): "
                        "create a QLDPC_POLAR_LANES context of the QLDPC_POLAR_SC rule for it", who);
        return QLDPC_EUNSUPPORTED;
    }
    const pl_ctx *c = pl_ctx_of_sc(sc);
    if (n_extra < 0 || n_extra > c->n_info) { qldpc_set_error("%s: n_extra=%d (0 .. n_info = %d)", who, n_extra, c->n_info); return QLDPC_ESIZE; }
    if (n_extra > 0 && !extra_pos) { qldpc_set_error("%s: extra_pos is NULL", who); return QLDPC_EINVAL; }
    qldpc_polar_recon *r = nullptr;
    int rc = qldpc_polar_recon_create(sc, nullptr, crc_len, crc_poly, prior, pin, max_blocks, &r);
    if (rc) return rc;
    const size_t N = (size_t)1 << c->n, B = (size_t)r->max_blocks;
    std::vector<uint32_t> mask(c->W);
    std::vector<int> rank(N);
    hipError_t e = hipMemcpy(mask.data(), c->d_fmask, sizeof(uint32_t) * c->W, hipMemcpyDeviceToHost);
    if (e != hipSuccess) { qldpc_set_error("%s: %s", who, hipGetErrorString(e)); rc = QLDPC_EHIP; }
    if (!rc) rc = pld_args_ladder(who, c->n, mask.data(), c->n_info, n_extra, extra_pos, rank.data());
    if (!rc && !((rc = prc_alloc(r, &r->d_extra_pos, (size_t)n_extra)) || (rc = prc_alloc(r, &r->d_rank, N)) || (rc = prc_alloc(r, &r->d_flags, B * c->W)) ||
                 (rc = prc_alloc(r, &r->d_open, 2 * B)) || (rc = prc_alloc(r, &r->d_count, (size_t)2)))) {
        e = hipMemcpy(r->d_rank, rank.data(), sizeof(int) * N, hipMemcpyHostToDevice);
        if (e == hipSuccess && n_extra) e = hipMemcpy(r->d_extra_pos, extra_pos, sizeof(int) * (size_t)n_extra, hipMemcpyHostToDevice);
        if (e != hipSuccess) { qldpc_set_error("%s: %s", who, hipGetErrorString(e)); rc = QLDPC_EHIP; }
    }
    if (rc) { qldpc_polar_recon_free(r); return rc; }
    r->has_ladder = true; r->n_extra = n_extra; r->We = pld_extra_words(n_extra);
    *out = r;
    return QLDPC_OK;
}

extern "C" int qldpc_polar_recon_extra_words(const qldpc_polar_recon *r) { return r ? (r->has_ladder ? (int)r->We : 0) : QLDPC_EINVAL; }

static int pld_check_ladder(const qldpc_polar_recon *r, const char *who)
{
    if (r->has_ladder) return QLDPC_OK;
    qldpc_set_error("%s: the session has no ladder: make it with qldpc_polar_recon_create_ladder", who);
    return QLDPC_ESTATE;
}

extern "C" int qldpc_polar_recon_encode_ladder_dev(qldpc_polar_recon *r, int n_blocks, const uint32_t *d_keys, const int *d_key_bits, uint32_t *d_syndrome,
                                                   uint32_t *d_crc, uint32_t *d_extra_bits)
{
    const char *who = "polar_recon_encode_ladder_dev";
    int rc = prc_check_blocks(r, n_blocks, who);
    if (!rc) rc = pld_check_ladder(r, who);
    if (rc || n_blocks == 0) return rc;
    if (r->n_extra && !d_extra_bits) { qldpc_set_error("%s: NULL device pointer (d_extra_bits)", who); return QLDPC_EINVAL; }
    if ((rc = qldpc_polar_recon_encode_dev(r, n_blocks, d_keys, d_key_bits, d_syndrome, d_crc))) return rc;      /* leaves u in the session's row */
    if (r->n_extra) {
        hipLaunchKernelGGL(pld_extra_rows, dim3(prc_grid((size_t)n_blocks, PRC_LANES / 64u)), dim3(PRC_LANES), 0, r->c->stream, (const uint32_t *)r->d_x,
                           (const int *)r->d_extra_pos, d_extra_bits, (unsigned)n_blocks, (unsigned)r->c->W, (unsigned)r->n_extra);
        LAUNCHCHK();
    }
    return QLDPC_OK;
}

/* the slot prior of a round: the open list's first n_open blocks into slots 0 .. n_open - 1 */
static int pld_launch_slot_prior(const qldpc_polar_recon *r, const int *d_open, int n_open, const uint32_t *d_keys, const int *d_key_bits, const uint32_t *d_syndrome,
                                 const uint32_t *d_extra_bits, const int *d_extra, int *d_decodes)
{
    const pl_ctx *c = r->c;
    const size_t total = (size_t)n_open * pmc_quads(c->n);
    if (c->messages == QLDPC_POLAR_I8)
        hipLaunchKernelGGL(pld_slot_prior<int>, dim3(prc_grid(total, PRC_LANES)), dim3(PRC_LANES), 0, c->stream, d_open, d_keys, d_key_bits, d_syndrome, d_extra_bits, d_extra,
                           (const uint32_t *)c->d_fmask, (const int *)r->d_fprefix, (const int *)r->d_rank, r->d_llr, r->d_frozen, r->d_flags, d_decodes, total, c->n,
                           (unsigned)c->W, (unsigned)r->Wf, (unsigned)r->We, r->prior_i, r->pin_i);
    else
        hipLaunchKernelGGL(pld_slot_prior<float>, dim3(prc_grid(total, PRC_LANES)), dim3(PRC_LANES), 0, c->stream, d_open, d_keys, d_key_bits, d_syndrome, d_extra_bits, d_extra,
                           (const uint32_t *)c->d_fmask, (const int *)r->d_fprefix, (const int *)r->d_rank, r->d_llr, r->d_frozen, r->d_flags, d_decodes, total, c->n,
                           (unsigned)c->W, (unsigned)r->Wf, (unsigned)r->We, r->prior_f, r->pin_f);
    LAUNCHCHK();
    return QLDPC_OK;
}

extern "C" int qldpc_polar_recon_decode_rounds(qldpc_polar_recon *r, int n_blocks, uint32_t *d_keys, const int *d_key_bits, const uint32_t *d_syndrome,
                                               const uint32_t *d_crc, const uint32_t *d_extra_bits, int *d_extra, int step, int max_rounds, int resume,
                                               int *d_status, int *d_corrected, int *d_decodes, int *open_per_round)
{
    const char *who = "polar_recon_decode_rounds";
    int rc = prc_check_blocks(r, n_blocks, who);
    if (!rc) rc = pld_args_rounds(who, step, max_rounds, resume);
    if (!rc) rc = pld_check_ladder(r, who);
    if (rc) return rc;
    if (n_blocks > 0 && (!d_keys || !d_crc || !d_status || !d_extra || (r->n_frozen && !d_syndrome) || (r->n_extra && !d_extra_bits))) {
        qldpc_set_error("%s: NULL device pointer (d_keys, d_crc, d_status and d_extra are required; d_syndrome where N > K, d_extra_bits where n_extra > 0)", who);
        return QLDPC_EINVAL;
    }
    for (int t = 0; open_per_round && t < max_rounds; t++) open_per_round[t] = 0;
    if (n_blocks == 0) return QLDPC_OK;
    const pl_ctx *c = r->c;
    const hipStream_t s = c->stream;
    const size_t B = (size_t)r->max_blocks;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemsetAsync(r->d_count, 0, 2 * sizeof(int), s));
    hipLaunchKernelGGL(pld_entry_blocks, dim3(prc_grid((size_t)n_blocks, PRC_LANES)), dim3(PRC_LANES), 0, s, d_key_bits, (const int *)d_extra, d_status, d_corrected, d_decodes,
                       r->d_open, r->d_count, (unsigned)n_blocks, c->n, r->n_extra, resume);
    LAUNCHCHK();
    for (int t = 0; t < max_rounds; t++) {
        const int cur = t & 1, nxt = cur ^ 1;
        HIPCHK(hipMemcpyAsync(&r->h_open, r->d_count + cur, sizeof(int), hipMemcpyDeviceToHost, s));      /* the ONE read-back of the round */
        HIPCHK(hipStreamSynchronize(s));
        const int n_open = r->h_open;
        if (n_open < 0 || n_open > n_blocks) { qldpc_set_error("%s: the open count %d of round %d is not in 0 .. n_blocks = %d", who, n_open, t, n_blocks); return QLDPC_ESTATE; }
        if (n_open == 0) break;
        if (open_per_round) open_per_round[t] = n_open;
        const int *open = r->d_open + (size_t)cur * B;
        HIPCHK(hipMemsetAsync(r->d_count + nxt, 0, sizeof(int), s));
        if ((rc = pld_launch_slot_prior(r, open, n_open, d_keys, d_key_bits, d_syndrome, d_extra_bits, d_extra, d_decodes))) return rc;
        if ((rc = qldpc_polar_decode_rows_dev(r->sc, n_open, r->d_llr, r->d_frozen, r->d_flags, nullptr, r->d_info, r->d_x, nullptr))) return rc;
        hipLaunchKernelGGL(pld_slot_verdict, dim3(prc_grid((size_t)n_open, PRC_LANES)), dim3(PRC_LANES), 0, s, open, (const uint32_t *)r->d_info, (const uint32_t *)r->d_x,
                           d_keys, d_key_bits, d_crc, d_extra, d_status, d_corrected, r->d_open + (size_t)nxt * B, r->d_count + nxt, (unsigned)n_open, c->n, c->n_info,
                           r->crc_len, r->crc_poly, r->n_extra, step, t, max_rounds);
        LAUNCHCHK();
    }
    return QLDPC_OK;
}

/* ---- SC-Flip trials: a ladder session with the scratch of the trials (qldpc_polar_flip_core.h) ---- */

extern "C" int qldpc_polar_recon_create_flip(qldpc_polar *sc, int crc_len, uint32_t crc_poly, double prior, double pin, int max_blocks, int n_extra,
                                             const int *extra_pos, int max_flips, qldpc_polar_recon **out)
{
    const char *who = "polar_recon_create_flip";
    if (!out) return QLDPC_EINVAL;
    *out = nullptr;
    if (!sc) { qldpc_set_error("%s: an SC context is required (the list decoder has no rows form)", who); return QLDPC_EINVAL; }
    if (max_flips > PFL_MAX_FLIPS || !pfl_flips_pow2(max_flips)) {
        qldpc_set_error("%s: max_flips=%d (a power of two in 1 .. %d)", who, max_flips, PFL_MAX_FLIPS);
        return QLDPC_EINVAL;
    }
    qldpc_polar_recon *r = nullptr;
    int rc = qldpc_polar_recon_create_ladder(sc, crc_len, crc_poly, prior, pin, max_blocks, n_extra, extra_pos, &r);
    if (rc) return rc;
    const pl_ctx *c = r->c;
    const size_t B = (size_t)r->max_blocks, N = (size_t)1 << c->n, esz = c->messages == QLDPC_POLAR_I8 ? 1 : sizeof(float);
    if (max_flips > r->max_blocks) {
        qldpc_set_error("%s: max_flips=%d exceeds max_blocks=%d: the trials of a block live in the rows of the call's blocks", who, max_flips, r->max_blocks);
        rc = QLDPC_ESIZE;
    }
    if (!rc && !((rc = prc_alloc(r, (uint8_t **)&r->d_leaf, esz * B * N)) || (rc = prc_alloc(r, &r->d_pos, B)))) r->max_flips = max_flips;
    if (rc) { qldpc_polar_recon_free(r); return rc; }
    *out = r;
    return QLDPC_OK;
}

extern "C" int qldpc_polar_recon_max_flips(const qldpc_polar_recon *r) { return r ? r->max_flips : QLDPC_EINVAL; }

/* the launch of the select kernel: the caller has checked everything and set the device */
static int pfl_launch_select(hipStream_t s, int log2_n, bool i8, int n_slots, const void *d_leaf, const uint32_t *d_fmask, const int *d_rank, const int *d_extra,
                             const int *d_open, int n_flips, int *d_pos)
{
    const dim3 grid(prc_grid((size_t)n_slots, PRC_LANES / 64u)), lanes(PRC_LANES);
    if (i8) hipLaunchKernelGGL(pfl_select<int8_t>, grid, lanes, 0, s, (const int8_t *)d_leaf, d_fmask, d_rank, d_extra, d_open, d_pos, (unsigned)n_slots, log2_n, n_flips);
    else hipLaunchKernelGGL(pfl_select<float>, grid, lanes, 0, s, (const float *)d_leaf, d_fmask, d_rank, d_extra, d_open, d_pos, (unsigned)n_slots, log2_n, n_flips);
    LAUNCHCHK();
    return QLDPC_OK;
}

extern "C" int qldpc_polar_flip_select_dev(void *hip_stream, int log2_n, int messages, int n_frames, const void *d_leaf, const uint32_t *d_frozen_mask, const int *d_rank,
                                           const int *d_extra, int n_flips, int *d_pos)
{
    const char *who = "polar_flip_select_dev";
    int rc = pl_args_scalars(who, log2_n, PL_MAX_LOG2N, messages, 1);
    if (!rc) rc = prc_args_count(who, n_frames);
    if (!rc) rc = pfl_args_flips(who, n_flips, PFL_MAX_FLIPS, 0);
    if (rc || n_frames == 0) return rc;
    if (!d_leaf || !d_frozen_mask || !d_pos) { qldpc_set_error("%s: NULL device pointer (d_leaf, d_frozen_mask and d_pos are required)", who); return QLDPC_EINVAL; }
    return pfl_launch_select((hipStream_t)hip_stream, log2_n, messages == QLDPC_POLAR_I8, n_frames, d_leaf, d_frozen_mask, d_rank, d_extra, nullptr, n_flips, d_pos);
}

extern "C" int qldpc_polar_recon_decode_flip(qldpc_polar_recon *r, int n_blocks, uint32_t *d_keys, const int *d_key_bits, const uint32_t *d_syndrome,
                                             const uint32_t *d_crc, const uint32_t *d_extra_bits, const int *d_extra, int n_flips, int resume, int *d_status,
                                             int *d_corrected, int32_t *d_flip_pos, int *d_decodes, int *n_tried)
{
    const char *who = "polar_recon_decode_flip";
    int rc = prc_check_blocks(r, n_blocks, who);
    if (!rc && !r->max_flips) { qldpc_set_error("%s: the session has no flip scratch: make it with qldpc_polar_recon_create_flip", who); rc = QLDPC_ESTATE; }
    if (!rc) rc = pfl_args_flips(who, n_flips, r->max_flips, resume);
    if (rc) return rc;
    if (n_blocks > 0 && (!d_keys || !d_crc || !d_status || !d_flip_pos || (r->n_frozen && !d_syndrome) || (r->n_extra && !d_extra_bits))) {
        qldpc_set_error("%s: NULL device pointer (d_keys, d_crc, d_status and d_flip_pos are required; d_syndrome where N > K, d_extra_bits where n_extra > 0)", who);
        return QLDPC_EINVAL;
    }
    if (n_tried) *n_tried = 0;
    if (n_blocks == 0) return QLDPC_OK;
    const pl_ctx *c = r->c;
    const hipStream_t s = c->stream;
    const bool i8 = c->messages == QLDPC_POLAR_I8;
    const int T = n_flips, Tlog = pl_ctz((long)T), C = r->max_blocks / T;
    const dim3 lanes(PRC_LANES);
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemsetAsync(r->d_count, 0, sizeof(int), s));
    HIPCHK(hipMemsetAsync(d_flip_pos, 0xff, sizeof(int32_t) * (size_t)n_blocks, s));      /* -1 */
    if (resume) {
        hipLaunchKernelGGL(pld_entry_blocks, dim3(prc_grid((size_t)n_blocks, PRC_LANES)), lanes, 0, s, d_key_bits, d_extra, d_status, d_corrected, d_decodes, r->d_open,
                           r->d_count, (unsigned)n_blocks, c->n, r->n_extra, 1);
        LAUNCHCHK();
    } else {                                                      /* the first pass: decode_rounds' round on slot b = block b, no count needed */
        if ((rc = pld_launch_slot_prior(r, nullptr, n_blocks, d_keys, d_key_bits, d_syndrome, d_extra_bits, d_extra, nullptr))) return rc;
        if ((rc = qldpc_polar_decode_rows_dev(r->sc, n_blocks, r->d_llr, r->d_frozen, r->d_flags, nullptr, r->d_info, r->d_x, nullptr))) return rc;
        hipLaunchKernelGGL(pfl_first_verdict, dim3(prc_grid((size_t)n_blocks, PRC_LANES)), lanes, 0, s, (const uint32_t *)r->d_info, (const uint32_t *)r->d_x, d_keys, d_key_bits,
                           d_crc, d_extra, d_status, d_corrected, d_decodes, r->d_open, r->d_count, (unsigned)n_blocks, c->n, c->n_info, r->crc_len, r->crc_poly, r->n_extra);
        LAUNCHCHK();
    }
    HIPCHK(hipMemcpyAsync(&r->h_open, r->d_count, sizeof(int), hipMemcpyDeviceToHost, s));      /* the ONE read-back of the call */
    HIPCHK(hipStreamSynchronize(s));
    const int n_open = r->h_open;
    if (n_open < 0 || n_open > n_blocks) { qldpc_set_error("%s: the open count %d is not in 0 .. n_blocks = %d", who, n_open, n_blocks); return QLDPC_ESTATE; }
    if (n_tried) *n_tried = n_open;
    for (int o0 = 0; o0 < n_open; o0 += C) {
        const int nc = n_open - o0 < C ? n_open - o0 : C;
        const int *open = r->d_open + o0;
        const size_t n_trials = (size_t)nc * (size_t)T, total = n_trials * pmc_quads(c->n);
        if ((rc = pld_launch_slot_prior(r, open, nc, d_keys, d_key_bits, d_syndrome, d_extra_bits, d_extra, nullptr))) return rc;
        if ((rc = qldpc_polar_decode_rows_dev(r->sc, nc, r->d_llr, r->d_frozen, r->d_flags, nullptr, nullptr, nullptr, r->d_leaf))) return rc;      /* the probe */
        if ((rc = pfl_launch_select(s, c->n, i8, nc, r->d_leaf, c->d_fmask, r->d_rank, d_extra, open, T, r->d_pos))) return rc;
        if (i8)
            hipLaunchKernelGGL((pfl_trial_prior<int, int8_t>), dim3(prc_grid(total, PRC_LANES)), lanes, 0, s, open, (const int *)r->d_pos, (const int8_t *)r->d_leaf, d_keys,
                               d_key_bits, d_syndrome, d_extra_bits, d_extra, (const uint32_t *)c->d_fmask, (const int *)r->d_fprefix, (const int *)r->d_rank, r->d_llr,
                               r->d_frozen, r->d_flags, total, c->n, (unsigned)c->W, (unsigned)r->Wf, (unsigned)r->We, Tlog, r->prior_i, r->pin_i);
        else
            hipLaunchKernelGGL((pfl_trial_prior<float, float>), dim3(prc_grid(total, PRC_LANES)), lanes, 0, s, open, (const int *)r->d_pos, (const float *)r->d_leaf, d_keys,
                               d_key_bits, d_syndrome, d_extra_bits, d_extra, (const uint32_t *)c->d_fmask, (const int *)r->d_fprefix, (const int *)r->d_rank, r->d_llr,
                               r->d_frozen, r->d_flags, total, c->n, (unsigned)c->W, (unsigned)r->Wf, (unsigned)r->We, Tlog, r->prior_f, r->pin_f);
        LAUNCHCHK();
        if ((rc = qldpc_polar_decode_rows_dev(r->sc, (int)n_trials, r->d_llr, r->d_frozen, r->d_flags, nullptr, r->d_info, r->d_x, nullptr))) return rc;
        hipLaunchKernelGGL(pfl_settle, dim3(prc_grid(n_trials, PRC_LANES)), lanes, 0, s, open, (const int *)r->d_pos, (const uint32_t *)r->d_info, (const uint32_t *)r->d_x, d_keys,
                           d_key_bits, d_crc, d_status, d_corrected, d_flip_pos, d_decodes, n_trials, c->n, c->n_info, r->crc_len, r->crc_poly, Tlog);
        LAUNCHCHK();
    }
    return QLDPC_OK;
}
