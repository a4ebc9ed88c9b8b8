/*
 * qldpc_polar_mc.hip -- the object and the launches of qldpc_polar_mc_*: a device-resident Monte-Carlo loop
 *
 *     source -> (CRC) -> gather to u -> encode -> table channel -> SC or list decode -> monitor
 *
 * around an existing qldpc_polar context (either form) or an existing qldpc_polar_list context.  The frames are qldpc_polar_mc_core.h's, the
 * kernels qldpc_kernels_polar_mc.h's, the mirror and the shared argument checks qldpc_polar_mc_host.c's.  Everything is queued on the context's
 * stream; a batch ends with ONE read-back of the counter row.
 *
 * The object owns the rows of a batch (info sent and decoded, u, x, LLRs, flips, pick, fail flags), rank[], the table and the counter row with the
 * failed-frame list behind it, all allocated by create: no call allocates anything.  The context is not owned and must outlive the object.
 *
 * qldpc_polar_mc_construct is the same loop with the tally of the genie-aided construction (qldpc_polar_tally_dev) in the decoder's place and no
 * monitor: source -> u -> encode -> table channel -> tally, into a [2][N] row the object owns where its context is an SC context of the lanes'
 * form, with ONE read-back at the end of the call.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "qldpc_kernels_polar_mc.h"
#include "qldpc_polar_ctx.h"

#define PMC_STAGES 5               /* source, encode, channel, decode, monitor */
#define PMC_EVENTS (PMC_STAGES + 1)       /* of a batch; there are two sets: run uses the first, construct takes them in turn */

struct qldpc_polar_mc {
    qldpc_polar *sc;
    qldpc_polar_list *list;
    const pl_ctx *c;               /* of the one that is given */
    int crc_len, A;
    uint32_t crc_poly;
    size_t Wi;                     /* words of an info row */
    uint64_t seed;
    int batch, fail_cap, frozen_mode, source;
    bool have_table;
    pmc_u64 last_failed;           /* frame errors of the last run */
    int *d_rank;
    mc_soft_table *d_tab;
    uint32_t *d_info, *d_dec, *d_u, *d_x, *d_flips, *d_fail, *d_wg_fail;
    int32_t *d_pick;
    void *d_llr;
    pmc_u64 *d_ctr, *h_ctr;        /* PMC_C_ROW counters, then fail_cap entries; the pinned copy of the counters */
    uint64_t *d_tally;             /* [2][N], the accumulator of construct; NULL unless the context is an SC context of the lanes' form */
    hipEvent_t ev[2 * PMC_EVENTS];
    int n_ev;
    dm_ledger mem;                 /* everything create allocates, the pinned h_ctr included (qldpc_devmem.h) */
};

extern "C" void qldpc_polar_mc_free(qldpc_polar_mc *mc)
{
    if (!mc) return;
    if (!mc->mem.blocks.empty() || mc->n_ev) {
        (void)hipSetDevice(mc->c->device);
        (void)hipStreamSynchronize(mc->c->stream);
    }
    for (int i = 0; i < mc->n_ev; i++) (void)hipEventDestroy(mc->ev[i]);
    dm_free_all(&mc->mem);
    delete mc;
}

template <class T> static int pmc_alloc(qldpc_polar_mc *mc, T **q, size_t count)
{
    count = std::max<size_t>(count, 1);      /* an empty array still gets one element */
    const int rc = dm_alloc(&mc->mem, q, count);
    if (rc) qldpc_set_error("polar_mc_create: device allocation of %zu bytes failed: lower batch", sizeof(T) * count);
    return rc;
}

static int pmc_build(qldpc_polar_mc *mc)
{
    const pl_ctx *c = mc->c;
    const size_t B = (size_t)mc->batch, N = (size_t)1 << c->n, esz = c->messages == QLDPC_POLAR_I8 ? 1 : sizeof(float);
    int rc;
    HIPCHK(hipSetDevice(c->device));
    if ((rc = pmc_alloc(mc, &mc->d_rank, 32 * c->W)) || (rc = pmc_alloc(mc, &mc->d_tab, 1)) || (rc = pmc_alloc(mc, &mc->d_info, B * mc->Wi)) ||
        (rc = pmc_alloc(mc, &mc->d_dec, B * mc->Wi)) || (rc = pmc_alloc(mc, &mc->d_u, B * c->W)) || (rc = pmc_alloc(mc, &mc->d_x, B * c->W)) ||
        (rc = pmc_alloc(mc, &mc->d_flips, B)) || (rc = pmc_alloc(mc, &mc->d_fail, B)) || (rc = pmc_alloc(mc, &mc->d_wg_fail, (B + PMC_LANES - 1) / PMC_LANES)) ||
        (rc = pmc_alloc(mc, &mc->d_pick, B)) || (rc = pmc_alloc(mc, (uint8_t **)&mc->d_llr, esz * B * N)) ||
        (rc = pmc_alloc(mc, &mc->d_ctr, (size_t)PMC_C_ROW + (size_t)mc->fail_cap)))
        return rc;
    if (mc->sc && !pl_sc_is_wide(mc->sc) && (rc = pmc_alloc(mc, &mc->d_tally, 2 * N))) return rc;
    if (dm_alloc_pinned(&mc->mem, &mc->h_ctr, PMC_C_ROW)) { qldpc_set_error("polar_mc_create: pinned allocation of the counters failed"); return QLDPC_EHIP; }
    memset(mc->h_ctr, 0, sizeof(pmc_u64) * PMC_C_ROW);
    for (; mc->n_ev < 2 * PMC_EVENTS; mc->n_ev++) HIPCHK(hipEventCreate(&mc->ev[mc->n_ev]));
    /* rank[] from the context's own info_pos */
    std::vector<int> pos((size_t)std::max(c->n_info, 1)), rank(32 * c->W);
    if (c->n_info) HIPCHK(hipMemcpy(pos.data(), c->d_info_pos, sizeof(int) * (size_t)c->n_info, hipMemcpyDeviceToHost));
    pmc_rank(c->n, c->n_info, pos.data(), rank.data());
    HIPCHK(hipMemcpy(mc->d_rank, rank.data(), sizeof(int) * rank.size(), hipMemcpyHostToDevice));
    return QLDPC_OK;
}

extern "C" int qldpc_polar_mc_create(qldpc_polar *sc, qldpc_polar_list *list, uint64_t seed, int batch, int fail_cap, int frozen_mode, qldpc_polar_mc **out)
{
    if (!out) return QLDPC_EINVAL;
    *out = nullptr;
    if ((sc != nullptr) == (list != nullptr)) { qldpc_set_error("polar_mc_create: exactly one of an SC context and a list context is required"); return QLDPC_EINVAL; }
    int rc = pmc_args_modes("polar_mc_create", frozen_mode, QLDPC_MC_SOURCE_RANDOM);
    if (rc) return rc;
    int crc_len = 0;
    uint32_t crc_poly = 0u;
    const pl_ctx *c = sc ? pl_ctx_of_sc(sc) : pl_ctx_of_list(list, &crc_len, &crc_poly);
    if (batch < 0 || batch > c->max_frames) {
        qldpc_set_error("polar_mc_create: batch=%d (0: the context's max_frames = %d, or 1 .. that)", batch, c->max_frames);
        return batch < 0 ? QLDPC_EINVAL : QLDPC_ESIZE;
    }
    if (batch == 0) batch = c->max_frames;
    if (fail_cap < 0 || fail_cap > (1 << 24)) { qldpc_set_error("polar_mc_create: fail_cap=%d (0 .. %d)", fail_cap, 1 << 24); return QLDPC_EINVAL; }
    if ((uint64_t)batch * pmc_quads(c->n) >= (1ull << 31)) {
        qldpc_set_error("polar_mc_create: %d frames of N = 2^%d pass 2^31 lanes of four positions: lower batch", batch, c->n);
        return QLDPC_ESIZE;
    }
    qldpc_polar_mc *mc = new (std::nothrow) qldpc_polar_mc();
    if (!mc) return QLDPC_ENOMEM;
    mc->sc = sc; mc->list = list; mc->c = c;
    mc->crc_len = crc_len; mc->crc_poly = crc_poly; mc->A = c->n_info - crc_len; mc->Wi = pmc_words(c->n_info);
    mc->seed = seed; mc->batch = batch; mc->fail_cap = fail_cap; mc->frozen_mode = frozen_mode; mc->source = QLDPC_MC_SOURCE_RANDOM;
    if ((rc = pmc_build(mc))) { qldpc_polar_mc_free(mc); return rc; }
    *out = mc;
    return QLDPC_OK;
}

extern "C" size_t qldpc_polar_mc_device_bytes(const qldpc_polar_mc *mc) { return mc ? mc->mem.dev_bytes : 0; }

extern "C" int qldpc_polar_mc_set_source(qldpc_polar_mc *mc, int mode)
{
    if (!mc) return QLDPC_EINVAL;
    const int rc = pmc_args_modes("polar_mc_set_source", mc->frozen_mode, mode);
    if (rc) return rc;
    mc->source = mode;
    return QLDPC_OK;
}

extern "C" int qldpc_polar_mc_set_channel(qldpc_polar_mc *mc, int levels, const uint64_t *cum0, const uint64_t *cum1, const float *value)
{
    if (!mc) return QLDPC_EINVAL;
    mc_soft_table tab;
    const int rc = pmc_args_table("polar_mc_set_channel", mc->c->messages, levels, cum0, cum1, value, &tab);
    if (rc) return rc;                                        /* the table in force stays */
    HIPCHK(hipSetDevice(mc->c->device));
    HIPCHK(hipStreamSynchronize(mc->c->stream));              /* a queued channel kernel may still read the old table */
    HIPCHK(hipMemcpy(mc->d_tab, &tab, sizeof(tab), hipMemcpyHostToDevice));
    mc->have_table = true;
    return QLDPC_OK;
}

static unsigned pmc_blocks(size_t lanes, unsigned per) { return (unsigned)((lanes + per - 1) / per); }

/* frames first .. first + n - 1 into the rows given (n <= batch): info, then u, x and the channel as far as `upto` asks (0 info, 1 u, 2 x, 3 channel;
   llr and flips may each be NULL at 3).  ev (or NULL): ev[1] behind the source, ev[2] behind the encoder */
static int pmc_generate(qldpc_polar_mc *mc, uint64_t first, int n, int upto, uint32_t *d_info, uint32_t *d_u, uint32_t *d_x, void *d_llr, uint32_t *d_flips,
                        hipStream_t s, hipEvent_t *ev)
{
    const pl_ctx *c = mc->c;
    hipLaunchKernelGGL(pmc_source, dim3((unsigned)n), dim3(PMC_WAVE), 0, s, d_info, upto >= 1 ? d_u : nullptr, (const int *)mc->d_rank, (const uint32_t *)c->d_fmask,
                       (unsigned)c->W, mc->A, c->n_info, mc->crc_len, mc->crc_poly, mc->frozen_mode, mc->source, mc->seed, first);
    LAUNCHCHK();
    if (ev) HIPCHK(hipEventRecord(ev[1], s));
    if (upto >= 2) {
        const int rc = pl_launch_encode(s, c->n, (size_t)n, d_u, d_x);      /* the launch of qldpc_polar_encode_dev */
        if (rc) return rc;
    }
    if (ev) HIPCHK(hipEventRecord(ev[2], s));
    if (upto < 3) return QLDPC_OK;
    if (d_flips) HIPCHK(hipMemsetAsync(d_flips, 0, sizeof(uint32_t) * (size_t)n, s));
    const unsigned total = (unsigned)((size_t)n * pmc_quads(c->n));
    if (c->messages == QLDPC_POLAR_I8)
        hipLaunchKernelGGL(pmc_channel<true>, dim3(pmc_blocks(total, PMC_LANES)), dim3(PMC_LANES), 0, s, (const uint32_t *)d_x, d_llr, d_flips,
                           (const mc_soft_table *)mc->d_tab, total, c->n, (unsigned)c->W, mc->seed, first);
    else
        hipLaunchKernelGGL(pmc_channel<false>, dim3(pmc_blocks(total, PMC_LANES)), dim3(PMC_LANES), 0, s, (const uint32_t *)d_x, d_llr, d_flips,
                           (const mc_soft_table *)mc->d_tab, total, c->n, (unsigned)c->W, mc->seed, first);
    LAUNCHCHK();
    return QLDPC_OK;
}

extern "C" int qldpc_polar_mc_frames_dev(qldpc_polar_mc *mc, uint64_t first_frame, int n_frames, uint32_t *d_info, uint32_t *d_u, uint32_t *d_x, void *d_llr,
                                         uint32_t *d_flips)
{
    if (!mc) return QLDPC_EINVAL;
    if (n_frames < 0) { qldpc_set_error("polar_mc_frames_dev: n_frames=%d is negative", n_frames); return QLDPC_EINVAL; }
    if (!mc->have_table) { qldpc_set_error("polar_mc_frames_dev: no channel table (qldpc_polar_mc_set_channel comes first)"); return QLDPC_ESTATE; }
    if (n_frames == 0) return QLDPC_OK;
    const pl_ctx *c = mc->c;
    const int upto = d_llr || d_flips ? 3 : (d_x ? 2 : (d_u ? 1 : 0));
    const size_t esz = c->messages == QLDPC_POLAR_I8 ? 1 : sizeof(float);
    HIPCHK(hipSetDevice(c->device));
    for (int done = 0; done < n_frames;) {                    /* by batches: a row that was not asked for is the object's own */
        const int nb = std::min(mc->batch, n_frames - done);
        const size_t o = (size_t)done;
        const int rc = pmc_generate(mc, first_frame + o, nb, upto, d_info ? d_info + o * mc->Wi : mc->d_info, d_u ? d_u + o * c->W : mc->d_u,
                                    d_x ? d_x + o * c->W : mc->d_x, d_llr ? (uint8_t *)d_llr + esz * (o << c->n) : nullptr, d_flips ? d_flips + o : nullptr,
                                    c->stream, nullptr);
        if (rc) return rc;
        done += nb;
    }
    return QLDPC_OK;
}

/* the decode of the batch in the object's rows: the sent u row is the frozen row where the frozen values are random */
static int pmc_decode(qldpc_polar_mc *mc, int n)
{
    const uint32_t *fz = mc->frozen_mode == QLDPC_POLAR_MC_FROZEN_RANDOM ? mc->d_u : nullptr;
    if (mc->sc) return qldpc_polar_decode_dev(mc->sc, n, mc->d_llr, fz, nullptr, mc->d_dec, nullptr, nullptr);
    return qldpc_polar_list_decode_dev(mc->list, n, mc->d_llr, fz, nullptr, nullptr, mc->d_dec, nullptr, mc->d_pick, nullptr, nullptr);
}

/* the stage times of the batch recorded in the event set `ev`, which has finished or is waited for, added to stage[] */
static int pmc_add_stage_times(hipEvent_t *ev, int stages, double *stage)
{
    HIPCHK(hipEventSynchronize(ev[stages]));
    for (int k = 0; k < stages; k++) {
        float t = 0.0f;
        HIPCHK(hipEventElapsedTime(&t, ev[k], ev[k + 1]));
        stage[k] += (double)t;
    }
    return QLDPC_OK;
}

extern "C" int qldpc_polar_mc_run(qldpc_polar_mc *mc, uint64_t first_frame, uint64_t max_frames, uint64_t max_frame_errors, uint64_t *counters, double *ms)
{
    if (!mc || !counters) return QLDPC_EINVAL;
    memset(counters, 0, sizeof(uint64_t) * QLDPC_POLAR_MC_COUNTERS);
    counters[QLDPC_POLAR_MC_NEXT_FRAME] = first_frame;
    if (ms) memset(ms, 0, sizeof(double) * 8);
    if (!mc->have_table) { qldpc_set_error("polar_mc_run: no channel table (qldpc_polar_mc_set_channel comes first)"); return QLDPC_ESTATE; }
    const pl_ctx *c = mc->c;
    HIPCHK(hipSetDevice(c->device));
    const hipStream_t s = c->stream;
    HIPCHK(hipMemsetAsync(mc->d_ctr, 0, sizeof(pmc_u64) * ((size_t)PMC_C_ROW + (size_t)mc->fail_cap), s));
    memset(mc->h_ctr, 0, sizeof(pmc_u64) * PMC_C_ROW);
    mc->last_failed = 0;
    double stage[PMC_STAGES] = {0.0};
    uint64_t batches = 0;
    const auto t_start = std::chrono::steady_clock::now();
    for (uint64_t done = 0; done < max_frames;) {
        const int nb = (int)std::min<uint64_t>((uint64_t)mc->batch, max_frames - done);
        const uint64_t first = first_frame + done;
        const pmc_u64 base = mc->h_ctr[PMC_C_FRAME_ERRORS];       /* the failed frames before this batch: the last read-back */
        HIPCHK(hipEventRecord(mc->ev[0], s));
        int rc = pmc_generate(mc, first, nb, 3, mc->d_info, mc->d_u, mc->d_x, mc->d_llr, mc->d_flips, s, mc->ev);
        if (rc) return rc;
        HIPCHK(hipEventRecord(mc->ev[3], s));
        if ((rc = pmc_decode(mc, nb))) return rc;
        HIPCHK(hipEventRecord(mc->ev[4], s));
        hipLaunchKernelGGL(pmc_monitor, dim3(pmc_blocks((size_t)nb, PMC_LANES)), dim3(PMC_LANES), 0, s, (const uint32_t *)mc->d_dec, (const uint32_t *)mc->d_info,
                           (const int32_t *)(mc->list ? mc->d_pick : nullptr), (const uint32_t *)mc->d_flips, (unsigned)nb, (unsigned)mc->Wi, mc->A, 1u << c->n, mc->d_ctr,
                           mc->d_fail, mc->d_wg_fail);
        LAUNCHCHK();
        if (base < (pmc_u64)mc->fail_cap) {                       /* a full list takes no more */
            hipLaunchKernelGGL(pmc_append, dim3(pmc_blocks((size_t)nb, PMC_WAVE)), dim3(PMC_WAVE), 0, s, (const uint32_t *)mc->d_fail, (const uint32_t *)mc->d_wg_fail,
                               (unsigned)nb, first, base, (pmc_u64)mc->fail_cap, mc->d_ctr + PMC_C_ROW);
            LAUNCHCHK();
        }
        HIPCHK(hipEventRecord(mc->ev[PMC_STAGES], s));
        HIPCHK(hipMemcpyAsync(mc->h_ctr, mc->d_ctr, sizeof(pmc_u64) * PMC_C_DEVICE, hipMemcpyDeviceToHost, s));      /* the ONE read-back of the batch */
        HIPCHK(hipStreamSynchronize(s));
        if ((rc = pmc_add_stage_times(mc->ev, PMC_STAGES, stage))) return rc;
        batches++;
        done += (uint64_t)nb;
        if (max_frame_errors && mc->h_ctr[PMC_C_FRAME_ERRORS] >= max_frame_errors) break;
    }
    static_assert(PMC_C_FRAMES == QLDPC_POLAR_MC_FRAMES && PMC_C_BIT_ERRORS == QLDPC_POLAR_MC_BIT_ERRORS && PMC_C_FRAME_ERRORS == QLDPC_POLAR_MC_FRAME_ERRORS &&
                  PMC_C_UNDETECTED == QLDPC_POLAR_MC_UNDETECTED && PMC_C_CRC_FAILS == QLDPC_POLAR_MC_CRC_FAILS && PMC_C_FLIPS == QLDPC_POLAR_MC_CHANNEL_FLIPS &&
                  PMC_C_CHANNEL_BITS == QLDPC_POLAR_MC_CHANNEL_BITS && PMC_C_DEVICE == QLDPC_POLAR_MC_BATCHES && PMC_C_ROW == QLDPC_POLAR_MC_COUNTERS,
                  "the device's counter row is the head of the ABI's");
    for (int k = 0; k < PMC_C_DEVICE; k++) counters[k] = mc->h_ctr[k];
    counters[QLDPC_POLAR_MC_BATCHES] = batches;
    counters[QLDPC_POLAR_MC_NEXT_FRAME] = first_frame + counters[QLDPC_POLAR_MC_FRAMES];
    mc->last_failed = mc->h_ctr[PMC_C_FRAME_ERRORS];
    if (ms) {
        static_assert(QLDPC_POLAR_MC_MS_SOURCE == 0 && QLDPC_POLAR_MC_MS_MONITOR == PMC_STAGES - 1 && QLDPC_POLAR_MC_MS_TOTAL == PMC_STAGES, "the stages in the ABI's order");
        for (int k = 0; k < PMC_STAGES; k++) ms[k] = stage[k];
        ms[QLDPC_POLAR_MC_MS_TOTAL] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    }
    return QLDPC_OK;
}

/* The genie-aided construction (qldpc_polar_tally_core.h) over the object's own frames: per batch source -> encode -> channel -> tally of the
   batch's LLRs against its sent u row, into the object's [2][N] row.  Nothing is read back before the end; the times of a batch are read one
   batch late, from the other event set, while the next batch runs */
extern "C" int qldpc_polar_mc_construct(qldpc_polar_mc *mc, uint64_t first_frame, uint64_t n_frames, uint64_t *tally, double *ms)
{
    if (!mc || !tally) return QLDPC_EINVAL;
    if (ms) memset(ms, 0, sizeof(double) * 8);
    if (!mc->sc) {
        qldpc_set_error("polar_mc_construct: the tally is the SC decoder's: create the object around a qldpc_polar context of the lanes' form, not a list context");
        return QLDPC_EUNSUPPORTED;
    }
    if (pl_sc_is_wide(mc->sc)) {
        qldpc_set_error("polar_mc_construct: the tally has no wide form: create the object around a QLDPC_POLAR_LANES context");
        return QLDPC_EUNSUPPORTED;
    }
    if (mc->frozen_mode != QLDPC_POLAR_MC_FROZEN_RANDOM) {
        qldpc_set_error("polar_mc_construct: u must be uniformly random at every position: create the object with QLDPC_POLAR_MC_FROZEN_RANDOM");
        return QLDPC_EUNSUPPORTED;
    }
    if (mc->source != QLDPC_MC_SOURCE_RANDOM) {
        qldpc_set_error("polar_mc_construct: u must be uniformly random at every position: qldpc_polar_mc_set_source(QLDPC_MC_SOURCE_RANDOM) comes first");
        return QLDPC_ESTATE;
    }
    if (!mc->have_table) { qldpc_set_error("polar_mc_construct: no channel table (qldpc_polar_mc_set_channel comes first)"); return QLDPC_ESTATE; }
    const pl_ctx *c = mc->c;
    const size_t row_bytes = sizeof(uint64_t) * ((size_t)2 << c->n);
    HIPCHK(hipSetDevice(c->device));
    const hipStream_t s = c->stream;
    HIPCHK(hipMemsetAsync(mc->d_tally, 0, row_bytes, s));
    double stage[PMC_STAGES] = {0.0};
    uint64_t batches = 0;
    int rc;
    const auto t_start = std::chrono::steady_clock::now();
    for (uint64_t done = 0; done < n_frames; batches++) {
        const int nb = (int)std::min<uint64_t>((uint64_t)mc->batch, n_frames - done);
        hipEvent_t *ev = mc->ev + (batches & 1u) * PMC_EVENTS;
        if (batches >= 2 && (rc = pmc_add_stage_times(ev, PMC_STAGES - 1, stage))) return rc;      /* the set's last use, two batches ago */
        HIPCHK(hipEventRecord(ev[0], s));
        if ((rc = pmc_generate(mc, first_frame + done, nb, 3, mc->d_info, mc->d_u, mc->d_x, mc->d_llr, nullptr, s, ev))) return rc;
        HIPCHK(hipEventRecord(ev[3], s));
        if ((rc = qldpc_polar_tally_dev(mc->sc, nb, mc->d_llr, mc->d_u, mc->d_tally))) return rc;
        HIPCHK(hipEventRecord(ev[4], s));
        done += (uint64_t)nb;
    }
    HIPCHK(hipMemcpyAsync(tally, mc->d_tally, row_bytes, hipMemcpyDeviceToHost, s));      /* the ONE read-back of the call */
    HIPCHK(hipStreamSynchronize(s));
    for (uint64_t b = batches > 2 ? batches - 2 : 0; b < batches; b++)
        if ((rc = pmc_add_stage_times(mc->ev + (b & 1u) * PMC_EVENTS, PMC_STAGES - 1, stage))) return rc;
    if (ms) {
        for (int k = 0; k < PMC_STAGES; k++) ms[k] = stage[k];      /* the tally in the decode slot, nothing in the monitor's */
        ms[QLDPC_POLAR_MC_MS_TOTAL] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    }
    return QLDPC_OK;
}

extern "C" int qldpc_polar_mc_failed_frames(qldpc_polar_mc *mc, uint64_t *frames, int cap)
{
    if (!mc || cap < 0 || (cap && !frames)) return QLDPC_EINVAL;
    const int listed = (int)std::min<pmc_u64>(mc->last_failed, (pmc_u64)mc->fail_cap), n = std::min(listed, cap);
    if (n == 0) return listed;
    HIPCHK(hipSetDevice(mc->c->device));
    HIPCHK(hipStreamSynchronize(mc->c->stream));
    HIPCHK(hipMemcpy(frames, mc->d_ctr + PMC_C_ROW, sizeof(pmc_u64) * (size_t)n, hipMemcpyDeviceToHost));
    return listed;
}
