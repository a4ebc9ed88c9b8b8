/*
 * qldpc_mc.hip -- the Monte-Carlo loop of the reference harness (source -> encoder -> BSC -> decoder -> monitor, BS/src/main.cpp:335-393)
 * with nothing per bit crossing the host (qldpc_mc_*).  The frame definition is qldpc_mc_core.h: frame i is a pure function of (seed, i).
 *
 * mc_source:  one lane per info word of the packed [frame][word] layout, consecutive lanes = consecutive words of a row (the last lanes of a
 *     row run on into the next one), one Philox call per word.
 * mc_channel: one lane per codeword word: 8 Philox calls, the 32 classes of the word by two 16-byte loads from the padded class map (32 N
 *     bytes shared by all frames: L2-resident), the two thresholds wave-uniform kernel arguments; rx = cw ^ flips.  The lanes of word 0 also
 *     write the frame's |LLR| for qldpc_load_bits_dev.
 * mc_monitor: one wave per frame (a wave strides over the frames): be = popcount((out ^ cw) & info_mask) and the flips at channel VNs summed
 *     over the lanes by shuffles, the per-frame verdicts summed in (wave-uniform) registers over the wave's frames, then ONE atomicAdd per
 *     wave and counter from lane 0 -- plus, per frame, one on the iteration histogram and, for a failed frame, one returning add on the
 *     slot counter of the failed-frame list.
 *
 * No kernel waits on another wave.  The decoder and the encoder are driven through their public calls only; qldpc_engine_int.h is read for
 * the decoder's sizes, device and stream.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/qldpc.h"
#include "qldpc_engine_int.h"
#include "qldpc_mc_core.h"

#define MC_LANES 256
#define MC_MAX_WAVES 2048          /* of a monitor launch */
enum { MC_FRAMES = 0, MC_BIT_ERRORS, MC_FRAME_ERRORS, MC_UNDETECTED, MC_NOT_CONVERGED, MC_ITER_SUM, MC_ITER_MAX, MC_FLIPS, MC_CHANNEL_BITS, MC_FAIL_SLOTS,
       MC_COUNTERS };

typedef unsigned long long mc_u64;

__global__ __launch_bounds__(MC_LANES) void mc_source(uint32_t *__restrict__ info, unsigned total, unsigned Wk, int K, uint64_t seed, uint64_t first)
{
    const unsigned i = blockIdx.x * MC_LANES + threadIdx.x;
    if (i >= total) return;
    const unsigned f = i / Wk, j = i - f * Wk;
    info[i] = mc_info_word(seed, first + f, j, K);
}

__global__ __launch_bounds__(MC_LANES) void mc_channel(const uint32_t *__restrict__ cw, uint32_t *__restrict__ rx, const uint4 *__restrict__ cls,
                                                       unsigned total, unsigned Wn, uint64_t seed, uint64_t first, uint32_t t_channel, uint32_t t_pinned,
                                                       float *__restrict__ llr_mag, float mag)
{
    const unsigned i = blockIdx.x * MC_LANES + threadIdx.x;
    if (i >= total) return;
    const unsigned f = i / Wn, w = i - f * Wn;
    const uint4 a = cls[2u * w], b = cls[2u * w + 1u];
    const uint32_t cls4[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    rx[i] = cw[i] ^ mc_flip_word(seed, first + f, w, cls4, t_channel, t_pinned);
    if (w == 0 && llr_mag) llr_mag[f] = mag;
}

__device__ static inline unsigned mc_wave_sum(unsigned x)
{
    for (int s = 32; s > 0; s >>= 1) x += __shfl_xor(x, s, 64);
    return x;
}

__global__ __launch_bounds__(MC_LANES) void mc_monitor(const uint32_t *__restrict__ out, const uint32_t *__restrict__ cw, const uint32_t *__restrict__ rx,
                                                       const uint32_t *__restrict__ info_mask, const uint32_t *__restrict__ chan_mask,
                                                       const int *__restrict__ iters, const int *__restrict__ ok, unsigned n, unsigned Wn, int n_ite,
                                                       uint64_t first, unsigned channel_vns, mc_u64 *__restrict__ ctr, mc_u64 *__restrict__ hist,
                                                       mc_u64 *__restrict__ fails, unsigned fail_cap)
{
    const unsigned lane = threadIdx.x & 63u, waves = gridDim.x * (MC_LANES / 64);
    mc_u64 s_frames = 0, s_be = 0, s_fe = 0, s_ud = 0, s_nc = 0, s_it = 0, s_mx = 0, s_fl = 0;
    for (unsigned f = blockIdx.x * (MC_LANES / 64) + (threadIdx.x >> 6); f < n; f += waves) {
        const size_t row = (size_t)f * Wn;
        unsigned be = 0, fl = 0;
        for (unsigned w = lane; w < Wn; w += 64u) {
            const uint32_t c = cw[row + w];
            be += (unsigned)__popc((out[row + w] ^ c) & info_mask[w]);
            fl += (unsigned)__popc((rx[row + w] ^ c) & chan_mask[w]);
        }
        be = mc_wave_sum(be);
        fl = mc_wave_sum(fl);
        const int it = min(max(iters[f], 0), n_ite);
        const bool good = ok[f] != 0;
        s_frames++; s_be += be; s_fl += fl; s_it += (mc_u64)it;
        s_mx = max(s_mx, (mc_u64)it);
        s_fe += be > 0; s_ud += good && be > 0; s_nc += !good;
        if (lane == 0) {
            atomicAdd(hist + it, 1ull);
            if (be > 0) {
                const mc_u64 slot = atomicAdd(ctr + MC_FAIL_SLOTS, 1ull);
                if (slot < fail_cap) fails[slot] = first + f;
            }
        }
    }
    if (lane != 0 || s_frames == 0) return;
    atomicAdd(ctr + MC_FRAMES, s_frames);
    atomicAdd(ctr + MC_ITER_SUM, s_it);
    atomicMax(ctr + MC_ITER_MAX, s_mx);
    atomicAdd(ctr + MC_CHANNEL_BITS, s_frames * channel_vns);
    if (s_fl) atomicAdd(ctr + MC_FLIPS, s_fl);
    if (s_be) atomicAdd(ctr + MC_BIT_ERRORS, s_be);
    if (s_fe) atomicAdd(ctr + MC_FRAME_ERRORS, s_fe);
    if (s_ud) atomicAdd(ctr + MC_UNDETECTED, s_ud);
    if (s_nc) atomicAdd(ctr + MC_NOT_CONVERGED, s_nc);
}

/* ------------------------------------------------------------------ host ---- */

struct qldpc_mc {
    qldpc_decoder *dec; qldpc_encoder *enc;      /* not owned */
    int N, K, Wn, Wk, n_ite, batch, fail_cap, device;
    unsigned channel_vns;
    uint64_t seed; double parity_ber;
    uint8_t *d_cls;                    /* [32 Wn] padded class map: qldpc_load_bits_dev reads its first N bytes, mc_channel all of it */
    uint32_t *d_info_mask, *d_chan_mask, *d_info, *d_cw, *d_rx, *d_out;
    float *d_mag; int *d_iters, *d_ok;
    mc_u64 *d_ctr;                     /* MC_COUNTERS counters, n_ite + 1 histogram bins, fail_cap frame indices */
    mc_u64 *h_ctr;                     /* pinned, MC_COUNTERS */
    hipEvent_t ev[7];                  /* the stage boundaries of a batch: source | encode | channel | load | run | fetch + monitor */
    size_t dev_bytes;
};

extern "C" void qldpc_mc_cfg_default(qldpc_mc_cfg *cfg)
{
    if (!cfg) return;
    memset(cfg, 0, sizeof(*cfg));
    cfg->fail_cap = 1024;
}

extern "C" void qldpc_mc_free(qldpc_mc *mc)
{
    if (!mc) return;
    (void)hipSetDevice(mc->device);
    void *dev[] = {mc->d_cls, mc->d_info_mask, mc->d_chan_mask, mc->d_info, mc->d_cw, mc->d_rx, mc->d_out, mc->d_mag, mc->d_iters, mc->d_ok, mc->d_ctr};
    for (void *p : dev) if (p) (void)hipFree(p);
    if (mc->h_ctr) (void)hipHostFree(mc->h_ctr);
    for (hipEvent_t e : mc->ev) if (e) (void)hipEventDestroy(e);
    delete mc;
}

template <typename T> static int mc_alloc(qldpc_mc *mc, T **p, size_t count)
{
    if (hipMalloc((void **)p, sizeof(T) * count) != hipSuccess) { *p = nullptr; qldpc_set_error("mc_create: device allocation of %zu bytes failed", sizeof(T) * count); return QLDPC_ENOMEM; }
    mc->dev_bytes += sizeof(T) * count;
    return QLDPC_OK;
}

static int mc_build(qldpc_mc *mc, const uint8_t *vn_class)
{
    std::vector<int> pos((size_t)mc->K);
    int rc = qldpc_encoder_info_bits_pos(mc->enc, pos.data());
    if (rc) return rc;
    const size_t Wn = (size_t)mc->Wn, B = (size_t)mc->batch;
    std::vector<uint8_t> cls(32 * Wn);
    std::vector<uint32_t> info_mask(Wn), chan_mask(Wn, 0u);
    if (mc_classes(mc->K, mc->N, pos.data(), vn_class, cls.data(), info_mask.data())) {
        qldpc_set_error("mc_create: the encoder's info_bits_pos do not fit the decoder's N = %d, or a VN class above 2", mc->N);
        return QLDPC_EINVAL;
    }
    for (int v = 0; v < mc->N; v++)
        if (cls[(size_t)v] == QLDPC_VN_CHANNEL) { chan_mask[(size_t)v >> 5] |= 0x80000000u >> (v & 31); mc->channel_vns++; }
    HIPCHK(hipSetDevice(mc->device));
    if ((rc = mc_alloc(mc, &mc->d_cls, 32 * Wn)) || (rc = mc_alloc(mc, &mc->d_info_mask, Wn)) || (rc = mc_alloc(mc, &mc->d_chan_mask, Wn)) ||
        (rc = mc_alloc(mc, &mc->d_info, B * (size_t)mc->Wk)) || (rc = mc_alloc(mc, &mc->d_cw, B * Wn)) || (rc = mc_alloc(mc, &mc->d_rx, B * Wn)) ||
        (rc = mc_alloc(mc, &mc->d_out, B * Wn)) || (rc = mc_alloc(mc, &mc->d_mag, B)) || (rc = mc_alloc(mc, &mc->d_iters, B)) || (rc = mc_alloc(mc, &mc->d_ok, B)) ||
        (rc = mc_alloc(mc, &mc->d_ctr, (size_t)MC_COUNTERS + (size_t)mc->n_ite + 1 + (size_t)mc->fail_cap)))
        return rc;
    if (hipHostMalloc((void **)&mc->h_ctr, sizeof(mc_u64) * MC_COUNTERS, hipHostMallocDefault) != hipSuccess) { mc->h_ctr = nullptr; return QLDPC_ENOMEM; }
    HIPCHK(hipMemcpy(mc->d_cls, cls.data(), 32 * Wn, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(mc->d_info_mask, info_mask.data(), 4 * Wn, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(mc->d_chan_mask, chan_mask.data(), 4 * Wn, hipMemcpyHostToDevice));
    for (hipEvent_t &e : mc->ev) HIPCHK(hipEventCreate(&e));
    return qldpc_encoder_reserve(mc->enc, mc->batch);
}

extern "C" int qldpc_mc_create(qldpc_decoder *dec, qldpc_encoder *enc, const uint8_t *vn_class, const qldpc_mc_cfg *cfg, qldpc_mc **out)
{
    if (!out) return QLDPC_EINVAL;
    *out = nullptr;
    if (!dec || !enc || !cfg) return QLDPC_EINVAL;
    if (cfg->reserved[0] || cfg->reserved[1]) return QLDPC_EINVAL;
    const int batch = cfg->batch ? cfg->batch : dec->cfg.max_frames;
    if (batch < 1 || batch > dec->cfg.max_frames) { qldpc_set_error("mc_create: batch=%d, the decoder holds %d frames", cfg->batch, dec->cfg.max_frames); return QLDPC_ESIZE; }
    if (cfg->fail_cap < 1) { qldpc_set_error("mc_create: fail_cap=%d (at least 1)", cfg->fail_cap); return QLDPC_ESIZE; }
    if (!(cfg->parity_ber >= 0.0 && cfg->parity_ber < 1.0)) { qldpc_set_error("mc_create: parity_ber=%g outside [0, 1)", cfg->parity_ber); return QLDPC_ESIZE; }
    if (qldpc_encoder_k(enc) != dec->K) { qldpc_set_error("mc_create: the encoder has K = %d, the decoder K = %d", qldpc_encoder_k(enc), dec->K); return QLDPC_ESIZE; }
    if ((uint64_t)batch * (uint64_t)((dec->N + 31) / 32) >= (1ull << 31)) { qldpc_set_error("mc_create: %d frames of N = %d pass 2^31 words", batch, dec->N); return QLDPC_ESIZE; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { qldpc_set_error("no HIP device visible: libqldpc has no CPU fallback"); return QLDPC_ENODEV; }
    qldpc_mc *mc = new (std::nothrow) qldpc_mc();
    if (!mc) return QLDPC_ENOMEM;
    mc->dec = dec; mc->enc = enc;
    mc->N = dec->N; mc->K = dec->K; mc->Wn = (dec->N + 31) / 32; mc->Wk = (dec->K + 31) / 32;
    mc->n_ite = dec->cfg.n_ite; mc->batch = batch; mc->fail_cap = cfg->fail_cap; mc->device = dec->device;
    mc->seed = cfg->seed; mc->parity_ber = cfg->parity_ber;
    const int rc = mc_build(mc, vn_class);
    if (rc) { qldpc_mc_free(mc); return rc; }
    *out = mc;
    return QLDPC_OK;
}

extern "C" size_t qldpc_mc_device_bytes(const qldpc_mc *mc) { return mc ? mc->dev_bytes : 0; }

static unsigned mc_blocks(size_t lanes) { return (unsigned)((lanes + MC_LANES - 1) / MC_LANES); }

/* source -> encoder -> channel for frames [first, first + n) on stream s; d_cw / d_rx / d_mag may be NULL from the right; ev != NULL: ev[1] after the
 * source, ev[2] after the encoder */
static int mc_generate(qldpc_mc *mc, uint64_t first, int n, double qber, uint32_t *d_info, uint32_t *d_cw, uint32_t *d_rx, float *d_mag, hipStream_t s,
                       hipEvent_t *ev = nullptr)
{
    const unsigned ti = (unsigned)n * (unsigned)mc->Wk, tn = (unsigned)n * (unsigned)mc->Wn;
    hipLaunchKernelGGL(mc_source, dim3(mc_blocks(ti)), dim3(MC_LANES), 0, s, d_info, ti, (unsigned)mc->Wk, mc->K, mc->seed, first);
    LAUNCHCHK();
    if (ev) HIPCHK(hipEventRecord(ev[1], s));
    if (!d_cw) return QLDPC_OK;
    const int rc = qldpc_encode_packed_dev(mc->enc, d_info, d_cw, n, (void *)s);
    if (rc || !d_rx) return rc;
    if (ev) HIPCHK(hipEventRecord(ev[2], s));
    hipLaunchKernelGGL(mc_channel, dim3(mc_blocks(tn)), dim3(MC_LANES), 0, s, (const uint32_t *)d_cw, d_rx, (const uint4 *)mc->d_cls, tn, (unsigned)mc->Wn,
                       mc->seed, first, mc_threshold(qber), mc_threshold(mc->parity_ber), d_mag, qldpc_bsc_llr((float)qber));
    LAUNCHCHK();
    return QLDPC_OK;
}

extern "C" int qldpc_mc_frames_dev(qldpc_mc *mc, uint64_t first_frame, int n_frames, double qber, uint32_t *d_info, uint32_t *d_cw, uint32_t *d_rx)
{
    if (!mc || !d_info || (d_rx && !d_cw) || n_frames < 0) return QLDPC_EINVAL;
    if (!(qber >= 0.0 && qber < 1.0)) { qldpc_set_error("mc_frames_dev: qber=%g outside [0, 1)", qber); return QLDPC_ESIZE; }
    if ((uint64_t)n_frames * (uint64_t)mc->Wn >= (1ull << 31)) { qldpc_set_error("mc_frames_dev: %d frames of N = %d pass 2^31 words", n_frames, mc->N); return QLDPC_ESIZE; }
    if (n_frames == 0) return QLDPC_OK;
    HIPCHK(hipSetDevice(mc->device));
    return mc_generate(mc, first_frame, n_frames, qber, d_info, d_cw, d_rx, nullptr, mc->dec->stream);
}

static void mc_result(const qldpc_mc *mc, uint64_t first, qldpc_mc_result *r)
{
    const mc_u64 *c = mc->h_ctr;
    r->frames = c[MC_FRAMES]; r->bit_errors = c[MC_BIT_ERRORS]; r->frame_errors = c[MC_FRAME_ERRORS]; r->undetected = c[MC_UNDETECTED];
    r->not_converged = c[MC_NOT_CONVERGED]; r->iter_sum = c[MC_ITER_SUM]; r->iter_max = c[MC_ITER_MAX];
    r->channel_flips = c[MC_FLIPS]; r->channel_bits = c[MC_CHANNEL_BITS];
    r->next_frame = first + r->frames;
}

extern "C" int qldpc_mc_run(qldpc_mc *mc, double qber, uint64_t first_frame, uint64_t max_frames, uint64_t max_frame_errors, qldpc_mc_result *result)
{
    if (!mc || !result) return QLDPC_EINVAL;
    memset(result, 0, sizeof(*result));
    result->next_frame = first_frame;
    if (!(qber > 0.0 && qber < 0.5)) { qldpc_set_error("mc_run: qber=%g outside (0, 0.5)", qber); return QLDPC_ESIZE; }
    HIPCHK(hipSetDevice(mc->device));
    const hipStream_t s = mc->dec->stream;
    const size_t ctr_words = (size_t)MC_COUNTERS + (size_t)mc->n_ite + 1 + (size_t)mc->fail_cap;
    mc_u64 *hist = mc->d_ctr + MC_COUNTERS, *fails = hist + mc->n_ite + 1;
    HIPCHK(hipMemsetAsync(mc->d_ctr, 0, sizeof(mc_u64) * ctr_words, s));
    memset(mc->h_ctr, 0, sizeof(mc_u64) * MC_COUNTERS);
    const auto t_start = std::chrono::steady_clock::now();
    for (uint64_t done = 0; done < max_frames;) {
        const int nb = (int)std::min<uint64_t>((uint64_t)mc->batch, max_frames - done);
        const uint64_t first = first_frame + done;
        HIPCHK(hipEventRecord(mc->ev[0], s));
        int rc = mc_generate(mc, first, nb, qber, mc->d_info, mc->d_cw, mc->d_rx, mc->d_mag, s, mc->ev);
        if (rc) return rc;
        HIPCHK(hipEventRecord(mc->ev[3], s));
        if ((rc = qldpc_load_bits_dev(mc->dec, mc->d_rx, mc->d_mag, mc->d_cls, nb))) return rc;
        HIPCHK(hipEventRecord(mc->ev[4], s));
        if ((rc = qldpc_run(mc->dec))) return rc;
        HIPCHK(hipEventRecord(mc->ev[5], s));
        if ((rc = qldpc_fetch_packed_dev(mc->dec, mc->d_out))) return rc;
        if ((rc = qldpc_fetch_status_dev(mc->dec, mc->d_iters, mc->d_ok))) return rc;
        const unsigned waves = (unsigned)std::min(nb, MC_MAX_WAVES);
        hipLaunchKernelGGL(mc_monitor, dim3((waves + 3u) / 4u), dim3(MC_LANES), 0, s, (const uint32_t *)mc->d_out, (const uint32_t *)mc->d_cw, (const uint32_t *)mc->d_rx,
                           (const uint32_t *)mc->d_info_mask, (const uint32_t *)mc->d_chan_mask, (const int *)mc->d_iters, (const int *)mc->d_ok, (unsigned)nb,
                           (unsigned)mc->Wn, mc->n_ite, first, mc->channel_vns, mc->d_ctr, hist, fails, (unsigned)mc->fail_cap);
        LAUNCHCHK();
        HIPCHK(hipEventRecord(mc->ev[6], s));
        HIPCHK(hipMemcpyAsync(mc->h_ctr, mc->d_ctr, sizeof(mc_u64) * MC_COUNTERS, hipMemcpyDeviceToHost, s));      /* the one read-back of a batch */
        HIPCHK(hipStreamSynchronize(s));
        double *const stage[6] = {&result->source_ms, &result->encode_ms, &result->channel_ms, &result->load_ms, &result->decode_ms, &result->monitor_ms};
        for (int k = 0; k < 6; k++) {
            float ms = 0.0f;
            HIPCHK(hipEventElapsedTime(&ms, mc->ev[k], mc->ev[k + 1]));
            *stage[k] += (double)ms;
        }
        result->batches++;
        done += (uint64_t)nb;
        if (max_frame_errors && mc->h_ctr[MC_FRAME_ERRORS] >= max_frame_errors) break;
    }
    result->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    mc_result(mc, first_frame, result);
    return QLDPC_OK;
}

extern "C" int qldpc_mc_iter_hist(qldpc_mc *mc, uint64_t *hist, int cap)
{
    if (!mc || !hist || cap < 0) return QLDPC_EINVAL;
    const int bins = std::min(cap, mc->n_ite + 1);
    HIPCHK(hipSetDevice(mc->device));
    HIPCHK(hipStreamSynchronize(mc->dec->stream));
    if (bins) HIPCHK(hipMemcpy(hist, mc->d_ctr + MC_COUNTERS, sizeof(mc_u64) * (size_t)bins, hipMemcpyDeviceToHost));
    return mc->n_ite + 1;
}

extern "C" int qldpc_mc_failed_frames(qldpc_mc *mc, uint64_t *frames, int cap)
{
    if (!mc || cap < 0 || (cap && !frames)) return QLDPC_EINVAL;
    HIPCHK(hipSetDevice(mc->device));
    HIPCHK(hipStreamSynchronize(mc->dec->stream));
    mc_u64 slots = 0;
    HIPCHK(hipMemcpy(&slots, mc->d_ctr + MC_FAIL_SLOTS, sizeof(slots), hipMemcpyDeviceToHost));
    const int listed = (int)std::min<mc_u64>(slots, (mc_u64)mc->fail_cap);
    if (listed == 0) return 0;
    std::vector<uint64_t> all((size_t)listed);
    HIPCHK(hipMemcpy(all.data(), mc->d_ctr + MC_COUNTERS + mc->n_ite + 1, sizeof(mc_u64) * (size_t)listed, hipMemcpyDeviceToHost));
    std::sort(all.begin(), all.end());      /* the slots of a batch are handed out in arrival order */
    const int n = std::min(listed, cap);
    if (n) memcpy(frames, all.data(), sizeof(uint64_t) * (size_t)n);
    return listed;
}
