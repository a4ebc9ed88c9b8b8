/*
 * qldpc_engine_edge.hip -- the edge-parallel engine of the BP decoder: one block at a time, lanes over edges (qldpc_kernels_edge.h).
 *
 * Flooding schedule, MS / OMS / NMS / SPA.  State: d_llr [F][N], d_a = v2c and d_b / e_c2v1 = c2v [F][E] (ping-pong by iteration parity), packed sign
 * and hard-decision words [F][W], and what struct edge_state holds.  qldpc_engine.hip owns the C ABI: it checks arguments and call sequence and hands
 * a decoder of this engine to the functions below (declared in qldpc_engine_int.h).
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <type_traits>

#include "qldpc_engine_int.h"
#include "qldpc_kernels_edge.h"

/* the largest VN degree: a chunk of QE_THREADS VNs stages QE_THREADS * max_dv messages in 64 KiB of LDS */
int edge_max_dv(void) { return (int)(64 * 1024 / (QE_THREADS * sizeof(float))); }

bool edge_supports(const qldpc_decoder_cfg *cfg, const qldpc_code *code)
{
    return cfg->schedule == QLDPC_SCHED_FLOODING && cfg->rule <= QLDPC_RULE_SPA && code->max_dc <= 64 && code->max_dv <= edge_max_dv();
}

int edge_create(qldpc_decoder *d, const qldpc_code *code)
{
    edge_state &s = d->edge;
    const size_t F = (size_t)d->cfg.max_frames;
    int rc;
    s.eW = words32(d->N);
    s.eS = code->max_dc <= 8 ? 8 : (code->max_dc <= 16 ? 16 : (code->max_dc <= 32 ? 32 : 64));
    s.e_lds = (size_t)QE_THREADS * (size_t)code->max_dv * sizeof(float);
    s.e_stride = d->cfg.n_ite + 2;
    if ((rc = dm_alloc(&d->mem, &d->d_llr, F * d->N))) return rc;
    if ((rc = dm_alloc(&d->mem, &d->d_a, F * d->E))) return rc;
    if ((rc = dm_alloc(&d->mem, &d->d_b, F * d->E))) return rc;
    if ((rc = dm_alloc(&d->mem, &s.e_c2v1, F * d->E))) return rc;
    if ((rc = dm_alloc(&d->mem, &s.e_sgn, F * s.eW))) return rc;
    if ((rc = dm_alloc(&d->mem, &s.e_hard, F * s.eW))) return rc;
    if ((rc = dm_alloc(&d->mem, &s.e_unsat, F * s.e_stride))) return rc;
    if ((rc = dm_alloc(&d->mem, &s.e_done_at, F))) return rc;
    if (dm_alloc_pinned(&d->mem, &s.h_done, F * 2)) { qldpc_set_error("edge_create: pinned allocation of %zu bytes failed", sizeof(int) * F * 2); return QLDPC_EHIP; }
    HIPCHK(hipEventCreateWithFlags(&s.e_ev[0], hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&s.e_ev[1], hipEventDisableTiming));
    d->poll_every = 2;
    env_int("QLDPC_POLL_EVERY", &d->poll_every);
    /* measured: replaying the chunks as hipGraphs is not faster than plain launches here (345 vs 321 us per
     * 65 536-VN block; the 2 x ~8 us kernels per iteration are latency-bound on the GPU, not launch-bound on
     * the host), so graphs stay opt-in */
    s.use_graphs = 0; s.graph_frames = -1;
    env_flag("QLDPC_GRAPH", &s.use_graphs);
    /* QLDPC_EDGE_PERSIST=1: the whole decode of up to 8 blocks as ONE launch, one XCD per block (qe_xcd).  Off by default: measured
     * 964 us per 65 536-VN block against 325 us with a launch per pass (a chunk of 64 checks is a chain of dependent L2 round trips,
     * ~8 us, and one XCD has a fifth of the workgroup slots the chunks of a block would fill) */
    s.persist = 0;
    if (const char *e = getenv("QLDPC_EDGE_PERSIST")) s.persist = (atoi(e) && d->cfg.max_frames <= QE_PERSIST_MAX_FRAMES) ? 1 : 0;
    return dm_alloc(&d->mem, &s.e_ctl, QE_CTL_WORDS);      /* claim / rank / barrier / fault words of qe_xcd */
}

/* what is not memory (that is the ledger's: qldpc_decoder_free) */
void edge_destroy(qldpc_decoder *d)
{
    edge_state &s = d->edge;
    for (auto &g : s.e_graphs) if (g) (void)hipGraphExecDestroy(g);
    if (s.cap_stream) (void)hipStreamDestroy(s.cap_stream);
    if (s.e_ev[0]) (void)hipEventDestroy(s.e_ev[0]);
    if (s.e_ev[1]) (void)hipEventDestroy(s.e_ev[1]);
}

/* ------------------------------------------------------------------ launches ----------------- */

/* fn(std::integral_constant<int, S>{}) for the decoder's check-row width: the one place that turns eS into a template argument */
template <typename F>
static auto with_es(const qldpc_decoder *d, F fn)
{
    switch (d->edge.eS) {
    case 8: return fn(std::integral_constant<int, 8>{});
    case 16: return fn(std::integral_constant<int, 16>{});
    case 32: return fn(std::integral_constant<int, 32>{});
    default: return fn(std::integral_constant<int, 64>{});
    }
}

/* the row kernels of the loads: 256 VNs a workgroup, at most 256 workgroups a frame */
static inline dim3 edge_rows_grid(const qldpc_decoder *d) { return dim3((unsigned)std::min((d->N + 255) / 256, 256), (unsigned)d->n_frames); }

template <int S>
static void launch_qe_cn(qldpc_decoder *d, const uint32_t *bits, int slot, int syndrome_only)
{
    const edge_state &s = d->edge;
    dim3 grid((unsigned)((d->M + QE_CPB - 1) / QE_CPB), (unsigned)d->n_frames);
    float *c2v_out = (slot & 1) ? s.e_c2v1 : d->d_b;        /* ping-pong by iteration parity */
    const auto kernel = d->cfg.rule == QLDPC_RULE_SPA ? qe_cn<S, QK_FAM_SPA> : qe_cn<S, QK_FAM_MS>;
    hipLaunchKernelGGL(kernel, grid, dim3(QE_THREADS), 0, d->stream, d->d_a, c2v_out, d->d_cn_ptr, d->d_cn_tr, d->d_cn_var, bits,
                       d->M, d->E, s.eW, s.e_unsat, s.e_stride, slot, s.e_done_at, rule_of(d), syndrome_only, d->has_synd ? s.e_synd : nullptr, words32(d->M));
}
static int edge_cn(qldpc_decoder *d, const uint32_t *bits, int slot, int syndrome_only)
{
    prof_scope ps(d, syndrome_only ? KS_SYND : KS_CN, syndrome_only ? (double)d->E * 4.0 * d->n_frames : bytes_cn(d));
    with_es(d, [&](auto S) { launch_qe_cn<S()>(d, bits, slot, syndrome_only); });
    LAUNCHCHK();
    return QLDPC_OK;
}
/* ite = index of the check pass whose messages are consumed (its parity selects the buffer); sel < 0: per-frame choice */
template <int MODE>
static int edge_vn(qldpc_decoder *d, int ite, int check, int force, float *post_out, int sel)
{
    const edge_state &s = d->edge;
    prof_scope ps(d, KS_VN, bytes_vn(d, MODE));
    dim3 grid((unsigned)((d->N + QE_THREADS - 1) / QE_THREADS), (unsigned)d->n_frames);
    hipLaunchKernelGGL((qe_vn<MODE>), grid, dim3(QE_THREADS), s.e_lds, d->stream, d->d_b, s.e_c2v1, sel, d->cfg.n_ite, d->d_llr, d->d_a, s.e_sgn, s.e_hard, post_out, d->d_vn_ptr,
                       d->N, d->E, s.eW, s.e_unsat, s.e_stride, ite, d->cfg.syndrome_depth, check, s.e_done_at, force);
    LAUNCHCHK();
    return QLDPC_OK;
}

/* launches of iterations [ite0, ite1) on d->stream (+ the decoder-reset prologue in front of iteration 0) */
static int edge_emit(qldpc_decoder *d, int ite0, int ite1)
{
    const edge_state &s = d->edge;
    int rc;
    const int n_ite = d->cfg.n_ite, synd = d->cfg.enable_syndrome;
    if (ite0 == 0) {
        hipLaunchKernelGGL(qe_init, dim3((unsigned)d->n_frames), dim3(64), 0, d->stream, s.e_unsat, s.e_stride, s.e_done_at, d->n_frames);
        LAUNCHCHK();
        if ((rc = edge_vn<QK_VN_FIRST>(d, 0, 0, 0, nullptr, 0))) return rc;
    }
    for (int ite = ite0; ite < ite1; ite++) {
        if ((rc = edge_cn(d, s.e_sgn, ite, 0))) return rc;
        if (ite == n_ite - 1) rc = edge_vn<QK_VN_POST>(d, ite, synd, 0, nullptr, ite & 1);
        else rc = edge_vn<QK_VN_NORMAL>(d, ite, synd, 0, nullptr, ite & 1);
        if (rc) return rc;
    }
    if (ite1 == n_ite + 1) return edge_cn(d, s.e_hard, n_ite + 1, 1);   /* epilogue chunk: success flag of the final hard decisions */
    return QLDPC_OK;
}

/*
 * The launch-bound inner loop as hipGraphs: one instantiated graph per chunk of `poll_every` iterations
 * (kernel arguments differ per iteration, so each chunk has its own graph), captured once per frame count
 * on a private stream and replayed on the caller's stream.  The host only polls between chunks.
 */
static int edge_chunk_graph(qldpc_decoder *d, int chunk, int ite0, int ite1, hipGraphExec_t *out)
{
    edge_state &s = d->edge;
    if (s.graph_frames != d->n_frames) {
        for (auto &g : s.e_graphs) if (g) (void)hipGraphExecDestroy(g);
        s.e_graphs.clear();
        s.graph_frames = d->n_frames;
    }
    if ((int)s.e_graphs.size() <= chunk) s.e_graphs.resize((size_t)chunk + 1, nullptr);
    if (!s.e_graphs[(size_t)chunk]) {
        if (!s.cap_stream) HIPCHK(hipStreamCreateWithFlags(&s.cap_stream, hipStreamNonBlocking));
        hipStream_t user = d->stream;
        d->stream = s.cap_stream;
        hipGraph_t g = nullptr;
        hipError_t e = hipStreamBeginCapture(s.cap_stream, hipStreamCaptureModeRelaxed);
        int rc = QLDPC_EHIP;
        if (e == hipSuccess) {
            rc = edge_emit(d, ite0, ite1);
            e = hipStreamEndCapture(s.cap_stream, &g);
        }
        d->stream = user;
        if (rc) { if (g) (void)hipGraphDestroy(g); return rc; }
        if (e != hipSuccess || !g) { qldpc_set_error("graph capture: %s", hipGetErrorString(e)); return QLDPC_EHIP; }
        hipGraphExec_t x = nullptr;
        e = hipGraphInstantiate(&x, g, nullptr, nullptr, 0);
        (void)hipGraphDestroy(g);
        if (e != hipSuccess) { qldpc_set_error("graph instantiate: %s", hipGetErrorString(e)); return QLDPC_EHIP; }
        s.e_graphs[(size_t)chunk] = x;
    }
    *out = s.e_graphs[(size_t)chunk];
    return QLDPC_OK;
}

template <int S, int FAM>
static int launch_persist(qldpc_decoder *d)
{
    edge_state &s = d->edge;
    const void *fn = (const void *)&qe_xcd<S, FAM>;
    const size_t lds = std::max((size_t)(2 * QE_MAX_EDGES + 16 + QE_CPB) * sizeof(float), s.e_lds);
    if (s.persist_blocks == 0) {
        int per_cu = 0, cus = 0;
        if (lds > 48 * 1024) HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, QE_THREADS, lds));
        HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, d->device));
        /* workgroups that can be resident on ONE XCD (an eighth of the CUs); the occupancy query is advisory (it can over-report by one
         * workgroup per CU), so one per CU is given away and at most 4 are counted on */
        const int reported = per_cu;
        per_cu = std::min(4, per_cu - 1);
        s.persist_blocks = per_cu * (cus / 8);
        env_int("QLDPC_EDGE_WGS", &s.persist_blocks);      /* workgroups per block (experiments) */
        if (getenv("QLDPC_DEBUG")) fprintf(stderr, "libqldpc: one-launch edge decode: occupancy query %d workgroups per CU, %d CUs, %d workgroups per block, %zu B LDS\n", reported, cus, s.persist_blocks, lds);
        if (s.persist_blocks < 1 || cus < 8) { s.persist = 0; return QLDPC_EUNSUPPORTED; }
    }
    const int nCN = (d->M + QE_CPB - 1) / QE_CPB, nVN = (d->N + QE_THREADS - 1) / QE_THREADS;
    const int nb = std::max(1, std::min(s.persist_blocks, std::max(nCN, nVN))), F = d->n_frames;
    static const int ctl_init[QE_CTL_WORDS] = {-1, -1, -1, -1, -1, -1, -1, -1};      /* the rest zero */
    HIPCHK(hipMemcpyAsync(s.e_ctl, ctl_init, sizeof(ctl_init), hipMemcpyHostToDevice, d->stream));
    /* twice the workgroups the 8 XCDs could use: the surplus (and the whole share of an XCD that got no block) exits at once */
    const unsigned grid = (unsigned)(8 * nb * 2);
    hipLaunchKernelGGL((qe_xcd<S, FAM>), dim3(grid), dim3(QE_THREADS), lds, d->stream, d->d_a, d->d_b, s.e_c2v1, d->d_llr, d->d_cn_ptr, d->d_cn_tr, d->d_cn_var, d->d_vn_ptr, s.e_sgn, s.e_hard,
                       d->N, d->M, d->E, s.eW, F, nb, d->cfg.n_ite, d->cfg.enable_syndrome, d->cfg.syndrome_depth, s.e_unsat, s.e_stride, s.e_done_at, rule_of(d),
                       d->has_synd ? s.e_synd : nullptr, words32(d->M), s.e_ctl);
    LAUNCHCHK();
    /* the host needs the verdict now anyway (the launch-per-pass path polls as well): read the control words back; a decode that did
     * not complete (a workgroup that never became resident: the grid drains on its bounded waits and says so) is repeated with a
     * launch per pass by the caller, and the one-launch path is switched off for this decoder */
    int ctl_h[QE_CTL_WORDS];
    HIPCHK(hipMemcpyAsync(ctl_h, s.e_ctl, sizeof(ctl_h), hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    if (ctl_h[QE_CTL_FAULT] || ctl_h[QE_CTL_NEXT] < F) {
        fprintf(stderr, "libqldpc: one-launch edge decode did not complete (barrier time-out %d, %d of %d blocks claimed): falling back to a launch per pass\n",
                ctl_h[QE_CTL_FAULT], ctl_h[QE_CTL_NEXT], F);
        s.persist = 0;
        return QLDPC_EUNSUPPORTED;
    }
    d->last_iters = ctl_h[QE_CTL_ITERS];
    return QLDPC_OK;
}

static int run_edges_persist(qldpc_decoder *d)
{
    const bool spa = d->cfg.rule == QLDPC_RULE_SPA;
    return with_es(d, [&](auto S) { return spa ? launch_persist<S(), QK_FAM_SPA>(d) : launch_persist<S(), QK_FAM_MS>(d); });
}

int edge_run(qldpc_decoder *d)
{
    edge_state &s = d->edge;
    int rc;
    if (s.persist && !d->prof_on && d->n_frames <= QE_PERSIST_MAX_FRAMES) {
        rc = run_edges_persist(d);
        if (rc != QLDPC_EUNSUPPORTED) return rc;      /* not co-resident on this device: the launch-per-pass path below */
    }
    const int n_ite = d->cfg.n_ite, F = d->n_frames, synd = d->cfg.enable_syndrome;
    const int P = (synd && d->poll_every > 0) ? d->poll_every : n_ite;
    const bool graphs = s.use_graphs && !d->prof_on;
    int ite = 0, pending = -1, flip = 0, chunk = 0;
    while (ite < n_ite) {
        const int ite1 = std::min(n_ite, ite + P);
        if (graphs) {
            hipGraphExec_t x;
            if ((rc = edge_chunk_graph(d, chunk, ite, ite1, &x))) return rc;
            HIPCHK(hipGraphLaunch(x, d->stream));
        } else if ((rc = edge_emit(d, ite, ite1))) return rc;
        ite = ite1; chunk++;
        if (synd && ite < n_ite) {
            /* look-ahead polling: wait for the snapshot queued one chunk ago, so the GPU always has work queued */
            if (pending >= 0) {
                HIPCHK(hipEventSynchronize(s.e_ev[pending]));
                bool all = true;
                for (int f = 0; f < F; f++) all = all && s.h_done[(size_t)pending * F + f] >= 0;
                if (all) break;
            }
            HIPCHK(hipMemcpyAsync(s.h_done + (size_t)flip * F, s.e_done_at, sizeof(int) * (size_t)F, hipMemcpyDeviceToHost, d->stream));
            HIPCHK(hipEventRecord(s.e_ev[flip], d->stream));
            pending = flip; flip ^= 1;
        }
    }
    d->last_iters = ite;
    /* success flag: syndrome of the final hard decisions into the last slot */
    return edge_cn(d, s.e_hard, n_ite + 1, 1);
}

/* ------------------------------------------------------------------ load --------------------- */

int edge_load_llr(qldpc_decoder *d, const float *d_llr)
{
    prof_scope ps(d, KS_LOAD, 2.0 * d->N * 4.0 * d->n_frames);
    HIPCHK(hipMemcpyAsync(d->d_llr, d_llr, sizeof(float) * (size_t)d->n_frames * d->N, hipMemcpyDeviceToDevice, d->stream));
    end_load(d);
    return QLDPC_OK;
}

int edge_load_bits(qldpc_decoder *d, const uint32_t *d_bits, const float *d_llr_mag, const uint8_t *d_vn_class, const int *d_n_channel)
{
    const int W = d->edge.eW;
    prof_scope ps(d, KS_LOAD, ((double)W * 4.0 + d->N * 4.0) * d->n_frames);
    hipLaunchKernelGGL(qe_load_bits, edge_rows_grid(d), dim3(256), 0, d->stream, d_bits, d_llr_mag, d_vn_class, d->d_llr, d->N, W, d_n_channel);
    LAUNCHCHK();
    end_load(d);
    return QLDPC_OK;
}

int edge_load_syndrome(qldpc_decoder *d, const uint32_t *d_synd_bits)
{
    edge_state &s = d->edge;
    const int Wm = words32(d->M);
    int rc;
    if (!s.e_synd && (rc = dm_alloc(&d->mem, &s.e_synd, (size_t)d->cfg.max_frames * Wm))) return rc;
    HIPCHK(hipMemcpyAsync(s.e_synd, d_synd_bits, sizeof(uint32_t) * (size_t)d->n_frames * Wm, hipMemcpyDeviceToDevice, d->stream));
    d->has_synd = 1; d->ran = 0;
    return QLDPC_OK;
}

int edge_erase(qldpc_decoder *d, const uint32_t *d_erase_bits)
{
    hipLaunchKernelGGL(qe_erase, edge_rows_grid(d), dim3(256), 0, d->stream, d_erase_bits, d->d_llr, d->N, d->edge.eW);
    LAUNCHCHK();
    d->ran = 0;
    return d->has_known ? edge_known(d) : (int)QLDPC_OK;      /* known wins over erased */
}

/* the masks qldpc_load_known_dev keeps in d_known, onto the rows of d_llr */
int edge_known(qldpc_decoder *d)
{
    const int W = d->edge.eW;
    const uint32_t *kn = d->d_known, *val = d->d_known + (size_t)d->cfg.max_frames * W;
    hipLaunchKernelGGL(qe_known, edge_rows_grid(d), dim3(256), 0, d->stream, kn, val, d->d_llr, d->N, W);
    LAUNCHCHK();
    return QLDPC_OK;
}

/* ------------------------------------------------------------------ fetch -------------------- */

int edge_fetch_packed(qldpc_decoder *d, uint32_t *d_out)
{
    HIPCHK(hipMemcpyAsync(d_out, d->edge.e_hard, sizeof(uint32_t) * (size_t)d->n_frames * d->edge.eW, hipMemcpyDeviceToDevice, d->stream));
    return QLDPC_OK;
}

int edge_fetch_info(qldpc_decoder *d, int *d_V_K)
{
    dim3 grid((unsigned)std::max(1, std::min((d->K + 255) / 256, 64)), (unsigned)d->n_frames);
    hipLaunchKernelGGL(qe_fetch_info, grid, dim3(256), 0, d->stream, d->edge.e_hard, d->d_info_pos, d_V_K, d->K, d->edge.eW);
    LAUNCHCHK();
    return QLDPC_OK;
}

int edge_fetch_status(qldpc_decoder *d, int *d_iters, int *d_ok)
{
    const edge_state &s = d->edge;
    dim3 grid((unsigned)((d->n_frames + 255) / 256));
    hipLaunchKernelGGL(qe_status_out, grid, dim3(256), 0, d->stream, s.e_unsat, s.e_stride, d->cfg.n_ite + 1, s.e_done_at, d->cfg.n_ite, d_iters, d_ok, d->n_frames);
    LAUNCHCHK();
    return QLDPC_OK;
}

/* posterior of the last executed check pass, written frame-major directly (exact in fixed-iteration mode) */
int edge_fetch_post(qldpc_decoder *d, float *d_post_out)
{
    return edge_vn<QK_VN_POST>(d, 0, 0, 1, d_post_out, -1);
}
