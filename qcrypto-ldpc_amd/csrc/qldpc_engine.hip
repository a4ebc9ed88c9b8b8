/*
 * qldpc_engine.hip -- decoder object, launch sequencing and the C ABI of the batched BP decoder.
 *
 * Mirrors module::Decoder_LDPC_BP_flooding / _horizontal_layered / _vertical_layered as the reference harness drives
 * them (BS/src/main.cpp:193,365,389; VAR/main.cpp (alist-v1.0.1):179-256,438): create(K, N, n_ite,
 * H, info_bits_pos, rule, enable_syndrome, syndrome_depth, n_frames), decode_siho(Y_N, V_K), reset().
 * Everything heavy is a HIP kernel from qldpc_kernels.h; there is no CPU fallback.  The FRAMES engine (lanes over frames) lives here; a
 * decoder of the edge-parallel engine leaves every entry point for qldpc_engine_edge.hip after the argument and state checks.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <optional>
#include <type_traits>
#include <vector>

#include "qldpc_engine_int.h"
#include "qldpc_kernels_chain.h"
#include "qldpc_kernels_compact.h"
#include "qldpc_kernels_fpost.h"
#include "qldpc_kernels_weakest.h"

extern "C" int qldpc_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

/* ------------------------------------------------------------------ bandwidth probe ---------- */

/* What this device sustains for the access shape the decoder is made of: 256-byte rows, one dword per lane, non-temporal, read + written
 * once.  bench.py prints it next to the kernels' rates (the 8 TB/s of the data sheet is not reachable by any kernel: DESIGN section 3.1). */
typedef float qk_probe_f4 __attribute__((ext_vector_type(4)));
template <int ROWS, bool WIDE>
static __global__ __launch_bounds__(256) void qk_copy_probe(const float *__restrict__ src, float *__restrict__ dst, size_t n_rows)
{
    /* one wavefront per ROWS consecutive 256-byte rows (WIDE: ROWS / 4 KiB-rows), every load issued before the first store: the shape of a
     * variable-node pass without its arithmetic */
    const int lane = threadIdx.x & 63;
    const size_t r0 = ((size_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * ROWS;
    if (r0 >= n_rows) return;
    if constexpr (WIDE) {
        qk_probe_f4 v[ROWS / 4];
#pragma unroll
        for (int k = 0; k < ROWS / 4; k++) v[k] = __builtin_nontemporal_load(reinterpret_cast<const qk_probe_f4 *>(src + (r0 + 4 * k) * 64) + lane);
#pragma unroll
        for (int k = 0; k < ROWS / 4; k++) __builtin_nontemporal_store(v[k], reinterpret_cast<qk_probe_f4 *>(dst + (r0 + 4 * k) * 64) + lane);
    } else {
        float v[ROWS];
#pragma unroll
        for (int k = 0; k < ROWS; k++) v[k] = __builtin_nontemporal_load(src + (r0 + k) * 64 + lane);
#pragma unroll
        for (int k = 0; k < ROWS; k++) __builtin_nontemporal_store(v[k], dst + (r0 + k) * 64 + lane);
    }
}

extern "C" int qldpc_copy_probe(int device, size_t bytes, int reps, int wide, double *gbytes_per_s)
{
    int ndev = 0;
    if (!gbytes_per_s || reps < 1 || bytes < (1u << 20)) return QLDPC_EINVAL;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { qldpc_set_error("no HIP device visible: libqldpc has no CPU fallback"); return QLDPC_ENODEV; }
    if (device < 0 || device >= ndev) return QLDPC_ENODEV;
    HIPCHK(hipSetDevice(device));
    const size_t n_rows = bytes / 256 / 64 * 64;      /* whole workgroups of 4 x 16 rows */
    const unsigned blocks = (unsigned)(n_rows / 64);
    float *a = nullptr, *b = nullptr;
    dm_scope tmp;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    int rc = QLDPC_OK;
    float ms = 0.0f;
    if (dm_alloc(&tmp.m, &a, n_rows * 64) || dm_alloc(&tmp.m, &b, n_rows * 64)) { rc = QLDPC_ENOMEM; goto out; }
    if (hipMemset(a, 0, n_rows * 256) != hipSuccess || hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) { rc = QLDPC_EHIP; goto out; }
    if (wide) hipLaunchKernelGGL((qk_copy_probe<16, true>), dim3(blocks), dim3(256), 0, 0, a, b, n_rows);      /* warm-up */
    else hipLaunchKernelGGL((qk_copy_probe<16, false>), dim3(blocks), dim3(256), 0, 0, a, b, n_rows);
    (void)hipEventRecord(e0, 0);
    for (int i = 0; i < reps; i++) {
        const float *from = (i & 1) ? b : a;
        float *to = (i & 1) ? a : b;
        if (wide) hipLaunchKernelGGL((qk_copy_probe<16, true>), dim3(blocks), dim3(256), 0, 0, from, to, n_rows);
        else hipLaunchKernelGGL((qk_copy_probe<16, false>), dim3(blocks), dim3(256), 0, 0, from, to, n_rows);
    }
    (void)hipEventRecord(e1, 0);
    if (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess || hipGetLastError() != hipSuccess) { rc = QLDPC_EHIP; goto out; }
    *gbytes_per_s = 2.0 * (double)(n_rows * 256) * reps / ((double)ms * 1e-3) / 1e9;
out:
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (rc == QLDPC_EHIP) qldpc_set_error("copy probe: HIP error");
    return rc;
}

/* ------------------------------------------------------------------ decoder object ----------- */

QLDPC_DECLARE_LAUNCH(1)
QLDPC_DECLARE_LAUNCH(2)
QLDPC_DECLARE_LAUNCH(4)

static const int CN_CAPS[] = {8, 12, 20, 40};
static constexpr int VN_CAPS[] = {4, 12};
static_assert(VN_CAPS[1] == QK_FPV_DMAX, "qk_vn_fpost has a body for every degree of the register-resident VN buckets, the cap-0 bucket holds the rest");

static int make_buckets(qldpc_decoder *d, const int *ptr, const int *ids, int n_ids, const int *caps, int n_caps, std::vector<bucket> &out, const int *var = nullptr)
{
    std::vector<std::vector<int>> lists(n_caps + 1);
    for (int i = 0; i < n_ids; i++) {
        const int id = ids ? ids[i] : i;
        const int deg = ptr[id + 1] - ptr[id];
        int b = n_caps;
        for (int k = 0; k < n_caps; k++) if (deg <= caps[k]) { b = k; break; }
        lists[b].push_back(id);
    }
    for (int k = 0; k <= n_caps; k++) {
        if (lists[k].empty()) continue;
        bucket bk;
        bk.cap = k < n_caps ? caps[k] : 0;
        bk.n = (int)lists[k].size();
        bk.d_rec = nullptr;
        int rc = dm_alloc(&d->mem, &bk.d_list, lists[k].size());
        if (rc != QLDPC_OK) return rc;
        out.push_back(bk);
        HIPCHK(hipMemcpy(bk.d_list, lists[k].data(), lists[k].size() * sizeof(int), hipMemcpyHostToDevice));
        if (var && bk.cap > 0) {      /* the list once more as records {id, first edge, degree, 0, var[0 .. cap)} (padding: VN 0, never asked for) */
            const size_t stride = (size_t)(QK_REC_HDR + bk.cap);
            std::vector<int> rec(lists[k].size() * stride, 0);
            for (size_t i = 0; i < lists[k].size(); i++) {
                const int id = lists[k][i], b = ptr[id], deg = ptr[id + 1] - b;
                int *r = rec.data() + i * stride;
                r[0] = id; r[1] = b; r[2] = deg;
                for (int e = 0; e < deg; e++) r[QK_REC_HDR + e] = var[b + e];
            }
            rc = dm_alloc(&d->mem, &bk.d_rec, rec.size());
            if (rc != QLDPC_OK) return rc;
            out.back().d_rec = bk.d_rec;
            HIPCHK(hipMemcpy(bk.d_rec, rec.data(), rec.size() * sizeof(int), hipMemcpyHostToDevice));
        }
    }
    return QLDPC_OK;
}

/* the VNs 0 .. n_vn - 1 of degree <= QK_FPV_DMAX (the register-resident buckets of VN_CAPS) by exact degree, as the records of qk_vn_fpost
 * (engine_int.h: fp_vn_class); vn_row = vn_tr.  VNs of a higher degree stay with the cap-0 bucket of the caller's list */
static int make_fp_vn_classes(qldpc_decoder *d, const int *vn_ptr, int n_vn, const int *vn_row, std::vector<fp_vn_class> &out)
{
    std::vector<std::vector<int>> recs(QK_FPV_DMAX + 1);
    for (int v = 0; v < n_vn; v++) {
        const int b = vn_ptr[v], deg = vn_ptr[v + 1] - b;
        if (deg > QK_FPV_DMAX) continue;
        std::vector<int> &r = recs[(size_t)deg];
        const size_t at = r.size();
        r.resize(at + (size_t)QK_FPV_STRIDE(deg), 0);      /* padding: row 0, never asked for */
        r[at] = v;
        for (int e = 0; e < deg; e++) r[at + 1 + (size_t)e] = vn_row[b + e];
    }
    for (int deg = 0; deg <= QK_FPV_DMAX; deg++) {
        const std::vector<int> &r = recs[(size_t)deg];
        if (r.empty()) continue;
        fp_vn_class c{deg, (int)(r.size() / (size_t)QK_FPV_STRIDE(deg)), nullptr};
        int rc = dm_alloc(&d->mem, &c.d_rec, r.size());
        if (rc != QLDPC_OK) return rc;
        out.push_back(c);
        HIPCHK(hipMemcpy(c.d_rec, r.data(), r.size() * sizeof(int), hipMemcpyHostToDevice));
    }
    return QLDPC_OK;
}

extern "C" void qldpc_decoder_cfg_default(qldpc_decoder_cfg *cfg)
{
    if (!cfg) return;
    memset(cfg, 0, sizeof(*cfg));
    cfg->schedule = QLDPC_SCHED_FLOODING;
    cfg->rule = QLDPC_RULE_SPA;        /* the harness default, BS/src/main.cpp:193 */
    cfg->rule_param = 0.0f;
    cfg->n_ite = 100;                  /* BS/src/main.cpp:95-104 */
    cfg->enable_syndrome = 1;
    cfg->syndrome_depth = 1;
    cfg->max_frames = 1;
    cfg->device = 0;
    cfg->frames_per_lane = 0;
}

static void view_reset(qldpc_decoder *d);

extern "C" void qldpc_decoder_free(qldpc_decoder *d)
{
    if (!d) return;
    (void)hipSetDevice(d->device);
    view_reset(d);
    if (d->stream) (void)hipStreamSynchronize(d->stream); else (void)hipDeviceSynchronize();
    for (auto &r : d->prof_pending) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    edge_destroy(d);
    dm_free_all(&d->mem);
    delete d;
}

static int frames_create(qldpc_decoder *d, const qldpc_code *code);

static int create_impl(const qldpc_code *code, int K, const int *info_bits_pos, const qldpc_decoder_cfg *cfg, qldpc_decoder *d)
{
    d->cfg = *cfg;
    d->N = code->N; d->M = code->M; d->E = code->E; d->K = K;
    d->device = cfg->device;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { qldpc_set_error("no HIP device visible: libqldpc has no CPU fallback"); return QLDPC_ENODEV; }
    if (cfg->device < 0 || cfg->device >= ndev) { qldpc_set_error("device %d out of range (%d visible)", cfg->device, ndev); return QLDPC_ENODEV; }
    HIPCHK(hipSetDevice(cfg->device));
    int V = cfg->frames_per_lane;
    if (V == 0) V = (cfg->msg_dtype == 1) ? 2 : 1;      /* fp16 storage: 2 frames per lane keep the rows at 256 bytes; measured on MI355X: 256-byte rows (V = 1) are 2-5 % faster than V = 2 / 4 at every batch size, and exit earlier */
    if (const char *e = getenv("QLDPC_FRAMES_PER_LANE")) { int x = atoi(e); if (x == 1 || x == 2 || x == 4) V = x; }
    if (cfg->msg_dtype == 2) V = QI_V;                   /* 8-bit messages: the four frames of a lane are the four bytes of a dword */
    d->V = V; d->FG = 64 * V; d->G = (cfg->max_frames + d->FG - 1) / d->FG;
    d->freeze = cfg->freeze_messages ? 1 : 0;
    env_flag("QLDPC_FREEZE", &d->freeze);
    /* early exit: the host looks at the active-group counter every 2 iterations once an iteration is long enough to hide the
     * ~30 us round trip (>= 2e7 message updates); small decodes run their iterations as early-returning launches instead */
    d->poll_every = (d->G >= 8 || (double)d->E * d->G * d->FG >= 2e7) ? 2 : 0;
    env_int("QLDPC_POLL_EVERY", &d->poll_every);

    int rc;
    if ((rc = dm_alloc(&d->mem, &d->d_cn_ptr, (size_t)d->M + 1))) return rc;
    if ((rc = dm_alloc(&d->mem, &d->d_cn_tr, (size_t)d->E + QK_IDX_PAD))) return rc;
    if ((rc = dm_alloc(&d->mem, &d->d_cn_var, (size_t)d->E + QK_IDX_PAD))) return rc;
    HIPCHK(hipMemset(d->d_cn_tr, 0, sizeof(int) * ((size_t)d->E + QK_IDX_PAD)));
    HIPCHK(hipMemset(d->d_cn_var, 0, sizeof(int) * ((size_t)d->E + QK_IDX_PAD)));
    if ((rc = dm_alloc(&d->mem, &d->d_vn_ptr, (size_t)d->N + 1))) return rc;
    if ((rc = dm_alloc(&d->mem, &d->d_info_pos, (size_t)K))) return rc;
    HIPCHK(hipMemcpy(d->d_cn_ptr, code->cn_ptr, sizeof(int) * ((size_t)d->M + 1), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d->d_cn_tr, code->transpose, sizeof(int) * (size_t)d->E, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d->d_cn_var, code->cn_var, sizeof(int) * (size_t)d->E, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d->d_vn_ptr, code->vn_ptr, sizeof(int) * ((size_t)d->N + 1), hipMemcpyHostToDevice));
    {   /* chk_to_var of the frames engine is CN-major: the variable-node passes find the row of slot s at vn_tr[s] */
        std::vector<int> vt((size_t)d->E + QK_IDX_PAD, 0);
        for (int k = 0; k < d->E; k++) vt[(size_t)code->transpose[k]] = k;
        if ((rc = dm_alloc(&d->mem, &d->d_vn_tr, vt.size()))) return rc;
        HIPCHK(hipMemcpy(d->d_vn_tr, vt.data(), sizeof(int) * vt.size(), hipMemcpyHostToDevice));
    }
    {   /* check -> VN table transposed to [edge position][check] for the syndrome pass (qk_syndrome) */
        d->max_dc = code->max_dc;
        std::vector<int> t((size_t)std::max(1, code->max_dc) * d->M, -1);
        for (int c = 0; c < d->M; c++)
            for (int k = code->cn_ptr[c]; k < code->cn_ptr[c + 1]; k++) t[(size_t)(k - code->cn_ptr[c]) * d->M + c] = code->cn_var[k];
        if ((rc = dm_alloc(&d->mem, &d->d_cn_var_t, t.size()))) return rc;
        HIPCHK(hipMemcpy(d->d_cn_var_t, t.data(), sizeof(int) * t.size(), hipMemcpyHostToDevice));
    }
    {
        std::vector<int> pos((size_t)K);
        for (int i = 0; i < K; i++) {
            pos[i] = info_bits_pos ? info_bits_pos[i] : i;
            if (pos[i] < 0 || pos[i] >= d->N) { qldpc_set_error("info_bits_pos[%d] = %d out of range", i, pos[i]); return QLDPC_EINVAL; }
        }
        HIPCHK(hipMemcpy(d->d_info_pos, pos.data(), sizeof(int) * (size_t)K, hipMemcpyHostToDevice));
    }
    for (int k = 0; k < KS_COUNT; k++) { memset(&d->stats[k], 0, sizeof(d->stats[k])); snprintf(d->stats[k].name, sizeof(d->stats[k].name), "%s", ks_names[k]); }
    /* engine choice: lanes over frames (batch) or lanes over edges (one block at a time) */
    {
        const bool edge_ok = edge_supports(cfg, code);
        int eng = cfg->engine;
        if (const char *e = getenv("QLDPC_ENGINE")) { int x = atoi(e); if (x >= 0 && x <= 2) eng = x; }
        if (eng == QLDPC_ENGINE_EDGES && !edge_ok) {
            qldpc_set_error("edge-parallel engine needs flooding, MS/OMS/NMS/SPA, check degree <= 64 (have %d) and VN degree <= %d (have %d)", code->max_dc, edge_max_dv(), code->max_dv);
            return QLDPC_EUNSUPPORTED;
        }
        if (cfg->giveup_patience > 0) {      /* the syndrome weights are counted by the FRAMES engine's test */
            if (eng == QLDPC_ENGINE_EDGES) { qldpc_set_error("giveup_patience needs the FRAMES engine: create the decoder with engine = FRAMES (or auto)"); return QLDPC_EUNSUPPORTED; }
            eng = QLDPC_ENGINE_FRAMES;
        }
        if (eng == QLDPC_ENGINE_AUTO) eng = (edge_ok && cfg->max_frames <= 8) ? QLDPC_ENGINE_EDGES : QLDPC_ENGINE_FRAMES;
        d->engine = eng;
        d->msg_half = cfg->msg_dtype == 1;
        env_flag("QLDPC_MSG_HALF", &d->msg_half);
        d->packed_h16 = 1;
        env_flag("QLDPC_PACKED_H16", &d->packed_h16);
        d->msg_i8 = cfg->msg_dtype == 2;
        d->quant_scale = cfg->quant_scale > 0.0f ? cfg->quant_scale : 8.0f;      /* measured on the config-2 code: FER at QBER 3.0 % 0.097 (fp32) / 0.119 (scale 8) / 0.168 (scale 4) */
        if (d->msg_i8) {
            if (cfg->rule > QLDPC_RULE_NMS || cfg->engine == QLDPC_ENGINE_EDGES || cfg->freeze_messages ||
                (cfg->frames_per_lane != 0 && cfg->frames_per_lane != QI_V)) {
                qldpc_set_error("8-bit messages are implemented for MS/OMS/NMS on the FRAMES engine (frames_per_lane 0 or 4, freeze_messages 0)");
                return QLDPC_EUNSUPPORTED;
            }
            if (code->max_dv > 256) { qldpc_set_error("8-bit messages: VN degree %d > 256 would overflow the 16-bit posterior", code->max_dv); return QLDPC_EUNSUPPORTED; }
            d->engine = eng = QLDPC_ENGINE_FRAMES;
            d->msg_half = 0;
        }
        if (d->msg_half && (eng != QLDPC_ENGINE_FRAMES || cfg->schedule != QLDPC_SCHED_FLOODING)) {
            if (cfg->engine == QLDPC_ENGINE_AUTO && cfg->schedule == QLDPC_SCHED_FLOODING) d->engine = QLDPC_ENGINE_FRAMES;
            else { qldpc_set_error("fp16 message storage is implemented for the flooding schedule on the FRAMES engine"); return QLDPC_EUNSUPPORTED; }
        }
    }
    return d->engine == QLDPC_ENGINE_EDGES ? edge_create(d, code) : frames_create(d, code);
}

/* the FRAMES engine's share of create_impl: the lists of its schedule, the message and per-frame arrays [G][..][FG], early exit and compaction */
static int frames_create(qldpc_decoder *d, const qldpc_code *code)
{
    const qldpc_decoder_cfg *cfg = &d->cfg;
    const int V = d->V;
    int rc;
    bool chain_asked = false;      /* horizontal layered: the one-launch sweep was asked for */
    if (cfg->schedule == QLDPC_SCHED_FLOODING) {
        if ((rc = make_buckets(d, code->cn_ptr, nullptr, d->M, CN_CAPS, 4, d->cn_buckets))) return rc;
        if ((rc = make_buckets(d, code->vn_ptr, nullptr, d->N, VN_CAPS, 2, d->vn_buckets))) return rc;
    } else if (cfg->schedule == QLDPC_SCHED_VLAYERED) {
        /* one VN list per class of the code's vlayer order (built on first use); the kernel walks list -> vn_ptr -> {vn_chk, vn_tr} -> cn_ptr -> cn_var */
        const int n_cls = qldpc_code_vlayer_count(code);
        if (n_cls < 0) return n_cls;
        for (int l = 0; l < n_cls; l++)
            if ((rc = make_buckets(d, code->vn_ptr, code->vlayer_order + code->vlayer_ptr[l], code->vlayer_ptr[l + 1] - code->vlayer_ptr[l], nullptr, 0, d->vlayer_classes))) return rc;
        if ((rc = dm_alloc(&d->mem, &d->d_vn_chk, (size_t)d->E))) return rc;
        HIPCHK(hipMemcpy(d->d_vn_chk, code->vn_chk, sizeof(int) * (size_t)d->E, hipMemcpyHostToDevice));
        double dc2 = 0.0;
        for (int c = 0; c < d->M; c++) { const double dc = code->cn_ptr[c + 1] - code->cn_ptr[c]; dc2 += dc * dc; }
        d->vl_rows = 2.0 * dc2 + 2.0 * d->N;
    } else {
        d->n_layers = code->n_layers;
        d->layer_buckets.resize((size_t)code->n_layers);
        /* QLDPC_LAYER_REC=0: the layer kernels walk list -> cn_ptr -> cn_var as in rounds 1 - 2 (A/B) */
        const char *rec_env = getenv("QLDPC_LAYER_REC");
        const int *rec_var = (rec_env && atoi(rec_env) == 0) ? nullptr : code->cn_var;
        for (int l = 0; l < code->n_layers; l++)
            if ((rc = make_buckets(d, code->cn_ptr, code->layer_order + code->layer_ptr[l], code->layer_ptr[l + 1] - code->layer_ptr[l], CN_CAPS, 4, d->layer_buckets[(size_t)l], rec_var))) return rc;
        /* A sweep as ONE launch in which a check waits for the earlier checks on its own VNs instead of for the whole layer before it
         * (qldpc_kernels_chain.h).  fp32 messages, 64-frame groups, messages never frozen, check degree <= 40.  Measured on the N = 10^6 code
         * (fixed 50 sweeps, fraction of the HBM peak, launch per layer -> one launch): 64 frames 0.575 -> 0.566, 128: 0.62 -> 0.68, 256: 0.63 -> 0.71,
         * 512: 0.67 -> 0.70, 1 024: 0.69 -> 0.69 (early exit loses from 512 frames on: finished groups still draw tickets); config-2 batch (64
         * groups, 437 checks per layer) 1 528 -> 1 300 Mbit/s; four session decoders side by side 19.0 -> 23.9 ms; with the per-sweep early exit the gain
         * at 128 - 256 frames is inside the run-to-run spread (+2 % .. -9 %).  So: auto = fixed-iteration runs with 2 .. 8 groups and a layer launch of
         * 8 192 .. 65 535 waves; cfg.layer_chain / QLDPC_LAYER_CHAIN = 1 / 0 force it on / off.  (Fewer or more waves in flight per SIMD,
         * QLDPC_CHAIN_WAVES: no difference outside the box-to-box spread, tools/gpu/r3_g47.sh.)  It works on explicit messages: the min-sum rules,
         * which run on the compressed check state below, do not use it. */
        /* Min-sum and AMS sweeps on a compressed check state (qldpc_kernels_cst.h): bit-identical, 0.59 x the bytes on the N = 10^6 code.  fp32 messages,
         * 64-frame groups, messages never frozen, check degree <= 32, and the state must fit the message array.  QLDPC_LAYER_CST = 0 keeps the dc messages. */
        d->layer_cst = 0;
        const char *chain_env = getenv("QLDPC_LAYER_CHAIN");
        chain_asked = chain_env ? atoi(chain_env) != 0 : cfg->layer_chain == 1;      /* an explicit request for the one-launch sweep keeps the explicit messages it works on */
        if (!chain_asked && !d->msg_i8 && !d->msg_half && d->V == 1 && !d->freeze && (family_of(cfg->rule) == QK_FAM_MS || family_of(cfg->rule) == QK_FAM_AMS) && d->max_dc <= 32 &&
            (size_t)d->M * 1024 <= (size_t)d->E * 256)
            d->layer_cst = 1;
        if (const char *e = getenv("QLDPC_LAYER_CST")) d->layer_cst = d->layer_cst && atoi(e) != 0;
        d->chain = 0;
        {
            const long per_layer = (long)d->M / std::max(1, code->n_layers) * d->G;
            bool want = !cfg->enable_syndrome && d->G >= 2 && d->G <= 8 && per_layer >= 8192 && per_layer < 65536 && code->n_layers > 1;
            if (cfg->layer_chain == 1) want = true;
            if (cfg->layer_chain == 2) want = false;
            if (const char *e = getenv("QLDPC_LAYER_CHAIN")) want = atoi(e) != 0;
            if (want && !d->layer_cst && !d->msg_i8 && !d->msg_half && d->V == 1 && !d->freeze && d->max_dc <= 40 && (long)d->M * d->G < (1L << 30) / 64) {
                std::vector<int> depv((size_t)d->E), seen((size_t)d->N, 0), chain_order((size_t)d->M), lastpos((size_t)d->N, -1);
                /* Execution order of the one-launch sweep: the code's layers in their order (so every VN sees its checks in the order of the
                 * launch-per-layer sweep and of the oracle), but INSIDE a layer -- whose checks share no VN, so their order is free -- the checks
                 * whose predecessors sit early in the order go first.  The waves in flight cover a window of a few thousand consecutive
                 * tickets; with the layer in arbitrary order 4 in 10 checks found a predecessor from the tail of the layer before still in that
                 * window and had to wait for it, sorted this way a check's predecessors are about one whole layer behind it. */
                {
                    std::vector<std::pair<int, int>> keyed;
                    int at = 0;
                    for (int l = 0; l < code->n_layers; l++) {
                        keyed.clear();
                        for (int i = code->layer_ptr[l]; i < code->layer_ptr[l + 1]; i++) {
                            const int c = code->layer_order[i];
                            int key = -1;
                            for (int k = code->cn_ptr[c]; k < code->cn_ptr[c + 1]; k++) key = std::max(key, lastpos[(size_t)code->cn_var[k]]);
                            keyed.emplace_back(key, c);
                        }
                        std::stable_sort(keyed.begin(), keyed.end(), [](const std::pair<int, int> &x, const std::pair<int, int> &y) { return x.first < y.first; });
                        for (auto &kc : keyed) {
                            const int c = kc.second;
                            chain_order[(size_t)at] = c;
                            for (int k = code->cn_ptr[c]; k < code->cn_ptr[c + 1]; k++) lastpos[(size_t)code->cn_var[k]] = at;
                            at++;
                        }
                    }
                }
                /* rank of check c among the checks of VN v in execution order: walk the checks in that order, count per VN */
                for (int p = 0; p < d->M; p++) {
                    const int c = chain_order[(size_t)p];
                    for (int k = code->cn_ptr[c]; k < code->cn_ptr[c + 1]; k++) {
                        const int v = code->cn_var[k];
                        const int dv = code->vn_ptr[v + 1] - code->vn_ptr[v];
                        depv[(size_t)k] = (dv << 16) | seen[(size_t)v]++;
                    }
                }
                if (code->max_dv < 32768) {
                    if ((rc = dm_alloc(&d->mem, &d->d_chain_order, (size_t)d->M)) || (rc = dm_alloc(&d->mem, &d->d_chain_dep, (size_t)d->E)) ||
                        (rc = dm_alloc(&d->mem, &d->d_chain_ver, (size_t)d->G * d->N)) || (rc = dm_alloc(&d->mem, &d->d_chain_ctl, QC_CTL_WORDS))) return rc;
                    HIPCHK(hipMemcpy(d->d_chain_order, chain_order.data(), sizeof(int) * (size_t)d->M, hipMemcpyHostToDevice));
                    HIPCHK(hipMemcpy(d->d_chain_dep, depv.data(), sizeof(int) * (size_t)d->E, hipMemcpyHostToDevice));
                    d->chain = 1;
                }
            }
        }
    }
    const size_t G = (size_t)d->G, FG = (size_t)d->FG;
    /* the fp32 LLR array [G][N][FG] is allocated on first use (ensure_llr): flooding decoders fed through qldpc_load_bits_* never read one */
    if (cfg->schedule == QLDPC_SCHED_FLOODING) {
        const size_t elems = d->msg_i8 ? (G * d->E * FG + 3) / 4 : (d->msg_half ? (G * d->E * FG + 1) / 2 : G * d->E * FG);      /* floats of storage */
        if (d->msg_i8 && (rc = dm_alloc(&d->mem, &d->d_llr8, G * d->N * 64))) return rc;
        const char *coded_env = getenv("QLDPC_CODED_LLR");      /* =0: keep the fp32 LLR array on the load_bits path too (A/B measurements) */
        /* measured: the 8-bit VN pass gets slower with coded LLRs (5.54 vs 6.0 TB/s: four ballot words and selects per VN to save one
         * of nine bytes), so it keeps its quantised LLR array unless QLDPC_CODED_LLR=1 asks otherwise */
        if (!(coded_env && coded_env[0] == '0') && (!d->msg_i8 || (coded_env && coded_env[0] == '1'))) {
            if ((rc = dm_alloc(&d->mem, &d->d_ybits, G * d->N * V))) return rc;
            if ((rc = dm_alloc(&d->mem, &d->d_fmag, G * FG))) return rc;
            if ((rc = dm_alloc(&d->mem, &d->d_fnch, G * FG))) return rc;
            if ((rc = dm_alloc(&d->mem, &d->d_vcls, ((size_t)d->N + 3) / 4 * 4))) return rc;      /* read as dwords by the kernels */
        }
        if ((rc = dm_alloc(&d->mem, &d->d_a, elems))) return rc;
        if ((rc = dm_alloc(&d->mem, &d->d_b, elems))) return rc;
        /* The posterior form of a fixed-iteration min-sum run (qldpc_kernels_fpost.h): 0.83 x the rows of an iteration, the same floats.  fp32 messages,
         * 64-frame groups, MS / OMS / NMS, no syndrome test (early exit needs the ballots of every VN after every iteration and stays on the kernels
         * above), every check in a register-resident bucket with degree <= 27, and the IRA chain verified edge by edge.  QLDPC_FLOOD_POST=0 keeps the
         * explicit messages (A/B measurements, tests).  var_to_chk is not used by this form: posteriors and state live in its allocation where they fit. */
        {
            bool ok = !d->msg_i8 && !d->msg_half && d->V == 1 && family_of(cfg->rule) == QK_FAM_MS && !cfg->enable_syndrome && code->max_dc <= QK_FP_DCMAX;
            for (auto &b : d->cn_buckets) ok = ok && b.cap > 0;
            if (const char *e = getenv("QLDPC_FLOOD_POST")) ok = ok && atoi(e) != 0;
            std::vector<uint32_t> tab;
            if (ok) { tab.resize((size_t)d->M); ok = qldpc_code_chain_table(code, tab.data()) == 1; }
            if (ok) {
                d->ira_K = code->ira_K;
                /* QLDPC_FLOOD_POST_VN=0 keeps the in-between posterior passes on qk_vn_flood, a launch per bucket (A/B measurements, tests) */
                d->fp_vn = 1;
                env_flag("QLDPC_FLOOD_POST_VN", &d->fp_vn);
                if ((rc = make_buckets(d, code->vn_ptr, nullptr, d->ira_K, VN_CAPS, 2, d->fp_vn_buckets))) return rc;
                if (d->fp_vn) {
                    std::vector<int> vt((size_t)d->E);
                    for (int k = 0; k < d->E; k++) vt[(size_t)code->transpose[k]] = k;
                    if ((rc = make_fp_vn_classes(d, code->vn_ptr, d->ira_K, vt.data(), d->fp_vn_classes))) return rc;
                }
                if ((rc = dm_alloc(&d->mem, &d->d_fp_chain, (size_t)d->M))) return rc;
                HIPCHK(hipMemcpy(d->d_fp_chain, tab.data(), sizeof(uint32_t) * (size_t)d->M, hipMemcpyHostToDevice));
                const size_t post_n = G * d->N * 64, st_n = G * d->M * (64 * QK_FP_ROWS);
                float *base = d->d_a;
                if (post_n + 2 * st_n > elems) { if ((rc = dm_alloc(&d->mem, &d->d_fp_mem, post_n + 2 * st_n))) return rc; base = d->d_fp_mem; }
                d->fp_post = base; d->fp_st[0] = base + post_n; d->fp_st[1] = base + post_n + st_n;
                d->fpost = 1;
            }
        }
    } else if (d->msg_i8) {
        if ((rc = dm_alloc(&d->mem, &d->d_llr8, G * d->N * 64))) return rc;
        if ((rc = dm_alloc(&d->mem, &d->d_a, G * d->N * 64))) return rc;      /* post8 */
        if ((rc = dm_alloc(&d->mem, &d->d_b, G * d->E * 64))) return rc;      /* msg8, CN-major */
    } else {
        if ((rc = dm_alloc(&d->mem, &d->d_a, G * d->N * FG))) return rc;
        if ((rc = dm_alloc(&d->mem, &d->d_b, G * d->E * FG))) return rc;
    }
    if ((rc = dm_alloc(&d->mem, &d->d_sgn, G * d->N * V))) return rc;
    if (d->msg_i8) d->d_hard = d->d_sgn;      /* integer posteriors: signbit(post) and !(post >= 0) are the same ballot */
    else if ((rc = dm_alloc(&d->mem, &d->d_hard, G * d->N * V))) return rc;
    if ((rc = dm_alloc(&d->mem, &d->d_unsat, G * V))) return rc;
    if ((rc = dm_alloc(&d->mem, &d->d_done, G * V))) return rc;
    if ((rc = dm_alloc(&d->mem, &d->d_depth, G * FG))) return rc;
    if ((rc = dm_alloc(&d->mem, &d->d_iters, G * FG))) return rc;
    d->gu.patience = cfg->giveup_patience;
    if (d->gu.patience > 0 && ((rc = dm_alloc(&d->mem, &d->gu.weight, G * FG)) || (rc = dm_alloc(&d->mem, &d->gu.last, G * FG)) || (rc = dm_alloc(&d->mem, &d->gu.best, G * FG)) ||
                               (rc = dm_alloc(&d->mem, &d->gu.since, G * FG)) || (rc = dm_alloc(&d->mem, &d->gu.gave, G * V)) || (rc = dm_alloc(&d->mem, &d->gu.total, 1)))) return rc;
    if (d->gu.total) HIPCHK(hipMemset(d->gu.total, 0, sizeof(*d->gu.total)));
    if ((rc = dm_alloc(&d->mem, &d->d_active, 4))) return rc;
    HIPCHK(hipMemset(d->d_active, 0, 4 * sizeof(int)));
    if ((rc = dm_alloc(&d->mem, &d->d_work, 1))) return rc;
    /* coherent (fine-grained): the host spins on a word the kernel releases at system scope while the stream is still running */
    if (dm_alloc_pinned(&d->mem, &d->h_active, 4, hipHostMallocMapped | hipHostMallocCoherent)) { qldpc_set_error("decoder_create: pinned allocation of the mapped status words failed"); return QLDPC_EHIP; }
    memset(d->h_active, 0, 4 * sizeof(int));
    HIPCHK(hipHostGetDevicePointer((void **)&d->h_active_dev, d->h_active, 0));
    /* active-frame compaction (early exit, messages not frozen): 0 auto (flooding: batches of >= 4 groups; layered: never), 1 always, 2 never.
     * The horizontal-layered schedule compacts only when told to (1), with fp32 messages and a launch per layer; the vertical-layered one never does. */
    d->G0 = d->G;
    d->compact_mode = cfg->compact;
    env_int("QLDPC_COMPACT", &d->compact_mode);
    d->compact_ratio = 0.6f;
    if (const char *e = getenv("QLDPC_COMPACT_RATIO")) { const float x = (float)atof(e); if (x > 0.0f && x <= 1.0f) d->compact_ratio = x; }
    const bool layered_compact = cfg->schedule == QLDPC_SCHED_HLAYERED && d->compact_mode == 1 && !d->msg_i8 && !chain_asked && !d->chain;
    if (!cfg->enable_syndrome || (cfg->schedule != QLDPC_SCHED_FLOODING && !layered_compact) || d->freeze || (d->compact_mode == 0 && d->G < 4)) d->compact_mode = 2;
    if (d->compact_mode != 2) {
        if ((rc = dm_alloc(&d->mem, &d->d_gcount, (size_t)d->G))) return rc;
        if ((rc = dm_alloc(&d->mem, &d->d_goff, (size_t)d->G + 1))) return rc;
        if (d->poll_every != 1 && !getenv("QLDPC_POLL_EVERY")) d->poll_every = 1;      /* a compaction is decided on the count the status pass leaves */
    }
    return QLDPC_OK;
}

extern "C" int qldpc_decoder_create(const qldpc_code *code, int K, const int *info_bits_pos, const qldpc_decoder_cfg *cfg, qldpc_decoder **out)
{
    if (!out) return QLDPC_EINVAL;
    *out = nullptr;
    if (!code || !cfg) { qldpc_set_error("decoder_create: null code/cfg"); return QLDPC_EINVAL; }
    /* AFF3CT's ctor throws on these (Decoder_LDPC_BP: 'N' vs H.get_n_rows(), K <= N, n_ite > 0) */
    if (K <= 0 || K > code->N) { qldpc_set_error("decoder_create: K=%d not in (0, N=%d]", K, code->N); return QLDPC_ESIZE; }
    if (cfg->n_ite <= 0) { qldpc_set_error("decoder_create: n_ite=%d", cfg->n_ite); return QLDPC_EINVAL; }
    if (cfg->max_frames <= 0) { qldpc_set_error("decoder_create: max_frames=%d", cfg->max_frames); return QLDPC_EINVAL; }
    if (cfg->rule < QLDPC_RULE_MS || cfg->rule > QLDPC_RULE_AMS_MINSTAR) { qldpc_set_error("decoder_create: rule=%d", cfg->rule); return QLDPC_EINVAL; }
    if (cfg->schedule != QLDPC_SCHED_FLOODING && cfg->schedule != QLDPC_SCHED_HLAYERED && cfg->schedule != QLDPC_SCHED_VLAYERED) { qldpc_set_error("decoder_create: schedule=%d", cfg->schedule); return QLDPC_EINVAL; }
    if (cfg->enable_syndrome && cfg->syndrome_depth < 1) { qldpc_set_error("decoder_create: syndrome_depth=%d", cfg->syndrome_depth); return QLDPC_EINVAL; }
    if (cfg->frames_per_lane != 0 && cfg->frames_per_lane != 1 && cfg->frames_per_lane != 2 && cfg->frames_per_lane != 4) { qldpc_set_error("decoder_create: frames_per_lane=%d", cfg->frames_per_lane); return QLDPC_EINVAL; }
    if (cfg->msg_dtype < 0 || cfg->msg_dtype > 2) { qldpc_set_error("decoder_create: msg_dtype=%d", cfg->msg_dtype); return QLDPC_EINVAL; }
    if (cfg->compact < 0 || cfg->compact > 2 || cfg->layer_chain < 0 || cfg->layer_chain > 2) { qldpc_set_error("decoder_create: compact=%d, layer_chain=%d (0 auto, 1 on, 2 off)", cfg->compact, cfg->layer_chain); return QLDPC_EINVAL; }
    if (cfg->giveup_patience < 0) { qldpc_set_error("decoder_create: giveup_patience=%d (0 = off, >= 1 = tests without a new minimum of the syndrome weight)", cfg->giveup_patience); return QLDPC_EINVAL; }
    if (cfg->giveup_patience > 0 && !cfg->enable_syndrome) { qldpc_set_error("decoder_create: giveup_patience=%d works on the syndrome tests of the early exit: set enable_syndrome = 1", cfg->giveup_patience); return QLDPC_EINVAL; }
    if (cfg->giveup_patience > 0 && cfg->schedule == QLDPC_SCHED_VLAYERED) {
        qldpc_set_error("giveup_patience is not built for the vertical-layered schedule: use QLDPC_SCHED_FLOODING or QLDPC_SCHED_HLAYERED, or giveup_patience = 0");
        return QLDPC_EUNSUPPORTED;
    }
    if (!(cfg->quant_scale >= 0.0f) || cfg->quant_scale > 64.0f) { qldpc_set_error("decoder_create: quant_scale=%g", (double)cfg->quant_scale); return QLDPC_EINVAL; }
    if (cfg->schedule == QLDPC_SCHED_VLAYERED && (cfg->engine == QLDPC_ENGINE_EDGES || cfg->msg_dtype != 0 || cfg->layer_chain == 1 || cfg->compact == 1)) {
        qldpc_set_error("the vertical-layered schedule runs on the FRAMES engine with fp32 messages, one launch per class and no compaction "
                        "(have engine=%d, msg_dtype=%d, layer_chain=%d, compact=%d)", cfg->engine, cfg->msg_dtype, cfg->layer_chain, cfg->compact);
        return QLDPC_EUNSUPPORTED;
    }
    /* the SPA fold of the FRAMES engine keeps prod (1 + e^-|x_j|) <= 2^dc in fp32 (qldpc_kernels.h): from degree 128 on it overflows and every edge of the check
     * gets the clamp.  The edge engine stops at degree 64, so such a code always comes here. */
    if (cfg->rule == QLDPC_RULE_SPA && code->max_dc >= 128) {
        qldpc_set_error("SPA is built for check degrees below 128 (have %d): its product of dc factors overflows fp32 beyond that; use QLDPC_RULE_LSPA, which has no product", code->max_dc);
        return QLDPC_EUNSUPPORTED;
    }
    qldpc_decoder *d = new (std::nothrow) qldpc_decoder();
    if (!d) return QLDPC_ENOMEM;
    int rc = create_impl(code, K, info_bits_pos, cfg, d);
    if (rc == QLDPC_ENOMEM) qldpc_set_error("decoder_create: out of device memory with %zu bytes allocated", d->mem.dev_bytes);
    if (rc != QLDPC_OK) { qldpc_decoder_free(d); return rc; }
    *out = d;
    return QLDPC_OK;
}

/* ---- generations of the per-frame state (active-frame compaction) ---------------------------- */

static void use_gen(qldpc_decoder *d, int k)
{
    const gen_state &n = d->gens[(size_t)k];
    d->G = n.G;
    d->d_sgn = n.sgn; d->d_hard = n.hard; d->d_unsat = n.unsat; d->d_done = n.done; d->d_ybits = n.ybits; d->d_synd = n.synd; d->d_ebits = n.ebits;
    d->d_depth = n.depth; d->d_iters = n.iters; d->d_fmag = n.fmag; d->d_fnch = n.fnch; d->d_llr = n.llr; d->d_llr8 = n.llr8;
    d->gu.last = n.gu_last; d->gu.best = n.gu_best; d->gu.since = n.gu_since; d->gu.gave = n.gu_gave;
    if (n.post) { d->d_a = n.post; d->d_b = n.msg; }      /* layered: each generation has its own posteriors and messages */
}
/* back to the batch as loaded (generation 0 = the decoder's base arrays) */
static void view_reset(qldpc_decoder *d)
{
    if (d->cur_gen != 0) { use_gen(d, 0); d->cur_gen = 0; }
    d->remap_src = nullptr; d->remap_msg = nullptr;
}
static void gen0_capture(qldpc_decoder *d)
{
    if (d->gens.empty()) d->gens.resize(1);
    gen_state &n = d->gens[0];
    n.G = n.cap = d->G0;
    n.sgn = d->d_sgn; n.hard = d->d_hard; n.unsat = d->d_unsat; n.done = d->d_done; n.ybits = d->d_ybits; n.synd = d->d_synd; n.ebits = d->d_ebits;
    n.depth = d->d_depth; n.iters = d->d_iters; n.origin = nullptr; n.src = nullptr; n.fmag = d->d_fmag; n.fnch = d->d_fnch; n.llr = d->d_llr; n.llr8 = d->d_llr8;
    n.gu_last = d->gu.last; n.gu_best = d->gu.best; n.gu_since = d->gu.since; n.gu_gave = d->gu.gave;
    n.post = d->d_a; n.msg = d->d_b;
}

static int ensure_llr(qldpc_decoder *d)
{
    if (d->d_llr) return QLDPC_OK;
    return dm_alloc(&d->mem, &d->d_llr, (size_t)d->G * d->N * d->FG);
}
/* the frame-interleaved posteriors [G][N][FG] fetch_post and fetch_weakest read, on first use */
static int ensure_post(qldpc_decoder *d)
{
    if (d->d_post) return QLDPC_OK;
    return dm_alloc(&d->mem, &d->d_post, (size_t)d->G * d->N * d->FG);
}

extern "C" int qldpc_decoder_set_stream(qldpc_decoder *d, void *s)
{
    if (!d) return QLDPC_EINVAL;
    HIPCHK(hipSetDevice(d->device));
    return qldpc_stream_switch(&d->stream, s);
}
extern "C" size_t qldpc_decoder_device_bytes(const qldpc_decoder *d) { return d ? d->mem.dev_bytes : 0; }
extern "C" int qldpc_decoder_flood_post(const qldpc_decoder *d) { return d ? d->fpost : (int)QLDPC_EINVAL; }
extern "C" int qldpc_last_run_iterations(const qldpc_decoder *d) { return d ? d->last_iters : (int)QLDPC_EINVAL; }

/* early-exit bookkeeping of the last run (FRAMES engine): out[0] = lane-iterations executed (groups that ran an iteration x frames
 * per group, counted by the status pass), out[1] = compactions, out[2] = groups in the last generation, out[3] = frames per group.
 * Synchronises the stream. */
extern "C" int qldpc_last_run_stats(qldpc_decoder *d, long long out[4])
{
    if (!d || !out) return QLDPC_EINVAL;
    out[0] = out[1] = out[2] = out[3] = 0;
    if (d->engine == QLDPC_ENGINE_EDGES || !d->d_work) return QLDPC_OK;
    HIPCHK(hipSetDevice(d->device));
    unsigned long long w = 0;
    HIPCHK(hipMemcpyAsync(&w, d->d_work, sizeof(w), hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    out[0] = (long long)w * d->FG; out[1] = d->compactions; out[2] = d->G; out[3] = d->FG;
    return QLDPC_OK;
}

/* reset(): the next decode starts from chk_to_var = 0 (BS/src/main.cpp:389).  Every qldpc_run starts
 * from that state anyway (frames are independent decodes), so this only drops loaded frames. */
extern "C" int qldpc_decoder_reset(qldpc_decoder *d)
{
    if (!d) return QLDPC_EINVAL;
    view_reset(d);
    d->loaded = 0; d->ran = 0; d->n_frames = 0;
    return QLDPC_OK;
}

extern "C" int qldpc_sync(qldpc_decoder *d)
{
    if (!d) return QLDPC_EINVAL;
    HIPCHK(hipSetDevice(d->device));
    HIPCHK(hipStreamSynchronize(d->stream));
    return QLDPC_OK;
}

/* ------------------------------------------------------------------ profiling ---------------- */

extern "C" int qldpc_profile_enable(qldpc_decoder *d, int on) { if (!d) return QLDPC_EINVAL; d->prof_on = on; return QLDPC_OK; }

static int prof_fold(qldpc_decoder *d)
{
    if (d->prof_pending.empty()) return QLDPC_OK;
    HIPCHK(hipStreamSynchronize(d->stream));
    for (auto &r : d->prof_pending) {
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) {
            d->stats[r.kind].launches++;
            d->stats[r.kind].total_ms += ms;
            d->stats[r.kind].alg_bytes += r.bytes;
            d->stats[r.kind].moved_bytes += r.moved;
        }
        (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b);
    }
    d->prof_pending.clear();
    return QLDPC_OK;
}

extern "C" int qldpc_profile_read(qldpc_decoder *d, qldpc_kernel_stat *out, int cap)
{
    if (!d || (!out && cap > 0)) return QLDPC_EINVAL;
    HIPCHK(hipSetDevice(d->device));
    int rc = prof_fold(d);
    if (rc) return rc;
    int n = 0;
    for (int k = 0; k < KS_COUNT && n < cap; k++) if (d->stats[k].launches) out[n++] = d->stats[k];
    return n;
}

extern "C" int qldpc_profile_clear(qldpc_decoder *d)
{
    if (!d) return QLDPC_EINVAL;
    int rc = prof_fold(d);
    if (rc) return rc;
    for (int k = 0; k < KS_COUNT; k++) { d->stats[k].launches = 0; d->stats[k].total_ms = 0; d->stats[k].alg_bytes = 0; d->stats[k].moved_bytes = 0; }
    return QLDPC_OK;
}

/* ------------------------------------------------------------------ launch helpers ----------- */

/* algorithmic bytes beyond bytes_cn / bytes_vn of qldpc_engine_int.h, and what the passes move.
 * What a variable-node pass has to fetch in the data form in use: with coded LLRs the channel values are N/8 bytes of received-bit
 * ballots per frame (plus a class byte per VN, shared by all frames) instead of an N * llr_b array */
static double moved_vn(const qldpc_decoder *d, int mode)
{
    if (!d->llr_coded) return bytes_vn(d, mode);
    const double msgs = (mode == QK_VN_NORMAL ? 2.0 : 1.0) * d->E * msg_b(d);
    return (msgs + d->N / 8.0) * live_frames(d) + d->N;
}
static double bytes_layer(const qldpc_decoder *d) { return 4.0 * d->E * msg_b(d) * live_frames(d); }
/* what a sweep moves: with the compressed check state 2 E posterior rows + 8 M state rows per 64-frame group */
static double moved_layer(const qldpc_decoder *d)
{
    if (!d->layer_cst) return bytes_layer(d);
    return (2.0 * d->E * 4.0 + 8.0 * d->M * 4.0) * live_frames(d);
}

/* fn(std::integral_constant<int, V>{}) for the decoder's frames-per-lane value: the one place that turns d->V into a template argument */
template <typename F>
static auto with_v(const qldpc_decoder *d, F fn)
{
    switch (d->V) {
    case 1: return fn(std::integral_constant<int, 1>{});
    case 2: return fn(std::integral_constant<int, 2>{});
    default: return fn(std::integral_constant<int, 4>{});
    }
}

/* grids {x, groups}: x = the workgroups that cover n_items at per_block each, capped so that the whole launch stays at 4 096 (load and fetch: a wave
 * per packed word) or 8 192 (the row kernels of a run: per_block rows a workgroup) workgroups */
static inline dim3 grid_4k(const qldpc_decoder *d, int n_words) { return dim3((unsigned)std::max(1, std::min((n_words + QK_WAVES - 1) / QK_WAVES, 4096 / std::max(1, d->G))), (unsigned)d->G); }
static inline dim3 grid_8k(int n_items, int per_block, int G) { return dim3((unsigned)std::max(1, std::min((n_items + per_block - 1) / per_block, 8192 / std::max(1, G))), (unsigned)G); }

template <int V, int MODE>
static int vn_pass(qldpc_decoder *d, float *post_out)
{
    prof_scope ps(d, KS_VN, bytes_vn(d, MODE), moved_vn(d, MODE));
    for (auto &b : d->vn_buckets) { qldpc_launch_vn<V, MODE>(d, b, post_out); LAUNCHCHK(); }
    return QLDPC_OK;
}
template <int V>
static int cn_pass(qldpc_decoder *d, bool first = false)
{
    /* the first pass with coded LLRs reads ballots instead of var_to_chk rows */
    prof_scope ps(d, KS_CN, bytes_cn(d), first && !d->msg_i8 ? ((double)d->E * msg_b(d) + d->N / 8.0) * live_frames(d) : -1.0);
    for (auto &b : d->cn_buckets) { qldpc_launch_cn<V>(d, b, first); LAUNCHCHK(); }
    d->remap_src = nullptr;      /* chk_to_var is in the current generation's layout now, and so is everything after it */
    return QLDPC_OK;
}
/* ---- the posterior form of the flooding run (qldpc_kernels_fpost.h) ----
 * Algorithmic bytes stay what DESIGN section 4 prices: 2 E rows for a check pass, E + N for a _compute_post.  Moved is what the kernels move: a check pass
 * gathers one posterior row and writes one message row per information edge and reads and writes its own three state rows (the neighbours' rows, cache
 * hits for three waves in four, are not counted); the first one reads channel values instead of posteriors and no state.  A posterior pass reads the
 * information edges' message rows and writes one row per information VN (in between) or only ballots (closing the run). */
static double fp_info_edges(const qldpc_decoder *d) { return (double)d->E - (2.0 * d->M - 1.0); }
static double fp_chan(const qldpc_decoder *d, double vns) { return d->llr_coded ? vns / 8.0 : vns * 4.0; }
static double moved_cn_fpost(const qldpc_decoder *d, bool first)
{
    const double Ei = fp_info_edges(d), st = (double)QK_FP_ROWS * d->M * 4.0;
    if (first) return (Ei * 4.0 + st + fp_chan(d, d->N)) * live_frames(d);
    return (2.0 * Ei * 4.0 + 2.0 * st + fp_chan(d, d->M)) * live_frames(d);
}
static double moved_vn_fpost(const qldpc_decoder *d, bool rows_out, bool ballots)
{
    return (fp_info_edges(d) * 4.0 + fp_chan(d, d->ira_K) + (rows_out ? d->ira_K * 4.0 : 0.0) + (ballots ? d->ira_K / 4.0 : 0.0)) * live_frames(d);
}
/* the records of qk_vn_fpost: every 64-frame group reads them once per pass */
static double fp_vn_rec_bytes(const qldpc_decoder *d)
{
    double b = 0.0;
    for (auto &c : d->fp_vn_classes) b += (double)c.n * QK_FPV_STRIDE(c.deg) * 4.0;
    return b * (live_frames(d) / 64.0);
}
static int cn_pass_fpost(qldpc_decoder *d, int ite)
{
    prof_scope ps(d, KS_CN, bytes_cn(d), moved_cn_fpost(d, ite == 0));
    for (auto &b : d->cn_buckets) { qldpc_launch_cn_fpost(d, b, ite); LAUNCHCHK(); }
    d->fp_last = ite & 1;
    return QLDPC_OK;
}
/* _compute_post over the information VNs: in between iterations it leaves the posterior rows the next check pass gathers and no ballots */
static int vn_pass_fpost(qldpc_decoder *d, float *post_out, bool between)
{
    const bool own = between && d->fp_vn;      /* qk_vn_fpost: every register-resident bucket in one launch, on the records */
    prof_scope ps(d, KS_VN, bytes_vn(d, QK_VN_POST), moved_vn_fpost(d, post_out != nullptr, !between) + (own ? fp_vn_rec_bytes(d) : 0.0));
    d->fp_between = between ? 1 : 0;
    if (own) { qldpc_launch_vn_fpost(d); LAUNCHCHK(); }
    for (auto &b : d->fp_vn_buckets)
        if (!own || b.cap == 0) { qldpc_launch_vn<1, QK_VN_POST>(d, b, post_out); LAUNCHCHK(); }
    d->fp_between = 0;
    return QLDPC_OK;
}
/* ... and over the chain VNs, from the final check state (own rows counted, as in the check pass) */
static int close_fpost(qldpc_decoder *d, float *post_out)
{
    const double b = ((double)QK_FP_ROWS * d->M * 4.0 + fp_chan(d, d->M) + (post_out ? d->M * 4.0 : 0.0) + d->M / 4.0) * live_frames(d);
    prof_scope ps(d, KS_VN, b, b);
    qldpc_launch_fpost_close(d, post_out);
    LAUNCHCHK();
    return QLDPC_OK;
}
static int run_flooding_post(qldpc_decoder *d)
{
    int rc;
    const int n_ite = d->cfg.n_ite;
    for (int ite = 0; ite < n_ite; ite++) {
        if ((rc = cn_pass_fpost(d, ite))) return rc;      /* iteration 0 rebuilds (Y + 0) - 0 itself: no _initialize_var_to_chk in front of it */
        if (ite < n_ite - 1 && (rc = vn_pass_fpost(d, d->fp_post, true))) return rc;
    }
    d->last_iters = n_ite;
    if ((rc = vn_pass_fpost(d, nullptr, false))) return rc;
    return close_fpost(d, nullptr);
}

template <int V>
static int synd_pass(qldpc_decoder *d, const u64 *mask, int skip_done)
{
    prof_scope ps(d, KS_SYND, (double)d->E * 8.0 * d->G * V);
    const int g8 = (d->G + 7) / 8 * 8;      /* groups rounded up to the XCD count: see qk_syndrome */
    /* early-exit passes go in two launches: an eighth of the checks first; the second launch returns at once for every group in which
     * all running frames already show an unsatisfied check (measured: 1.17 -> 0.69 ms of syndrome passes per config-2 step).  The closing success-flag pass
     * (skip_done = 0) and small codes take one launch. */
    const int Mp = (skip_done && d->M >= 4096) ? ((d->M / 8 + 255) / 256) * 256 : d->M;
    for (int part = 0; part < (Mp < d->M ? 2 : 1); part++) {
        const int lo = part ? Mp : 0, hi = part ? d->M : Mp;
        const int bx = std::max(1, std::min((hi - lo + 255) / 256, 4096 / std::max(1, d->G)));
        hipLaunchKernelGGL((qk_syndrome<V>), dim3((unsigned)((d->G < 8 ? d->G : g8) * bx)), dim3(256), 0, d->stream, mask, d->d_cn_var_t, d->max_dc, d->M, d->N,
                           d->d_unsat, d->d_done, skip_done, target_synd(d), d->G, bx, lo, hi, part);
    }
    LAUNCHCHK();
    return QLDPC_OK;
}
template <int V>
static int status_pass(qldpc_decoder *d, int ite_done)
{
    prof_scope ps(d, KS_STATUS, 0.0);
    hipLaunchKernelGGL((qk_status<V>), dim3((unsigned)d->G), dim3(64), 0, d->stream, d->d_unsat, d->d_done, d->d_depth, d->d_iters, d->G,
                       d->cfg.syndrome_depth, ite_done, d->d_active, d->d_work, (volatile int *)d->h_active_dev, ++d->poll_seq);
    LAUNCHCHK();
    return QLDPC_OK;
}
/* the same two passes with giveup_patience > 0 (qldpc_kernels_giveup.h): every check counted in one launch, and the status pass that runs the rule */
template <int V>
static int synd_count_pass(qldpc_decoder *d)
{
    prof_scope ps(d, KS_SYND, (double)d->E * 8.0 * d->G * V);
    const int g8 = (d->G + 7) / 8 * 8;
    const int bx = std::max(1, std::min((d->M + 255) / 256, 4096 / std::max(1, d->G)));
    hipLaunchKernelGGL((qk_syndrome_count<V>), dim3((unsigned)((d->G < 8 ? d->G : g8) * bx)), dim3(256), 0, d->stream, d->d_sgn, d->d_cn_var_t, d->max_dc, d->M, d->N,
                       d->d_unsat, d->d_done, target_synd(d), d->G, bx, d->gu.weight);
    LAUNCHCHK();
    return QLDPC_OK;
}
template <int V>
static int status_count_pass(qldpc_decoder *d, int ite_done)
{
    prof_scope ps(d, KS_STATUS, 0.0);
    hipLaunchKernelGGL((qk_status_count<V>), dim3((unsigned)d->G), dim3(64), 0, d->stream, d->d_unsat, d->d_done, d->d_depth, d->d_iters, d->G,
                       d->cfg.syndrome_depth, ite_done, d->d_active, d->d_work, (volatile int *)d->h_active_dev, ++d->poll_seq, d->gu);
    LAUNCHCHK();
    return QLDPC_OK;
}
/* blocking: how many groups still have unconverged frames after the status pass launched last, and how many frames those are.
 * The kernel writes the counts and then its sequence number into mapped pinned memory; the host spins on the sequence word. */
static int poll_active(qldpc_decoder *d, int *active, int *active_frames)
{
    int *h = d->h_active;
    const auto t0 = std::chrono::steady_clock::now();
    unsigned spins = 0;
    while (__atomic_load_n(&h[2], __ATOMIC_ACQUIRE) != d->poll_seq) {
        if ((++spins & 0xfffu) == 0) {
            hipError_t e = hipStreamQuery(d->stream);      /* a failed launch / device fault must not leave the host spinning */
            if (e != hipSuccess && e != hipErrorNotReady) { qldpc_set_error("early-exit poll: %s", hipGetErrorString(e)); return QLDPC_EHIP; }
            if (e == hipSuccess && __atomic_load_n(&h[2], __ATOMIC_ACQUIRE) != d->poll_seq) {
                /* the stream has drained: the report is on its way through the host's memory system, or was never written */
                if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(5)) { qldpc_set_error("early-exit poll: status report never arrived"); return QLDPC_EHIP; }
            }
            if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(120)) { qldpc_set_error("early-exit poll: timed out"); return QLDPC_EHIP; }
        }
    }
    *active = h[0];
    *active_frames = h[1];
    return QLDPC_OK;
}

/*
 * Open the next generation: the `active_frames` frames that have not converged move into ceil(active_frames / FG) full groups
 * (qldpc_kernels_compact.h).  The message arrays are not touched: the next check pass reads through d->remap_src.
 * Layered schedule: the posteriors are gathered into a side buffer, the next sweep reads the messages of the old generation through d->remap_src and
 * writes them into a side buffer too (the layer kernels update in place: a generation cannot take the place of the one it is read from).
 */
template <typename T> static int gen_alloc(qldpc_decoder *d, T **p, size_t n) { return *p ? QLDPC_OK : dm_alloc(&d->mem, p, n); }

template <int V>
static int compact(qldpc_decoder *d, int active_frames)
{
    int rc;
    const int FG = d->FG, k = d->cur_gen + 1;
    const int Gn = (active_frames + FG - 1) / FG;
    if ((int)d->gens.size() <= k) d->gens.resize((size_t)k + 1);
    const gen_state o = d->gens[(size_t)k - 1];
    gen_state &n = d->gens[(size_t)k];
    if (n.cap < Gn) {      /* first use (or a larger need than any run before): sized for the largest batch this generation can get */
        (void)hipStreamSynchronize(d->stream);
        /* everything a generation past 0 owns (llr / llr8 / post / msg are views into the decoder's side buffers) */
        dm_release(&d->mem, &n.sgn); dm_release(&d->mem, &n.hard); dm_release(&d->mem, &n.unsat); dm_release(&d->mem, &n.done); dm_release(&d->mem, &n.ybits); dm_release(&d->mem, &n.synd); dm_release(&d->mem, &n.ebits);
        dm_release(&d->mem, &n.depth); dm_release(&d->mem, &n.iters); dm_release(&d->mem, &n.origin); dm_release(&d->mem, &n.src); dm_release(&d->mem, &n.fmag); dm_release(&d->mem, &n.fnch);
        dm_release(&d->mem, &n.gu_last); dm_release(&d->mem, &n.gu_best); dm_release(&d->mem, &n.gu_since); dm_release(&d->mem, &n.gu_gave);
        n.cap = std::max(Gn, std::min(o.cap, (int)(d->compact_ratio * (float)o.cap) + 1));
    }
    const size_t C = (size_t)n.cap;
    if ((rc = gen_alloc(d, &n.sgn, C * d->N * V))) return rc;
    if (d->msg_i8) n.hard = n.sgn;
    else if ((rc = gen_alloc(d, &n.hard, C * d->N * V))) return rc;
    if ((rc = gen_alloc(d, &n.unsat, C * V)) || (rc = gen_alloc(d, &n.done, C * V))) return rc;
    if ((rc = gen_alloc(d, &n.depth, C * FG)) || (rc = gen_alloc(d, &n.iters, C * FG)) || (rc = gen_alloc(d, &n.origin, C * FG)) || (rc = gen_alloc(d, &n.src, C * FG))) return rc;
    if (o.fmag && ((rc = gen_alloc(d, &n.fmag, C * FG)) || (rc = gen_alloc(d, &n.fnch, C * FG)))) return rc;
    if (d->gu.patience > 0 && ((rc = gen_alloc(d, &n.gu_last, C * FG)) || (rc = gen_alloc(d, &n.gu_best, C * FG)) || (rc = gen_alloc(d, &n.gu_since, C * FG)) || (rc = gen_alloc(d, &n.gu_gave, C * V)))) return rc;
    if (d->llr_coded && (rc = gen_alloc(d, &n.ybits, C * d->N * V))) return rc;
    if (d->has_synd && (rc = gen_alloc(d, &n.synd, C * d->M * V))) return rc;
    if (d->llr_coded && d->has_erase && (rc = gen_alloc(d, &n.ebits, C * d->N * V))) return rc;
    n.G = Gn;
    n.llr = nullptr; n.llr8 = nullptr; n.post = nullptr; n.msg = nullptr;
    const bool layered = d->cfg.schedule == QLDPC_SCHED_HLAYERED;      /* reads no channel LLRs after var_nodes = Y_N: they stay where they are */
    const bool rows8 = !layered && !d->llr_coded && d->msg_i8, rows32 = !layered && !d->llr_coded && !d->msg_i8;
    if (layered) {
        const int side = k & 1;
        if (d->lay_alt_cap[side] < n.cap) {      /* sized by the first generation that uses it; grows if a later batch needs more */
            (void)hipStreamSynchronize(d->stream);
            dm_release(&d->mem, &d->d_post_alt[side]); dm_release(&d->mem, &d->d_msg_alt[side]);
            d->lay_alt_cap[side] = 0;
            if ((rc = dm_alloc(&d->mem, &d->d_post_alt[side], C * d->N * FG)) || (rc = dm_alloc(&d->mem, &d->d_msg_alt[side], C * d->E * FG))) { dm_release(&d->mem, &d->d_post_alt[side]); return rc; }
            d->lay_alt_cap[side] = n.cap;
        }
        n.post = d->d_post_alt[side]; n.msg = d->d_msg_alt[side];
    }
    if (rows8 || rows32) {      /* the decoder reads an LLR array: its rows move too, ping-pong between two side buffers (the loaded batch stays intact) */
        const int side = k & 1;
        if (d->llr_alt_cap[side] < n.cap) {      /* sized by the first generation that uses it (later ones are smaller); grows if a later batch needs more */
            (void)hipStreamSynchronize(d->stream);
            dm_release(&d->mem, &d->d_llr_alt[side]); dm_release(&d->mem, &d->d_llr8_alt[side]);
            d->llr_alt_cap[side] = n.cap;
        }
        const size_t need = (size_t)d->llr_alt_cap[side] * d->N * (rows8 ? 64 : (size_t)FG);
        if (rows8 && !d->d_llr8_alt[side] && (rc = dm_alloc(&d->mem, &d->d_llr8_alt[side], need))) return rc;
        if (rows32 && !d->d_llr_alt[side] && (rc = dm_alloc(&d->mem, &d->d_llr_alt[side], need))) return rc;
        n.llr8 = rows8 ? d->d_llr8_alt[side] : nullptr; n.llr = rows32 ? d->d_llr_alt[side] : nullptr;
    }
    prof_scope ps(d, KS_STATUS, 0.0);
    hipLaunchKernelGGL((qk_compact_count<V>), dim3((unsigned)((o.G + 255) / 256)), dim3(256), 0, d->stream, o.done, d->d_gcount, o.G);
    hipLaunchKernelGGL(qk_compact_scan, dim3(1), dim3(256), 0, d->stream, d->d_gcount, d->d_goff, o.G);
    hipLaunchKernelGGL((qk_compact_scatter<V>), dim3((unsigned)o.G), dim3(64), 0, d->stream, o.done, d->d_goff, n.src);
    hipLaunchKernelGGL((qk_compact_fill<V>), dim3((unsigned)Gn), dim3(64), 0, d->stream, n.src, d->d_goff + o.G, o.origin, n.origin, o.fmag, n.fmag, o.fnch, n.fnch,
                       o.depth, n.depth, n.iters, n.done, n.unsat, d->cfg.n_ite, d->N, qk_giveup{nullptr, o.gu_last, o.gu_best, o.gu_since, o.gu_gave, nullptr, 0},
                       qk_giveup{nullptr, n.gu_last, n.gu_best, n.gu_since, n.gu_gave, nullptr, 0});
    LAUNCHCHK();
    if (d->llr_coded) hipLaunchKernelGGL((qk_compact_ballots<V>), dim3((unsigned)((d->N + 64 * QK_WAVES - 1) / (64 * QK_WAVES)), (unsigned)Gn), dim3(QK_THREADS), 0, d->stream, o.ybits, n.ybits, n.src, d->N);
    if (d->has_synd) hipLaunchKernelGGL((qk_compact_ballots<V>), dim3((unsigned)((d->M + 64 * QK_WAVES - 1) / (64 * QK_WAVES)), (unsigned)Gn), dim3(QK_THREADS), 0, d->stream, o.synd, n.synd, n.src, d->M);
    if (d->llr_coded && d->has_erase) hipLaunchKernelGGL((qk_compact_ballots<V>), dim3((unsigned)((d->N + 64 * QK_WAVES - 1) / (64 * QK_WAVES)), (unsigned)Gn), dim3(QK_THREADS), 0, d->stream, o.ebits, n.ebits, n.src, d->N);
    const dim3 rows = grid_8k(d->N, QK_WAVES, Gn);
    if (rows32) hipLaunchKernelGGL((qk_compact_rows<V, float>), rows, dim3(QK_THREADS), 0, d->stream, o.llr, n.llr, n.src, d->N, 1.0f);
    if (rows8) hipLaunchKernelGGL((qk_compact_rows<V, uint8_t>), rows, dim3(QK_THREADS), 0, d->stream, (const uint8_t *)o.llr8, (uint8_t *)n.llr8, n.src, d->N, (uint8_t)0);
    LAUNCHCHK();
    if (layered) {
        prof_scope pr(d, KS_COMPACT_ROWS, 2.0 * d->N * 4.0 * active_frames);
        hipLaunchKernelGGL((qk_compact_rows<V, float>), rows, dim3(QK_THREADS), 0, d->stream, (const float *)o.post, n.post, n.src, d->N, 1.0f);
        LAUNCHCHK();
        d->remap_msg = o.msg;
    }
    d->cur_gen = k;
    use_gen(d, k);
    d->remap_src = n.src;
    d->compactions++;
    return QLDPC_OK;
}

/* ------------------------------------------------------------------ run ---------------------- */

/* the sign ballots of the posteriors of a layered run (what the variable-node pass of a flooding run leaves behind) */
template <int V>
static int post_ballots(qldpc_decoder *d)
{
    if (d->msg_i8) hipLaunchKernelGGL(qi_post_ballots, grid_8k(d->N, QK_WAVES, d->G), dim3(QK_THREADS), 0, d->stream, (const uint32_t *)d->d_a, d->d_sgn, (u64 *)nullptr, d->N, d->d_done);
    else hipLaunchKernelGGL((qk_post_ballots<V>), grid_8k(d->N, 32 * QK_WAVES, d->G), dim3(QK_THREADS), 0, d->stream, d->d_a, d->d_sgn, d->d_hard, d->N, d->d_done);
    LAUNCHCHK();
    return QLDPC_OK;
}

/*
 * What follows an iteration / a sweep when the syndrome test is on, `ite_done` of them done: syndrome pass, status pass and -- every poll_every
 * iterations -- the host's look at what the status pass counted.  *stop: no group has a frame left to decode.  Otherwise, few enough frames left:
 * deal them into fewer, full groups (the next check pass / sweep reads through the slot map; d->G is the number of groups that hold frames).
 * track_live: the byte accounting of the profile follows the groups still running.
 */
/* its two halves, which a gang run (gang_run) issues for all members before it waits for any of them: the launches ... */
template <int V>
static int early_exit_launch(qldpc_decoder *d, int ite_done)
{
    int rc;
    if (d->gu.patience > 0) return (rc = synd_count_pass<V>(d)) ? rc : status_count_pass<V>(d, ite_done);
    if ((rc = synd_pass<V>(d, d->d_sgn, 1)) || (rc = status_pass<V>(d, ite_done))) return rc;
    return QLDPC_OK;
}
/* ... and the host's look at the count of the status pass launched last */
template <int V>
static int early_exit_poll(qldpc_decoder *d, int ite_done, bool track_live, bool *stop)
{
    int rc;
    *stop = false;
    int active = 1, left = 0;
    if ((rc = poll_active(d, &active, &left))) return rc;
    if (track_live) d->live_lanes = active * d->FG;
    *stop = active == 0;
    const int Gn = (left + d->FG - 1) / d->FG;
    if (!*stop && d->compact_mode != 2 && d->cur_gen + 1 < QLDPC_MAX_GENS && ite_done + 1 < d->cfg.n_ite && Gn < d->G &&
        (d->compact_mode == 1 || (float)Gn <= d->compact_ratio * (float)d->G))
        return compact<V>(d, left);
    return QLDPC_OK;
}
template <int V>
static int early_exit_step(qldpc_decoder *d, int ite_done, bool track_live, bool *stop)
{
    int rc;
    *stop = false;
    if ((rc = early_exit_launch<V>(d, ite_done))) return rc;
    if (d->poll_every <= 0 || (ite_done % d->poll_every) != 0) return QLDPC_OK;
    return early_exit_poll<V>(d, ite_done, track_live, stop);
}

template <int V>
static int run_flooding(qldpc_decoder *d)
{
    if constexpr (V == 1) { if (d->fpost) return run_flooding_post(d); }
    int rc;
    const int n_ite = d->cfg.n_ite;
    /* coded LLRs (fp32 / binary16 messages): the first check pass rebuilds its inputs itself, so _initialize_var_to_chk of
     * iteration 0 (E rows written, E rows read back) is not run at all */
    const bool skip_first = d->msg_i8 ? !d->llr_coded : (d->llr_coded != 0);      /* 8-bit: the first check pass reads llr8 itself */
    if (!skip_first && (rc = vn_pass<V, QK_VN_FIRST>(d, nullptr))) return rc;
    int ite = 0;
    for (; ite < n_ite; ite++) {
        if ((rc = cn_pass<V>(d, skip_first && ite == 0))) return rc;
        if (ite == n_ite - 1) { ite++; break; }      /* no test after the last iteration: the closing _compute_post and run_v's success flag follow */
        if ((rc = vn_pass<V, QK_VN_NORMAL>(d, nullptr))) return rc;
        if (d->cfg.enable_syndrome) {
            bool stop;
            if ((rc = early_exit_step<V>(d, ite + 1, true, &stop))) return rc;
            if (stop) { ite++; break; }
        }
    }
    d->last_iters = ite;
    /* final _compute_post for every frame (frozen frames recompute the posterior they stopped at) */
    d->post_closes_run = d->cfg.enable_syndrome ? 1 : 0;
    rc = vn_pass<V, QK_VN_POST>(d, nullptr);
    d->post_closes_run = 0;
    return rc;
}

/* for the length of a layered run, d->G = the groups that hold frames (run_layered says why) */
struct live_groups {
    qldpc_decoder *d; int saved;
    explicit live_groups(qldpc_decoder *d_) : d(d_), saved(d_->G) { const int gl = std::max(1, (d->n_frames + d->FG - 1) / d->FG); if (gl < d->G) d->G = gl; }
    ~live_groups() { if (d->cur_gen == 0) d->G = saved; }      /* a run that compacted leaves the last generation's view, as a flooding run does */
};

/* The parts of a layered run: run_layered strings them together for one decoder, gang_run for several decoders in lockstep.
 * All of them run with live_groups in place. */
static inline bool layered_skip_clear(const qldpc_decoder *d) { return !d->msg_i8 && !d->freeze; }

/* prologue: var_nodes = Y_N, messages = 0 where a sweep reads them before it writes them, the one-launch sweep's counters */
template <int V>
static int layered_begin(qldpc_decoder *d, bool *chain_out)
{
    const size_t G = (size_t)d->G, FG = (size_t)d->FG;
    const size_t cell = d->msg_i8 ? 1 : sizeof(float);
    HIPCHK(hipMemcpyAsync(d->d_a, d->msg_i8 ? (const void *)d->d_llr8 : (const void *)d->d_llr, G * d->N * FG * cell, hipMemcpyDeviceToDevice, d->stream));   /* var_nodes = Y_N */
    /* messages = 0: fp32 sweeps that never mask a store (freeze = 0) do not clear and re-read E rows per frame group for that -- sweep 0's
     * layer kernels take the messages as zero and write every row (config 5: 0.92 GB not written and not read per decode) */
    if (!layered_skip_clear(d)) HIPCHK(hipMemsetAsync(d->d_b, 0, G * d->E * FG * cell, d->stream));
    bool chain = false;
    if constexpr (V == 1) {
        chain = d->chain != 0;
        if (chain) {
            if (d->chain_blocks == 0) { d->chain_blocks = qldpc_chain_resident_blocks(d); if (d->chain_blocks < 64) chain = false, d->chain = 0;
                if (getenv("QLDPC_DEBUG")) fprintf(stderr, "libqldpc: one-launch layered sweep: %d resident workgroups of %d waves\n", d->chain_blocks, QK_WAVES); }
            if (chain) {
                HIPCHK(hipMemsetAsync(d->d_chain_ver, 0, sizeof(int) * G * d->N, d->stream));
                HIPCHK(hipMemsetAsync(d->d_chain_ctl, 0, sizeof(int) * QC_CTL_WORDS, d->stream));
            }
        }
    }
    *chain_out = chain;
    return QLDPC_OK;
}

/* sweep `ite`: a launch per layer and bucket, or the one launch of the chain */
template <int V>
static int layered_sweep(qldpc_decoder *d, int ite, bool chain)
{
    prof_scope ps(d, d->remap_src ? KS_LAYER_REMAP : KS_LAYER, bytes_layer(d), moved_layer(d));
    d->layer_first = (layered_skip_clear(d) && ite == 0) ? 1 : 0;
    if (chain) {
        HIPCHK(hipMemsetAsync(d->d_chain_ctl + QC_CTL_SHARD0, 0, sizeof(int) * 32 * QC_SHARDS, d->stream));      /* the ticket counters; the fault word stays */
        qldpc_launch_layer_chain(d, ite);
        LAUNCHCHK();
    }
    else
        for (int l = 0; l < d->n_layers; l++)
            for (auto &b : d->layer_buckets[(size_t)l]) { qldpc_launch_layer<V>(d, b); LAUNCHCHK(); }
    d->remap_src = nullptr; d->remap_msg = nullptr;      /* every message row is in the current generation's layout now */
    return QLDPC_OK;
}

/* after a sweep with the syndrome test on: the sign ballots of the posteriors the test reads (N rows read) */
template <int V>
static int layered_test_ballots(qldpc_decoder *d)
{
    prof_scope ps(d, KS_SYND, 0.0, (double)d->N * 4.0 * d->n_frames);
    return post_ballots<V>(d);
}

/* epilogue: `ite` sweeps were issued; the closing ballots, and the one-launch sweep's fault word */
template <int V>
static int layered_end(qldpc_decoder *d, int ite, bool chain)
{
    int rc;
    d->last_iters = std::min(ite, d->cfg.n_ite);
    if ((rc = post_ballots<V>(d))) return rc;
    if (chain) {
        /* a wait that ran into its bound left the fault word set: the decode cannot be trusted; say so and go back to a launch per layer */
        int ctl[4] = {0, 0, 0, 0};
        HIPCHK(hipMemcpyAsync(ctl, d->d_chain_ctl, sizeof(ctl), hipMemcpyDeviceToHost, d->stream));
        HIPCHK(hipStreamSynchronize(d->stream));
        if (getenv("QLDPC_DEBUG")) fprintf(stderr, "libqldpc: one-launch layered sweeps: %d sweeps x %d checks x %d groups, %d checks waited for a predecessor, %d polls on top\n", d->last_iters, d->M, d->G, ctl[2], ctl[3]);
        if (ctl[1]) {
            d->chain = 0;
            qldpc_set_error("layered decode: a dependency wait of the one-launch sweep timed out (decoder switched back to a launch per layer; run again)");
            return QLDPC_EHIP;
        }
    }
    return QLDPC_OK;
}

template <int V>
static int run_layered(qldpc_decoder *d)
{
    int rc;
    const int n_ite = d->cfg.n_ite;
    /* A decoder sized for more frames than the call brought (the sessions' decoders take every batch up to max_blocks) runs its sweeps over the
     * groups that hold frames only.  The layered schedule has no generations: d->G only sizes grids, copies and the status pass, the arrays are
     * strided per group.  Empty groups were skipped inside the kernels before, but their workgroups were still dispatched -- 23 small launches per
     * sweep each carrying up to 8 x the workgroups: the config-3 stream on session decoders sized for 512 blocks 15.7 -> 13.65 ms (sized for 256: 13.9 -> 13.5). */
    live_groups live_guard(d);
    bool chain = false;
    if ((rc = layered_begin<V>(d, &chain))) return rc;
    int ite = 0;
    for (; ite < n_ite; ite++) {
        if ((rc = layered_sweep<V>(d, ite, chain))) return rc;
        if (d->cfg.enable_syndrome) {
            if ((rc = layered_test_ballots<V>(d))) return rc;
            /* the live lanes are followed only where the run can compact (compact = 1).  A compaction never comes before sweep 0 is done, so the
             * "messages are zero" shortcut of that sweep and the remap read never meet. */
            bool stop;
            if ((rc = early_exit_step<V>(d, ite + 1, d->compact_mode != 2, &stop))) return rc;
            if (stop) { ite++; break; }
        }
    }
    return layered_end<V>(d, ite, chain);
}

/*
 * Vertical-layered run (qldpc_kernels_vl.h): state and per-sweep chain as in run_layered -- var_nodes = Y_N from whatever load formed the frames,
 * one launch per class, then ballots -> syndrome -> status after EVERY sweep, the last included.  The messages are cleared at run start: sweep 0
 * already reads messages written earlier in the same sweep, so the horizontal sweep's "take them as zero" shortcut does not hold.
 */
template <int V>
static int run_vlayered(qldpc_decoder *d)
{
    int rc;
    const int n_ite = d->cfg.n_ite;
    live_groups live_guard(d);      /* sweeps run over the groups that hold frames only (see run_layered) */
    const size_t G = (size_t)d->G, FG = (size_t)d->FG;
    HIPCHK(hipMemcpyAsync(d->d_a, d->d_llr, G * d->N * FG * sizeof(float), hipMemcpyDeviceToDevice, d->stream));   /* var_nodes = Y_N */
    HIPCHK(hipMemsetAsync(d->d_b, 0, G * d->E * FG * sizeof(float), d->stream));                                   /* messages = 0 */
    int ite = 0;
    for (; ite < n_ite; ite++) {
        {
            prof_scope ps(d, KS_VLAYER, bytes_layer(d), d->vl_rows * 4.0 * live_frames(d));
            for (auto &b : d->vlayer_classes) { qldpc_launch_vlayer<V>(d, b); LAUNCHCHK(); }
        }
        if (d->cfg.enable_syndrome) {
            {
                prof_scope ps(d, KS_SYND, 0.0, (double)d->N * 4.0 * d->n_frames);
                if ((rc = post_ballots<V>(d))) return rc;
            }
            bool stop;
            if ((rc = early_exit_step<V>(d, ite + 1, d->compact_mode != 2, &stop))) return rc;      /* create forces compact_mode = 2 for this schedule: no live lanes, no compaction */
            if (stop) { ite++; break; }
        }
    }
    d->last_iters = std::min(ite, n_ite);
    return post_ballots<V>(d);
}

/* what every FRAMES run starts and ends with (run_v; gang_run per member) */
template <int V>
static int run_begin(qldpc_decoder *d)
{
    view_reset(d);
    gen0_capture(d);
    d->compactions = 0;
    d->live_lanes = 0;
    {
        prof_scope ps(d, KS_STATUS, 0.0);
        if (d->gu.patience > 0)
            hipLaunchKernelGGL((qk_status_init_count<V>), dim3((unsigned)d->G), dim3(64), 0, d->stream, d->d_unsat, d->d_done, d->d_depth, d->d_iters, d->n_frames, d->cfg.n_ite, d->d_work, d->d_active, d->gu);
        else
            hipLaunchKernelGGL((qk_status_init<V>), dim3((unsigned)d->G), dim3(64), 0, d->stream, d->d_unsat, d->d_done, d->d_depth, d->d_iters, d->n_frames, d->cfg.n_ite, d->d_work, d->d_active);
        LAUNCHCHK();
    }
    return QLDPC_OK;
}
template <int V>
static int run_end(qldpc_decoder *d)
{
    /* success flag: syndrome of the hard decision, in every generation (a frame's result lives where it converged) */
    int rc = QLDPC_OK;
    const int last = d->cur_gen;
    for (int k = 0; k <= last && !rc; k++) {
        use_gen(d, k);
        if (hipMemsetAsync(d->d_unsat, 0, sizeof(u64) * (size_t)d->G * V, d->stream) != hipSuccess) rc = QLDPC_EHIP;
        if (!rc) rc = synd_pass<V>(d, d->d_hard, 0);
    }
    use_gen(d, last);
    return rc;
}

template <int V>
static int run_v(qldpc_decoder *d)
{
    int rc;
    if ((rc = run_begin<V>(d))) return rc;
    rc = d->cfg.schedule == QLDPC_SCHED_FLOODING ? run_flooding<V>(d) : (d->cfg.schedule == QLDPC_SCHED_VLAYERED ? run_vlayered<V>(d) : run_layered<V>(d));
    if (rc) return rc;
    return run_end<V>(d);
}

/* fn(origin, final_mask, n_slots) launches once per generation, with that generation's view in place: which slots hold a frame's result
 * and where it belongs in the caller's batch (qk_result_frame).  The launch is checked here */
template <typename F>
static int for_each_gen(qldpc_decoder *d, F fn)
{
    const int last = d->cur_gen;
    int rc = QLDPC_OK;
    for (int k = 0; k <= last && !rc; k++) {
        use_gen(d, k);
        const gen_state &n = d->gens[(size_t)k];
        rc = [&]() -> int { fn(n.origin, k < last ? (const u64 *)n.done : (const u64 *)nullptr, k == 0 ? d->n_frames : n.G * d->FG); LAUNCHCHK(); return QLDPC_OK; }();
    }
    use_gen(d, last);
    return rc;
}

extern "C" int qldpc_run(qldpc_decoder *d)
{
    if (!d) return QLDPC_EINVAL;
    if (!d->loaded) { qldpc_set_error("qldpc_run: nothing loaded"); return QLDPC_ESTATE; }
    HIPCHK(hipSetDevice(d->device));
    const int rc = d->engine == QLDPC_ENGINE_EDGES ? edge_run(d) : with_v(d, [&](auto v) { return run_v<v()>(d); });
    if (rc == QLDPC_OK) d->ran = 1;
    return rc;
}

/* ------------------------------------------------------------------ decoder gangs ------------ */

/* the member's qk_gang_entry array: what its solo layer launches pass as arguments, written once */
static int gang_entries(qldpc_decoder *d)
{
    if (d->d_gang) return QLDPC_OK;
    std::vector<qk_gang_entry> h;
    d->gang_off.clear();
    for (int l = 0; l < d->n_layers; l++) {
        d->gang_off.push_back((int)h.size());
        for (auto &b : d->layer_buckets[(size_t)l]) {
            qk_gang_entry e{};
            qk_gang_set(e.post, d->d_a); qk_gang_set(e.msg, d->d_b); qk_gang_set(e.done, d->d_done);
            qk_gang_set(e.list, b.d_list); qk_gang_set(e.rec, b.cap > 0 ? b.d_rec : (int *)nullptr);
            qk_gang_set(e.cn_ptr, d->d_cn_ptr); qk_gang_set(e.cn_var, d->d_cn_var);
            e.group_stride = (size_t)d->E * d->FG;
            e.n = b.n; e.rec_stride = QK_REC_HDR + b.cap; e.N = d->N; e.M = d->M;
            e.rule = rule_of(d); e.freeze = d->freeze;
            h.push_back(e);
        }
    }
    HIPCHK(hipSetDevice(d->device));
    int rc = dm_alloc(&d->mem, &d->d_gang, std::max<size_t>(h.size(), 1));
    if (rc) return rc;
    HIPCHK(hipMemcpy(d->d_gang, h.data(), h.size() * sizeof(qk_gang_entry), hipMemcpyHostToDevice));
    return QLDPC_OK;
}

extern "C" int qldpc_gang_create(qldpc_decoder *const *members, int n, qldpc_gang **out)
{
    if (!out) return QLDPC_EINVAL;
    *out = nullptr;
    if (!members || n < 1 || n > QLDPC_GANG_MAX_MEMBERS) { qldpc_set_error("qldpc_gang_create: %d members (1 .. %d)", n, QLDPC_GANG_MAX_MEMBERS); return QLDPC_EINVAL; }
    for (int i = 0; i < n; i++) {
        const qldpc_decoder *d = members[i];
        if (!d) { qldpc_set_error("qldpc_gang_create: member %d is NULL", i); return QLDPC_EINVAL; }
        for (int j = 0; j < i; j++) if (members[j] == d) { qldpc_set_error("qldpc_gang_create: member %d is member %d again", i, j); return QLDPC_EINVAL; }
        const char *why = nullptr;
        if (d->engine != QLDPC_ENGINE_FRAMES) why = "not on the FRAMES engine";
        else if (d->cfg.schedule != QLDPC_SCHED_HLAYERED) why = "schedule is not QLDPC_SCHED_HLAYERED";
        else if (d->msg_i8 || d->msg_half) why = "messages are not fp32";
        else if (d->V != 1) why = "frame groups are not 64 wide (frames_per_lane != 1)";
        else if (d->compact_mode != 2) why = "active-frame compaction is enabled";
        else if (d->chain || d->cfg.layer_chain == 1) why = "the one-launch sweep (layer_chain) is in use";
        else if (d->gu.patience > 0) why = "giveup_patience is set (a gang has no give-up rule: create the member with giveup_patience = 0)";
        if (why) { qldpc_set_error("qldpc_gang_create: member %d: %s", i, why); return QLDPC_EUNSUPPORTED; }
        if (d->device != members[0]->device) { qldpc_set_error("qldpc_gang_create: member %d is on device %d, member 0 on device %d", i, d->device, members[0]->device); return QLDPC_EINVAL; }
        if (d->cfg.n_ite != members[0]->cfg.n_ite || !d->cfg.enable_syndrome != !members[0]->cfg.enable_syndrome) {
            qldpc_set_error("qldpc_gang_create: member %d has n_ite=%d, enable_syndrome=%d, member 0 has %d, %d (a gang sweeps in lockstep)", i, d->cfg.n_ite, d->cfg.enable_syndrome,
                            members[0]->cfg.n_ite, members[0]->cfg.enable_syndrome);
            return QLDPC_EINVAL;
        }
    }
    qldpc_gang *g = new (std::nothrow) qldpc_gang();
    if (!g) return QLDPC_ENOMEM;
    g->device = members[0]->device;
    g->stream = members[0]->stream;
    for (int i = 0; i < n; i++) {
        qldpc_decoder *d = members[i];
        int rc = gang_entries(d);
        if (rc) { delete g; return rc; }
        g->m.push_back(d);
        int nb = 0;
        for (int l = 0; l < d->n_layers; l++) {
            const auto &bs = d->layer_buckets[(size_t)l];
            for (size_t k = 0; k < bs.size(); k++) gang_plan_add(g->steps, l, bs[k].cap, family_of(d->cfg.rule), d->layer_cst, gang_slot{i, d->gang_off[(size_t)l] + (int)k, bs[k].n});
            nb += (int)bs.size();
        }
        g->buckets.push_back(nb);
    }
    *out = g;
    return QLDPC_OK;
}

extern "C" void qldpc_gang_free(qldpc_gang *g) { delete g; }

extern "C" int qldpc_gang_set_stream(qldpc_gang *g, void *hip_stream)
{
    if (!g) return QLDPC_EINVAL;
    HIPCHK(hipSetDevice(g->device));
    int rc;
    for (auto *d : g->m) if ((rc = qldpc_stream_switch(&d->stream, hip_stream))) return rc;
    g->stream = (hipStream_t)hip_stream;
    return QLDPC_OK;
}

extern "C" int qldpc_gang_last_run_stats(qldpc_gang *g, long long out[4])
{
    if (!g || !out) return QLDPC_EINVAL;
    for (int k = 0; k < 4; k++) out[k] = g->stats[k];
    return QLDPC_OK;
}

/* the planning of qldpc_gang_create as a function of the codes alone: a check's bucket is the smallest of CN_CAPS that holds its degree, else 0 */
extern "C" int qldpc_gang_plan(const qldpc_code *const *codes, const int *rule, const int *compressed, int n, int *steps, int *launches_per_sweep, int *solo_launches_per_sweep)
{
    if (!codes || !rule || n < 1 || n > QLDPC_GANG_MAX_MEMBERS) { qldpc_set_error("qldpc_gang_plan: %d codes (1 .. %d), codes and rules must be given", n, QLDPC_GANG_MAX_MEMBERS); return QLDPC_EINVAL; }
    gang_steps plan;
    int solo = 0;
    for (int i = 0; i < n; i++) {
        const qldpc_code *c = codes[i];
        if (!c || rule[i] < QLDPC_RULE_MS || rule[i] > QLDPC_RULE_AMS_MINSTAR) { qldpc_set_error("qldpc_gang_plan: code %d: NULL or rule out of range", i); return QLDPC_EINVAL; }
        const int fam = family_of(rule[i]), cst = compressed && compressed[i] ? 1 : 0;
        if (cst && ((fam != QK_FAM_MS && fam != QK_FAM_AMS) || c->max_dc > 32)) {
            qldpc_set_error("qldpc_gang_plan: code %d: the compressed check state takes the min-sum and AMS rules and check degrees <= 32", i);
            return QLDPC_EINVAL;
        }
        for (int l = 0; l < c->n_layers; l++) {
            int cnt[5] = {0, 0, 0, 0, 0};
            for (int k = c->layer_ptr[l]; k < c->layer_ptr[l + 1]; k++) {
                const int id = c->layer_order[k], deg = c->cn_ptr[id + 1] - c->cn_ptr[id];
                int b = 4;
                for (int q = 0; q < 4; q++) if (deg <= CN_CAPS[q]) { b = q; break; }
                cnt[b]++;
            }
            for (int q = 0; q < 5; q++)
                if (cnt[q]) { gang_plan_add(plan, l, q < 4 ? CN_CAPS[q] : 0, fam, cst, gang_slot{i, 0, cnt[q]}); solo++; }
        }
    }
    int launches = 0;
    for (auto &st : plan) launches += (int)st.size();
    if (steps) *steps = (int)plan.size();
    if (launches_per_sweep) *launches_per_sweep = launches;
    if (solo_launches_per_sweep) *solo_launches_per_sweep = solo;
    return QLDPC_OK;
}

/* one class of one step for the members still taking part, QK_GANG_SLOTS to a launch */
static int gang_launch_class(qldpc_gang *g, const gang_class &c, const bool *live, bool first_sweep)
{
    qk_gang_args a;
    int k = 0;
    auto flush = [&]() -> int {
        for (int j = k; j < QK_GANG_SLOTS; j++) { a.entry[j] = a.entry[0]; a.synd[j] = a.synd[0]; a.prefix[j + 1] = a.prefix[k]; }
        int rc = qldpc_launch_layer_gang(g->stream, c.cap, c.fam, c.cst, a, (unsigned)a.prefix[k]);
        if (rc) return rc;
        LAUNCHCHK();
        g->stats[1]++;
        k = 0;
        return QLDPC_OK;
    };
    for (const auto &s : c.slots) {
        if (!live[s.member]) continue;
        const qldpc_decoder *d = g->m[(size_t)s.member];
        const long long blocks = (long long)grid_x(s.n, 1) * d->G;      /* d->G: the groups that hold frames (live_groups) */
        if (blocks > 0x7fffffffLL) { qldpc_set_error("qldpc_gang_run: member %d: %lld workgroups in one step", s.member, blocks); return QLDPC_ESIZE; }
        if (k > 0 && (k == QK_GANG_SLOTS || (long long)a.prefix[k] + blocks > 0x7fffffffLL)) { int rc = flush(); if (rc) return rc; }
        if (k == 0) { a.prefix[0] = 0; a.first = 0u; }
        qk_gang_set(a.entry[k], d->d_gang + s.entry);
        qk_gang_set(a.synd[k], target_synd(d));
        a.prefix[k + 1] = a.prefix[k] + (int)blocks;
        if (first_sweep && layered_skip_clear(d)) a.first |= 1u << k;      /* sweep 0: the member's messages are taken as zero (layered_sweep) */
        k++;
    }
    return k > 0 ? flush() : QLDPC_OK;
}

extern "C" int qldpc_gang_run(qldpc_gang *g, const unsigned char *take)
{
    if (!g) return QLDPC_EINVAL;
    const int n = (int)g->m.size();
    bool live[QLDPC_GANG_MAX_MEMBERS], in[QLDPC_GANG_MAX_MEMBERS];
    int left = 0, first_in = -1;
    for (int i = 0; i < n; i++) {
        in[i] = live[i] = !take || take[i];
        if (!in[i]) continue;
        if (!g->m[(size_t)i]->loaded) { qldpc_set_error("qldpc_gang_run: member %d has nothing loaded", i); return QLDPC_ESTATE; }
        if (first_in < 0) first_in = i;
        left++;
    }
    for (int k = 0; k < 4; k++) g->stats[k] = 0;
    if (!left) return QLDPC_OK;
    HIPCHK(hipSetDevice(g->device));
    int rc;
    /* one stream for the whole gang: a member that was moved to another stream since is brought back by the stream switch (qldpc_hip.h) */
    for (int i = 0; i < n; i++)
        if (in[i] && (rc = qldpc_stream_switch(&g->m[(size_t)i]->stream, (void *)g->stream))) return rc;
    const int n_ite = g->m[(size_t)first_in]->cfg.n_ite;
    const bool synd = g->m[(size_t)first_in]->cfg.enable_syndrome != 0;
    /* the host looks at the mailboxes every p sweeps, p = the smallest poll_every a member asks for; none asks: every sweep is issued and the
     * kernels return early for converged groups, as in a small solo run */
    int p = 0;
    std::optional<live_groups> lg[QLDPC_GANG_MAX_MEMBERS];
    int swept[QLDPC_GANG_MAX_MEMBERS];
    for (int i = 0; i < n; i++) {
        if (!in[i]) continue;
        qldpc_decoder *d = g->m[(size_t)i];
        if (d->poll_every > 0 && (p == 0 || d->poll_every < p)) p = d->poll_every;
        bool chain;
        if ((rc = run_begin<1>(d))) return rc;
        lg[i].emplace(d);
        if ((rc = layered_begin<1>(d, &chain))) return rc;
        swept[i] = 0;
    }
    int ite = 0;
    for (; ite < n_ite && left > 0; ite++) {
        {
            qldpc_decoder *lead = nullptr;
            double bytes = 0.0, moved = 0.0;
            for (int i = 0; i < n; i++)
                if (live[i]) { qldpc_decoder *d = g->m[(size_t)i]; if (!lead) lead = d; bytes += bytes_layer(d); moved += moved_layer(d); g->stats[2] += g->buckets[(size_t)i]; swept[i] = ite + 1; }
            prof_scope ps(lead, KS_LAYER_GANG, bytes, moved);      /* one record per sweep, as KS_LAYER, on the first member taking part */
            for (const auto &step : g->steps)
                for (const auto &c : step)
                    if ((rc = gang_launch_class(g, c, live, ite == 0))) return rc;
            g->stats[0]++;
        }
        if (!synd) continue;
        for (int i = 0; i < n; i++)
            if (live[i] && ((rc = layered_test_ballots<1>(g->m[(size_t)i])) || (rc = early_exit_launch<1>(g->m[(size_t)i], ite + 1)))) return rc;
        if (p <= 0 || ((ite + 1) % p) != 0) continue;
        for (int i = 0; i < n; i++) {
            if (!live[i]) continue;
            bool stop;
            if ((rc = early_exit_poll<1>(g->m[(size_t)i], ite + 1, false, &stop))) return rc;
            if (stop) { live[i] = false; left--; }
        }
    }
    for (int i = 0; i < n; i++) {
        if (!in[i]) continue;
        qldpc_decoder *d = g->m[(size_t)i];
        if (swept[i] < (int)g->stats[0]) g->stats[3]++;      /* left before the last sweep */
        if ((rc = layered_end<1>(d, swept[i], false))) return rc;
        lg[i].reset();
        if ((rc = run_end<1>(d))) return rc;
        d->ran = 1;
    }
    return QLDPC_OK;
}

/* ------------------------------------------------------------------ load --------------------- */

static int check_frames(qldpc_decoder *d, int n_frames, const char *who)
{
    if (n_frames <= 0 || n_frames > d->cfg.max_frames) {
        qldpc_set_error("%s: n_frames=%d not in [1, max_frames=%d]", who, n_frames, d->cfg.max_frames);
        return QLDPC_ESIZE;
    }
    return QLDPC_OK;
}

/* what every load of a batch opens with: the frame count checked, the device, the view of the batch as loaded, and the state of the batch
 * before it (target syndromes, erasures, known bits, the coded form) gone.  end_load (qldpc_engine_int.h) closes the call */
static int begin_load(qldpc_decoder *d, int n_frames, const char *who)
{
    int rc = check_frames(d, n_frames, who);
    if (rc) return rc;
    HIPCHK(hipSetDevice(d->device));
    view_reset(d);
    d->n_frames = n_frames;
    d->has_synd = d->has_erase = d->has_known = d->llr_coded = 0;
    return QLDPC_OK;
}

/* the loads that add to a batch (target syndromes, erasures, known bits) take the frame count of the batch in place */
static int need_loaded(qldpc_decoder *d, int n_frames, const char *who)
{
    if (!d->loaded || n_frames != d->n_frames) { qldpc_set_error("%s: load %d frames first (have %d)", who, n_frames, d->loaded ? d->n_frames : 0); return QLDPC_ESTATE; }
    HIPCHK(hipSetDevice(d->device));
    view_reset(d);
    return QLDPC_OK;
}

/* 8-bit messages: dword-wise passes over the [G][N][64] dwords of the quantised LLRs / posteriors */
static inline size_t i8_dwords(const qldpc_decoder *d) { return (size_t)d->G * d->N * 64; }
static inline dim3 i8_grid(const qldpc_decoder *d) { return dim3((unsigned)std::min<size_t>((i8_dwords(d) + 255) / 256, 16384)); }
static int quantise_llr(qldpc_decoder *d)
{
    hipLaunchKernelGGL(qi_quant_llr, i8_grid(d), dim3(256), 0, d->stream, d->d_llr, d->d_llr8, i8_dwords(d), d->quant_scale);
    LAUNCHCHK();
    return QLDPC_OK;
}

extern "C" int qldpc_load_llr_dev(qldpc_decoder *d, const float *d_llr, int n_frames)
{
    if (!d || !d_llr) return QLDPC_EINVAL;
    int rc = begin_load(d, n_frames, "qldpc_load_llr_dev");
    if (rc) return rc;
    if (d->engine == QLDPC_ENGINE_EDGES) return edge_load_llr(d, d_llr);
    if ((rc = ensure_llr(d))) return rc;
    {
        prof_scope ps(d, KS_LOAD, 2.0 * d->N * 4.0 * n_frames);
        dim3 grid((unsigned)((d->N + 63) / 64), (unsigned)d->G);
        with_v(d, [&](auto v) { hipLaunchKernelGGL((qk_load_llr<v()>), grid, dim3(256), 0, d->stream, d_llr, d->d_llr, d->N, n_frames); });
        LAUNCHCHK();
        if (d->msg_i8 && (rc = quantise_llr(d))) return rc;
    }
    end_load(d);
    return QLDPC_OK;
}

extern "C" int qldpc_load_bits_dev(qldpc_decoder *d, const uint32_t *d_bits, const float *d_llr_mag, const uint8_t *d_vn_class, int n_frames)
{
    return qldpc_load_bits_short_dev(d, d_bits, d_llr_mag, d_vn_class, nullptr, n_frames);
}

/* as qldpc_load_bits_dev, with a per-frame count of channel VNs: class-0 VNs at index >= d_n_channel[f] are known bits of
 * frame f (shortening: blocks of different length sharing one code), i.e. pinned like class 1 */
extern "C" int qldpc_load_bits_short_dev(qldpc_decoder *d, const uint32_t *d_bits, const float *d_llr_mag, const uint8_t *d_vn_class, const int *d_n_channel, int n_frames)
{
    if (!d || !d_bits || !d_llr_mag) return QLDPC_EINVAL;
    int rc = begin_load(d, n_frames, "qldpc_load_bits_dev");
    if (rc) return rc;
    if (d->engine == QLDPC_ENGINE_EDGES) return edge_load_bits(d, d_bits, d_llr_mag, d_vn_class, d_n_channel);
    const int W = words32(d->N);
    const dim3 grid = grid_4k(d, W);
    if (d->d_ybits) {
        /* flooding, fp32 / binary16 messages: keep the received bits as ballots and rebuild Y in the VN passes (qk_coded_llr) */
        prof_scope ps(d, KS_LOAD, ((double)W * 4.0 + d->N / 8.0) * n_frames);
        with_v(d, [&](auto v) { hipLaunchKernelGGL((qk_load_syndrome<v()>), grid, dim3(QK_THREADS), 0, d->stream, d_bits, d->d_ybits, d->N, W, n_frames); });
        LAUNCHCHK();
        const int total = d->G * d->FG;
        hipLaunchKernelGGL(qk_load_frame_consts, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, d->stream, d_llr_mag, d_n_channel, d->d_fmag, d->d_fnch, n_frames, total, d->N);
        LAUNCHCHK();
        if (d_vn_class) HIPCHK(hipMemcpyAsync(d->d_vcls, d_vn_class, (size_t)d->N, hipMemcpyDeviceToDevice, d->stream));
        else HIPCHK(hipMemsetAsync(d->d_vcls, 0, (size_t)d->N, d->stream));
        d->llr_coded = 1;
    } else if (d->msg_i8) {
        /* 8-bit variant: straight into the quantised array, no fp32 LLRs in between */
        prof_scope ps(d, KS_LOAD, ((double)W * 4.0 + d->N) * n_frames);
        hipLaunchKernelGGL(qi_load_bits, grid, dim3(QK_THREADS), 0, d->stream, d_bits, d_llr_mag, d_vn_class, d->d_llr8, d->N, W, n_frames, d_n_channel, d->quant_scale);
        LAUNCHCHK();
    } else {
        if ((rc = ensure_llr(d))) return rc;
        prof_scope ps(d, KS_LOAD, ((double)W * 4.0 + d->N * 4.0) * n_frames);
        with_v(d, [&](auto v) { hipLaunchKernelGGL((qk_load_bits<v()>), grid, dim3(QK_THREADS), 0, d->stream, d_bits, d_llr_mag, d_vn_class, d->d_llr, d->N, W, n_frames, d_n_channel); });
        LAUNCHCHK();
    }
    end_load(d);
    return QLDPC_OK;
}

/* syndrome form: target syndromes for the frames just loaded (cleared again by the next qldpc_load_*) */
extern "C" int qldpc_load_syndrome_dev(qldpc_decoder *d, const uint32_t *d_synd_bits, int n_frames)
{
    if (!d || !d_synd_bits) return QLDPC_EINVAL;
    int rc = need_loaded(d, n_frames, "qldpc_load_syndrome_dev");
    if (rc) return rc;
    if (d->engine == QLDPC_ENGINE_EDGES) return edge_load_syndrome(d, d_synd_bits);
    const int Wm = words32(d->M);
    if (!d->d_synd && (rc = dm_alloc(&d->mem, &d->d_synd, (size_t)d->G * d->M * d->V))) return rc;
    const dim3 grid = grid_4k(d, Wm);
    with_v(d, [&](auto v) { hipLaunchKernelGGL((qk_load_syndrome<v()>), grid, dim3(QK_THREADS), 0, d->stream, d_synd_bits, d->d_synd, d->M, Wm, n_frames); });
    LAUNCHCHK();
    d->has_synd = 1; d->ran = 0;
    return QLDPC_OK;
}

static int apply_known(qldpc_decoder *d);      /* the known bits of qldpc_load_known_dev, below */

/*
 * Per-frame puncturing: d_erase_bits[n_frames][ceil(N/32)] packed MSB-first, a set bit makes that VN of that frame an erasure
 * (channel LLR 0, BS/src/main.cpp:359-362) whatever its class.  For the frames just loaded (cleared again by the next qldpc_load_*).
 */
extern "C" int qldpc_load_erasures_dev(qldpc_decoder *d, const uint32_t *d_erase_bits, int n_frames)
{
    if (!d || !d_erase_bits) return QLDPC_EINVAL;
    int rc = need_loaded(d, n_frames, "qldpc_load_erasures_dev");
    if (rc) return rc;
    if (d->engine == QLDPC_ENGINE_EDGES) return edge_erase(d, d_erase_bits);
    const int W = words32(d->N);
    const dim3 grid = grid_4k(d, W);
    if (d->llr_coded) {
        if (!d->d_ebits && (rc = dm_alloc(&d->mem, &d->d_ebits, (size_t)d->G * d->N * d->V))) return rc;
        with_v(d, [&](auto v) { hipLaunchKernelGGL((qk_load_syndrome<v()>), grid, dim3(QK_THREADS), 0, d->stream, d_erase_bits, d->d_ebits, d->N, W, n_frames); });
        LAUNCHCHK();
        d->has_erase = 1; d->ran = 0;
        return QLDPC_OK;
    }
    if (d->msg_i8) hipLaunchKernelGGL((qk_erase_rows<4, uint8_t>), grid, dim3(QK_THREADS), 0, d->stream, d_erase_bits, (uint8_t *)d->d_llr8, d->N, W, n_frames);
    else {
        with_v(d, [&](auto v) { hipLaunchKernelGGL((qk_erase_rows<v(), float>), grid, dim3(QK_THREADS), 0, d->stream, d_erase_bits, d->d_llr, d->N, W, n_frames); });
    }
    LAUNCHCHK();
    d->ran = 0;
    return d->has_known ? apply_known(d) : (int)QLDPC_OK;      /* known wins over erased */
}

/*
 * Known bits (blind reconciliation): d_known_bits / d_value_bits[n_frames][ceil(N/32)] packed MSB-first, a set known bit pins that VN of that frame
 * to its value bit (channel LLR +-23.03, the 8-bit form what that quantises to) whatever its class and whether or not it is erased.  For the frames
 * just loaded (cleared again by the next qldpc_load_*).  A frame set in the coded-LLR form is written out as the LLR array it stands for and runs
 * on that: the same floats reach the passes.  The masks are kept so that erasures loaded afterwards leave the known bits standing.
 */
static int apply_known(qldpc_decoder *d)
{
    if (d->engine == QLDPC_ENGINE_EDGES) return edge_known(d);
    const int W = words32(d->N);
    const uint32_t *kn = d->d_known, *val = d->d_known + (size_t)d->cfg.max_frames * W;
    const dim3 grid = grid_4k(d, W);
    if (d->msg_i8) {
        const int q = (int)lrintf(std::min(127.0f, QLDPC_CONFIRMED_BIT_LLR * d->quant_scale));      /* qi_quant1 of the pin */
        hipLaunchKernelGGL((qk_known_rows<4, uint8_t>), grid, dim3(QK_THREADS), 0, d->stream, kn, val, (uint8_t *)d->d_llr8, d->N, W, d->n_frames, (uint8_t)q, (uint8_t)(-q));
    } else {
        with_v(d, [&](auto v) { hipLaunchKernelGGL((qk_known_rows<v(), float>), grid, dim3(QK_THREADS), 0, d->stream, kn, val, d->d_llr, d->N, W, d->n_frames, QLDPC_CONFIRMED_BIT_LLR, -QLDPC_CONFIRMED_BIT_LLR); });
    }
    LAUNCHCHK();
    return QLDPC_OK;
}

extern "C" int qldpc_load_known_dev(qldpc_decoder *d, const uint32_t *d_known_bits, const uint32_t *d_value_bits, int n_frames)
{
    if (!d || !d_known_bits || !d_value_bits) return QLDPC_EINVAL;
    int rc = need_loaded(d, n_frames, "qldpc_load_known_dev");
    if (rc) return rc;
    const int W = words32(d->N);
    if (!d->d_known && (rc = dm_alloc(&d->mem, &d->d_known, (size_t)d->cfg.max_frames * W * 2))) return rc;
    HIPCHK(hipMemcpyAsync(d->d_known, d_known_bits, sizeof(uint32_t) * (size_t)n_frames * W, hipMemcpyDeviceToDevice, d->stream));
    HIPCHK(hipMemcpyAsync(d->d_known + (size_t)d->cfg.max_frames * W, d_value_bits, sizeof(uint32_t) * (size_t)n_frames * W, hipMemcpyDeviceToDevice, d->stream));
    if (d->llr_coded) {      /* the FRAMES engine's coded form (the edge engine has none) */
        if ((rc = ensure_llr(d))) return rc;
        const qk_coded_llr coded = coded_llr_of(d);
        const dim3 grid((unsigned)std::max(1, std::min((d->N + QK_WAVES - 1) / QK_WAVES, 4096)), (unsigned)d->G);
        with_v(d, [&](auto v) { hipLaunchKernelGGL((qk_decode_llr<v()>), grid, dim3(QK_THREADS), 0, d->stream, coded, d->d_llr, d->N); });
        LAUNCHCHK();
        if (d->msg_i8 && (rc = quantise_llr(d))) return rc;
        d->llr_coded = 0; d->has_erase = 0;      /* the erasures are in the array now */
    }
    if ((rc = apply_known(d))) return rc;
    d->has_known = 1; d->ran = 0;
    return QLDPC_OK;
}

/* allocate now what the load calls would allocate on first use (the per-frame erasure ballots of the coded-LLR form), so that a
 * caller who must not allocate later -- the daemon after ldpc_init -- can say so */
extern "C" int qldpc_decoder_reserve(qldpc_decoder *d)
{
    if (!d) return QLDPC_EINVAL;
    HIPCHK(hipSetDevice(d->device));
    view_reset(d);
    return d->d_ybits && !d->d_ebits ? dm_alloc(&d->mem, &d->d_ebits, (size_t)d->G0 * d->N * d->V) : (int)QLDPC_OK;
}

/* s = H x on the device for packed words (Alice's side of the syndrome form; also a codeword test) */
extern "C" int qldpc_syndrome_dev(qldpc_decoder *d, const uint32_t *d_bits, uint32_t *d_synd_bits, int n_frames)
{
    if (!d || !d_bits || !d_synd_bits || n_frames <= 0) return QLDPC_EINVAL;
    HIPCHK(hipSetDevice(d->device));
    const int Wn = words32(d->N), Wm = words32(d->M);
    hipLaunchKernelGGL(qk_syndrome_of_bits, dim3((unsigned)((Wm + 255) / 256), (unsigned)n_frames), dim3(256), 0, d->stream, d_bits, d->d_cn_ptr, d->d_cn_var, d_synd_bits,
                       d->M, Wn, Wm);
    LAUNCHCHK();
    return QLDPC_OK;
}

/* ------------------------------------------------------------------ fetch -------------------- */

/* what every fetch opens with: a completed run, the device */
static int need_ran(qldpc_decoder *d, const char *who)
{
    if (!d->ran) { qldpc_set_error("%s: no completed qldpc_run", who); return QLDPC_ESTATE; }
    HIPCHK(hipSetDevice(d->device));
    return QLDPC_OK;
}

extern "C" int qldpc_fetch_packed_dev(qldpc_decoder *d, uint32_t *d_out)
{
    if (!d || !d_out) return QLDPC_EINVAL;
    int rc = need_ran(d, "qldpc_fetch_packed_dev");
    if (rc) return rc;
    const int W = words32(d->N);
    prof_scope ps(d, KS_FETCH, (double)W * 4.0 * d->n_frames);
    if (d->engine == QLDPC_ENGINE_EDGES) return edge_fetch_packed(d, d_out);
    return for_each_gen(d, [&](const int *origin, const u64 *fin, int n_slots) {
        const dim3 grid = grid_4k(d, W);
        with_v(d, [&](auto v) { hipLaunchKernelGGL((qk_fetch_packed<v()>), grid, dim3(QK_THREADS), 0, d->stream, d->d_hard, d_out, d->N, W, n_slots, origin, fin); });
    });
}

extern "C" int qldpc_fetch_info_dev(qldpc_decoder *d, int *d_V_K)
{
    if (!d || !d_V_K) return QLDPC_EINVAL;
    int rc = need_ran(d, "qldpc_fetch_info_dev");
    if (rc) return rc;
    prof_scope ps(d, KS_FETCH, (double)d->K * 4.0 * d->n_frames);
    if (d->engine == QLDPC_ENGINE_EDGES) return edge_fetch_info(d, d_V_K);
    return for_each_gen(d, [&](const int *origin, const u64 *fin, int n_slots) {
        dim3 gk((unsigned)std::max(1, std::min((d->K + 255) / 256, 64)), (unsigned)n_slots);
        with_v(d, [&](auto v) { hipLaunchKernelGGL((qk_fetch_info<v()>), gk, dim3(256), 0, d->stream, d->d_hard, d->d_info_pos, d_V_K, d->N, d->K, n_slots, origin, fin); });
    });
}

extern "C" int qldpc_fetch_status_dev(qldpc_decoder *d, int *d_iters, int *d_ok)
{
    if (!d) return QLDPC_EINVAL;
    int rc = need_ran(d, "qldpc_fetch_status_dev");
    if (rc) return rc;
    if (d->engine == QLDPC_ENGINE_EDGES) return edge_fetch_status(d, d_iters, d_ok);
    return for_each_gen(d, [&](const int *origin, const u64 *fin, int n_slots) {
        dim3 gs((unsigned)((n_slots + 255) / 256));
        with_v(d, [&](auto v) { hipLaunchKernelGGL((qk_status_out<v()>), gs, dim3(256), 0, d->stream, d->d_unsat, d->d_iters, d_iters, d_ok, n_slots, origin, fin); });
    });
}

/* per frame: 1 if the run gave the frame up, its syndrome weight at its last test and the smallest one it showed (qldpc.h) */
extern "C" int qldpc_fetch_giveup_dev(qldpc_decoder *d, int *d_gave, int *d_last_weight, int *d_best_weight)
{
    if (!d) return QLDPC_EINVAL;
    if (d->gu.patience <= 0) { qldpc_set_error("qldpc_fetch_giveup_dev: the decoder counts no syndrome weights: create it with giveup_patience >= 1"); return QLDPC_EUNSUPPORTED; }
    int rc = need_ran(d, "qldpc_fetch_giveup_dev");
    if (rc) return rc;
    return for_each_gen(d, [&](const int *origin, const u64 *fin, int n_slots) {
        dim3 gs((unsigned)((n_slots + 255) / 256));
        with_v(d, [&](auto v) { hipLaunchKernelGGL((qk_giveup_out<v()>), gs, dim3(256), 0, d->stream, d->gu, d_gave, d_last_weight, d_best_weight, n_slots, origin, fin); });
    });
}

/* frames given up by every run since the decoder was created: qk_status_count adds them up on the device.  Synchronises the stream. */
extern "C" int qldpc_giveup_total(qldpc_decoder *d, uint64_t *frames)
{
    if (!d || !frames) return QLDPC_EINVAL;
    *frames = 0;
    if (d->gu.patience <= 0) return QLDPC_OK;
    HIPCHK(hipSetDevice(d->device));
    unsigned long long n = 0;
    HIPCHK(hipMemcpyAsync(&n, d->gu.total, sizeof(n), hipMemcpyDeviceToHost, d->stream));
    HIPCHK(hipStreamSynchronize(d->stream));
    *frames = n;
    return QLDPC_OK;
}

/* the a-posteriori rows of the last run, frame-interleaved [G][N][FG] floats, where they lie or after the pass that makes them (FRAMES engine) */
static int post_rows(qldpc_decoder *d, const char *who, const float **rows)
{
    int rc;
    if (d->cur_gen != 0) {
        qldpc_set_error("%s: the run compacted its active frames (%d times), the messages of frames that converged earlier are gone; "
                        "create the decoder with compact = 2 (or freeze_messages = 1) to read posteriors", who, d->compactions);
        return QLDPC_EUNSUPPORTED;
    }
    if (d->cfg.schedule == QLDPC_SCHED_FLOODING) {
        if ((rc = ensure_post(d))) return rc;
        if (d->fpost) { if ((rc = vn_pass_fpost(d, d->d_post, false)) || (rc = close_fpost(d, d->d_post))) return rc; }
        else if ((rc = with_v(d, [&](auto v) { return vn_pass<v(), QK_VN_POST>(d, d->d_post); }))) return rc;
        *rows = d->d_post;
    } else if (d->msg_i8) {
        if ((rc = ensure_post(d))) return rc;
        hipLaunchKernelGGL(qi_post_to_f32, i8_grid(d), dim3(256), 0, d->stream, (const uint32_t *)d->d_a, d->d_post, i8_dwords(d));
        LAUNCHCHK();
        *rows = d->d_post;
    } else {
        *rows = d->d_a;
    }
    return QLDPC_OK;
}

extern "C" int qldpc_fetch_post_dev(qldpc_decoder *d, float *d_post_out)
{
    if (!d || !d_post_out) return QLDPC_EINVAL;
    int rc = need_ran(d, "qldpc_fetch_post_dev");
    if (rc) return rc;
    if (d->engine == QLDPC_ENGINE_EDGES) return edge_fetch_post(d, d_post_out);
    const float *src;
    if ((rc = post_rows(d, "qldpc_fetch_post_dev", &src))) return rc;
    dim3 grid((unsigned)((d->N + 63) / 64), (unsigned)d->G);
    with_v(d, [&](auto v) { hipLaunchKernelGGL((qk_unload_f32<v()>), grid, dim3(256), 0, d->stream, src, d_post_out, d->N, d->n_frames); });
    LAUNCHCHK();
    return QLDPC_OK;
}

/*
 * Blind reconciliation: row f of d_weak_bits = the select of qldpc_weakest_core.h (the min(d, candidates) smallest |posterior| in (key, v) order)
 * over the floats qldpc_fetch_post_dev returns for frame f, read where they lie (qk_weakest).  Rows of frames not taken are zero.
 */
extern "C" int qldpc_fetch_weakest_dev(qldpc_decoder *d, const uint32_t *d_cand_bits, const int *d_take, int n_weak, uint32_t *d_weak_bits)
{
    if (!d || !d_weak_bits || n_weak < 0) return QLDPC_EINVAL;
    int rc = need_ran(d, "qldpc_fetch_weakest_dev");
    if (rc) return rc;
    if (d->engine == QLDPC_ENGINE_EDGES) {
        qldpc_set_error("qldpc_fetch_weakest_dev: not built for the edge-parallel engine (create the decoder with engine = FRAMES)");
        return QLDPC_EUNSUPPORTED;
    }
    const float *src;
    if ((rc = post_rows(d, "qldpc_fetch_weakest_dev", &src))) return rc;
    const int W = words32(d->N);
    prof_scope ps(d, KS_FETCH, ((double)d->N * 4.0 * (WK_DIGITS + 1) + (double)W * 4.0) * d->n_frames);
    HIPCHK(hipMemsetAsync(d_weak_bits, 0, sizeof(uint32_t) * (size_t)d->n_frames * W, d->stream));
    if (n_weak == 0) return QLDPC_OK;
    hipLaunchKernelGGL(qk_weakest, dim3((unsigned)d->V, (unsigned)d->G), dim3(WK_THREADS), 0, d->stream, src, d->N, d->FG, d->n_frames, d_cand_bits, d_take, (uint32_t)n_weak, d_weak_bits, W);
    LAUNCHCHK();
    return QLDPC_OK;
}

/* ------------------------------------------------------------------ AFF3CT mirror ------------ */

/* decoder->decode_siho(LLRs, dec_bits) with host vectors (BS/src/main.cpp:365): H2D, run, D2H. */
extern "C" int qldpc_decode_siho(qldpc_decoder *d, const float *Y_N, int *V_K, int n_frames)
{
    if (!d || !Y_N || !V_K) return QLDPC_EINVAL;
    int rc = check_frames(d, n_frames, "qldpc_decode_siho");
    if (rc) return rc;
    HIPCHK(hipSetDevice(d->device));
    /* staging buffers for the host-pointer call live with the decoder (sized for max_frames on first use) */
    if (!d->h_in) {
        if ((rc = dm_alloc(&d->mem, &d->h_in, (size_t)d->cfg.max_frames * d->N))) return rc;
        if ((rc = dm_alloc(&d->mem, &d->h_out, (size_t)d->cfg.max_frames * d->K))) return rc;
    }
    float *din = d->h_in; int *dout = d->h_out;
    rc = QLDPC_OK;
    if (hipMemcpyAsync(din, Y_N, sizeof(float) * (size_t)n_frames * d->N, hipMemcpyHostToDevice, d->stream) != hipSuccess) rc = QLDPC_EHIP;
    if (!rc) rc = qldpc_load_llr_dev(d, din, n_frames);
    if (!rc) rc = qldpc_run(d);
    if (!rc) rc = qldpc_fetch_info_dev(d, dout);
    if (!rc && hipMemcpyAsync(V_K, dout, sizeof(int) * (size_t)n_frames * d->K, hipMemcpyDeviceToHost, d->stream) != hipSuccess) rc = QLDPC_EHIP;
    if (hipStreamSynchronize(d->stream) != hipSuccess && !rc) rc = QLDPC_EHIP;
    if (rc == QLDPC_EHIP) qldpc_set_error("decode_siho: HIP failure (%s)", hipGetErrorString(hipGetLastError()));
    return rc;
}
