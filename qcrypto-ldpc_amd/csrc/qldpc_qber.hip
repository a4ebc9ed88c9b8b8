/*
 * qldpc_qber.hip -- the syndrome-weight QBER estimator: context, tables and launches (kernels: qldpc_kernels_qber.h, rule: qldpc_qber_core.h).
 * It needs no decoder: it reads the frame-major packed rows the loads take and runs on the caller's stream.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "qldpc_hip.h"
#include "qldpc_devmem.h"
#include "qldpc_kernels_qber.h"

#define QBER_LDS_MAX (144u * 1024u)      /* of the 160 KB of a CU: the rows of one frame plus the histogram, one workgroup resident */

struct qldpc_qber {
    qldpc_qber_cfg cfg;
    int N, M, D, Wn, Wm, bins;
    int cpb;               /* cfg.checks_per_block (below 256: part of a workgroup idles); 0 = per call from the frame count */
    int staged;            /* the rows of a frame fit the LDS (QLDPC_QBER_STAGE=0: gather from memory all the same) */
    int no_stage;          /* QLDPC_QBER_STAGE=0 was set at creation */
    int merge;             /* qldpc_qber_set_merge: runs across erased chain VNs are one observation, counts have QB_MAX_DEGREE + 1 rows */
    int mstaged;           /* `staged` for the merged kernel's larger histogram */
    size_t mlds_bytes;
    uint8_t *d_rep;        /* [D][M] repeat table (qb_earlier_in_run); its presence = the merged tables and buffers are in place */
    int cus;
    size_t lds_bytes;
    dm_ledger mem;         /* every device array of the estimator (qldpc_devmem.h) */
    hipStream_t stream;
    int *d_tab;            /* [D][M] transposed check table, -1 past a check's degree */
    int32_t *d_L1, *d_L0;  /* [D + 1][n_grid]; after the first qldpc_qber_set_merge(1) [QB_MAX_DEGREE + 1][n_grid], the same rows and more */
    float *d_q, *d_llr;    /* [n_grid] */
    uint32_t *d_cls_rows;  /* [2][Wn] */
    uint32_t *d_counts;    /* [max_frames][rows][2]: used when the caller takes no counts */
    unsigned long long *d_pool;      /* [rows][2] */
    std::vector<float> h_q, h_llr;
    std::vector<int> h_tab;          /* d_tab on the host: qldpc_qber_set_merge verifies the chain and builds the repeat table from it */
};

extern "C" void qldpc_qber_cfg_default(qldpc_qber_cfg *cfg)
{
    if (!cfg) return;
    memset(cfg, 0, sizeof(*cfg));
    cfg->device = 0;
    cfg->max_frames = 1;
    cfg->n_grid = 256;
    cfg->q_lo = 0.001f;      /* the clamp of qldpc_recon_plan */
    cfg->q_hi = 0.25f;
    cfg->checks_per_block = 0;
}

extern "C" void qldpc_qber_free(qldpc_qber *est)
{
    if (!est) return;
    (void)hipSetDevice(est->cfg.device);
    dm_free_all(&est->mem);
    delete est;
}

extern "C" int qldpc_qber_create(const qldpc_code *code, const qldpc_qber_cfg *cfg, qldpc_qber **out)
{
    if (!out) return QLDPC_EINVAL;
    *out = nullptr;
    if (!code || !cfg) return QLDPC_EINVAL;
    if (cfg->max_frames < 1 || cfg->max_frames > 65535 || cfg->checks_per_block < 0) {
        qldpc_set_error("qber_create: max_frames in 1 .. 65535 and checks_per_block >= 0 are required");
        return QLDPC_EINVAL;
    }
    const int N = code->N, M = code->M, D = code->max_dc;
    std::vector<int32_t> L1((size_t)(std::max(D, 1) + 1) * (size_t)std::max(cfg->n_grid, 0)), L0(L1.size());
    std::vector<float> q((size_t)std::max(cfg->n_grid, 0)), llr(q.size());
    int rc = qldpc_qber_table_host(D, cfg->n_grid, cfg->q_lo, cfg->q_hi, L1.data(), L0.data(), q.data(), llr.data());
    if (rc) return rc;
    if ((unsigned long long)cfg->max_frames * (unsigned long long)M >= (1ull << 35)) {
        qldpc_set_error("qber_create: max_frames x M = %d x %d >= 2^35: the pooled score could overflow", cfg->max_frames, M);
        return QLDPC_EUNSUPPORTED;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { qldpc_set_error("no HIP device visible: libqldpc has no CPU fallback"); return QLDPC_ENODEV; }
    if (cfg->device < 0 || cfg->device >= ndev) { qldpc_set_error("device %d out of range", cfg->device); return QLDPC_ENODEV; }
    HIPCHK(hipSetDevice(cfg->device));
    qldpc_qber *e = new (std::nothrow) qldpc_qber();
    if (!e) return QLDPC_ENOMEM;
    e->cfg = *cfg;
    e->N = N; e->M = M; e->D = D; e->Wn = (N + 31) / 32; e->Wm = (M + 31) / 32; e->bins = 2 * (D + 1);
    e->cpb = cfg->checks_per_block;
    e->stream = nullptr;
    e->h_q = q; e->h_llr = llr;
    const size_t staged_bytes = sizeof(uint32_t) * ((size_t)e->bins + 3 * (size_t)e->Wn);
    e->staged = staged_bytes <= QBER_LDS_MAX;
    if (const char *env = getenv("QLDPC_QBER_STAGE")) if (atoi(env) == 0) e->no_stage = 1;
    if (e->no_stage) e->staged = 0;
    e->lds_bytes = e->staged ? staged_bytes : sizeof(uint32_t) * (size_t)e->bins;
    e->cus = 256;
    (void)hipDeviceGetAttribute(&e->cus, hipDeviceAttributeMultiprocessorCount, cfg->device);
    if (e->cus < 1) e->cus = 1;
    /* the check table, transposed so that the threads of a wavefront read neighbouring words */
    std::vector<int> tab((size_t)D * (size_t)M, -1);
    for (int c = 0; c < M; c++)
        for (int k = code->cn_ptr[c]; k < code->cn_ptr[c + 1]; k++) tab[(size_t)(k - code->cn_ptr[c]) * M + c] = code->cn_var[k];
    const size_t tbytes = sizeof(int32_t) * L1.size(), gbytes = sizeof(float) * q.size();
    dm_ledger *m = &e->mem;
    if ((rc = dm_alloc(m, &e->d_tab, tab.size())) || (rc = dm_alloc(m, &e->d_L1, L1.size())) || (rc = dm_alloc(m, &e->d_L0, L0.size())) ||
        (rc = dm_alloc(m, &e->d_q, q.size())) || (rc = dm_alloc(m, &e->d_llr, llr.size())) || (rc = dm_alloc(m, &e->d_cls_rows, 2 * (size_t)e->Wn)) ||
        (rc = dm_alloc(m, &e->d_counts, (size_t)cfg->max_frames * (size_t)e->bins)) || (rc = dm_alloc(m, &e->d_pool, (size_t)e->bins))) {
        qldpc_set_error("qber_create: device allocation failed");
        qldpc_qber_free(e);
        return rc;
    }
    e->h_tab = tab;
    hipError_t he = hipMemcpy(e->d_tab, tab.data(), sizeof(int) * tab.size(), hipMemcpyHostToDevice);
    if (he == hipSuccess) he = hipMemcpy(e->d_L1, L1.data(), tbytes, hipMemcpyHostToDevice);
    if (he == hipSuccess) he = hipMemcpy(e->d_L0, L0.data(), tbytes, hipMemcpyHostToDevice);
    if (he == hipSuccess) he = hipMemcpy(e->d_q, q.data(), gbytes, hipMemcpyHostToDevice);
    if (he == hipSuccess) he = hipMemcpy(e->d_llr, llr.data(), gbytes, hipMemcpyHostToDevice);
    if (he == hipSuccess && e->lds_bytes > 48 * 1024)
        he = hipFuncSetAttribute((const void *)&qk_qber_count<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)e->lds_bytes);
    if (he != hipSuccess) { qldpc_set_error("qber_create: %s", hipGetErrorString(he)); qldpc_qber_free(e); return QLDPC_EHIP; }
    *out = e;
    return QLDPC_OK;
}

extern "C" size_t qldpc_qber_device_bytes(const qldpc_qber *est) { return est ? est->mem.dev_bytes : 0; }

extern "C" int qldpc_qber_set_stream(qldpc_qber *est, void *hip_stream)
{
    if (!est) return QLDPC_EINVAL;
    HIPCHK(hipSetDevice(est->cfg.device));
    return qldpc_stream_switch(&est->stream, hip_stream);
}

extern "C" int qldpc_qber_count_rows(const qldpc_qber *est) { return est ? (est->merge ? QB_MAX_DEGREE + 1 : est->D + 1) : QLDPC_EINVAL; }

/*
 * Merging on or off (qldpc_qber_core.h, MERGING).  The first call that turns it on verifies the chain, uploads the repeat table and replaces the score
 * tables and the estimator's own count rows by ones of QB_MAX_DEGREE + 1 rows (the first D + 1 table rows are the ones they replace, so the unmerged
 * call reads what it read before).  Not to be called while a call of the estimator is in flight.
 */
extern "C" int qldpc_qber_set_merge(qldpc_qber *est, int on)
{
    if (!est) return QLDPC_EINVAL;
    if (!on || est->d_rep) { est->merge = on != 0; return QLDPC_OK; }
    const qldpc_qber_cfg &cfg = est->cfg;
    const int M = est->M, D = est->D, R = QB_MAX_DEGREE + 1;
    std::vector<uint8_t> rep((size_t)D * (size_t)M);
    int rc = qldpc_qber_repeat_table_host(est->h_tab.data(), est->N, M, D, rep.data());
    if (rc) return rc;
    std::vector<int32_t> L1((size_t)R * (size_t)cfg.n_grid), L0(L1.size());
    if ((rc = qldpc_qber_table_host(QB_MAX_DEGREE, cfg.n_grid, cfg.q_lo, cfg.q_hi, L1.data(), L0.data(), nullptr, nullptr))) return rc;
    HIPCHK(hipSetDevice(cfg.device));
    const size_t tbytes = sizeof(int32_t) * L1.size();
    dm_ledger *m = &est->mem;
    int32_t *d_L1 = nullptr, *d_L0 = nullptr;
    uint32_t *d_counts = nullptr;
    unsigned long long *d_pool = nullptr;
    uint8_t *d_rep = nullptr;
    hipError_t he = hipSuccess;
    if (dm_alloc(m, &d_L1, L1.size()) || dm_alloc(m, &d_L0, L0.size()) || dm_alloc(m, &d_counts, (size_t)cfg.max_frames * 2 * (size_t)R) ||
        dm_alloc(m, &d_pool, 2 * (size_t)R) || dm_alloc(m, &d_rep, rep.size())) he = hipErrorOutOfMemory;
    if (he == hipSuccess) he = hipMemcpy(d_L1, L1.data(), tbytes, hipMemcpyHostToDevice);
    if (he == hipSuccess) he = hipMemcpy(d_L0, L0.data(), tbytes, hipMemcpyHostToDevice);
    if (he == hipSuccess) he = hipMemcpy(d_rep, rep.data(), rep.size(), hipMemcpyHostToDevice);
    const size_t staged_bytes = sizeof(uint32_t) * (2 * (size_t)R + 3 * (size_t)est->Wn);
    const int mstaged = staged_bytes <= QBER_LDS_MAX && !est->no_stage;
    const size_t mlds = mstaged ? staged_bytes : sizeof(uint32_t) * 2 * (size_t)R;
    if (he == hipSuccess && mlds > 48 * 1024)
        he = hipFuncSetAttribute((const void *)&qk_qber_count_merged<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)mlds);
    if (he == hipSuccess) he = hipDeviceSynchronize();      /* no call reads the rows that are freed below */
    if (he != hipSuccess) {
        dm_release(m, &d_L1); dm_release(m, &d_L0); dm_release(m, &d_counts); dm_release(m, &d_pool); dm_release(m, &d_rep);
        qldpc_set_error("qber_set_merge: %s", hipGetErrorString(he));
        return QLDPC_EHIP;
    }
    dm_release(m, &est->d_L1); dm_release(m, &est->d_L0); dm_release(m, &est->d_counts); dm_release(m, &est->d_pool);
    est->d_L1 = d_L1; est->d_L0 = d_L0; est->d_counts = d_counts; est->d_pool = d_pool; est->d_rep = d_rep;
    est->mstaged = mstaged; est->mlds_bytes = mlds;
    est->merge = 1;
    return QLDPC_OK;
}

extern "C" int qldpc_qber_grid(const qldpc_qber *est, float *q, float *llr)
{
    if (!est) return QLDPC_EINVAL;
    if (q) memcpy(q, est->h_q.data(), sizeof(float) * est->h_q.size());
    if (llr) memcpy(llr, est->h_llr.data(), sizeof(float) * est->h_llr.size());
    return est->cfg.n_grid;
}

extern "C" int qldpc_qber_estimate_dev(qldpc_qber *est, const uint32_t *d_bits, const uint8_t *d_vn_class, const int *d_n_channel, const uint32_t *d_synd_bits,
                                       const uint32_t *d_erase_bits, const uint32_t *d_known_bits, const uint32_t *d_value_bits, int n_frames,
                                       uint32_t *d_counts, int *d_index, float *d_qber, float *d_llr_mag, uint64_t *d_pool_counts, int *d_pool_index)
{
    if (!est || !d_bits || n_frames < 1 || (d_known_bits && !d_value_bits)) return QLDPC_EINVAL;
    if (n_frames > est->cfg.max_frames) { qldpc_set_error("qber_estimate: %d frames, the estimator was made for %d", n_frames, est->cfg.max_frames); return QLDPC_EINVAL; }
    HIPCHK(hipSetDevice(est->cfg.device));
    hipStream_t s = est->stream;
    const int M = est->M, Wn = est->Wn;
    const int bins = est->merge ? 2 * (QB_MAX_DEGREE + 1) : est->bins, Dsc = bins / 2 - 1;      /* count rows in use, and the score's largest degree */
    const bool want_index = d_index || d_qber || d_llr_mag, want_pool = d_pool_counts || d_pool_index;
    if (!d_counts && !want_index && !want_pool) return QLDPC_OK;
    uint32_t *counts = d_counts ? d_counts : est->d_counts;
    unsigned long long *pool = want_pool ? (d_pool_counts ? reinterpret_cast<unsigned long long *>(d_pool_counts) : est->d_pool) : nullptr;
    HIPCHK(hipMemsetAsync(counts, 0, sizeof(uint32_t) * (size_t)n_frames * (size_t)bins, s));
    if (pool) HIPCHK(hipMemsetAsync(pool, 0, sizeof(unsigned long long) * (size_t)bins, s));
    qbk_frame_rows in = {d_bits, d_erase_bits, d_known_bits, d_value_bits, d_synd_bits, d_n_channel, nullptr};
    if (d_vn_class) {
        hipLaunchKernelGGL(qk_qber_class_rows, dim3((unsigned)((Wn + QBK_THREADS - 1) / QBK_THREADS)), dim3(QBK_THREADS), 0, s, d_vn_class, est->d_cls_rows, est->N, Wn);
        LAUNCHCHK();
        in.cls_rows = est->d_cls_rows;
    }
    /* checks per workgroup: as given, else as few chunks per frame as still give every CU about eight workgroups -- a chunk stages the whole frame */
    int cpb = est->cpb;
    if (!cpb) {
        const int passes = (M + QBK_THREADS - 1) / QBK_THREADS;
        const int chunks = std::max(1, std::min(passes, (8 * est->cus + n_frames - 1) / n_frames));
        cpb = (passes + chunks - 1) / chunks * QBK_THREADS;
    }
    const dim3 grid((unsigned)((M + cpb - 1) / cpb), (unsigned)n_frames);
    if (est->merge && est->mstaged)
        hipLaunchKernelGGL(qk_qber_count_merged<true>, grid, dim3(QBK_THREADS), est->mlds_bytes, s, in, est->d_tab, est->d_rep, est->N, M, est->D, Wn, est->Wm, cpb, counts, pool);
    else if (est->merge)
        hipLaunchKernelGGL(qk_qber_count_merged<false>, grid, dim3(QBK_THREADS), est->mlds_bytes, s, in, est->d_tab, est->d_rep, est->N, M, est->D, Wn, est->Wm, cpb, counts, pool);
    else if (est->staged)
        hipLaunchKernelGGL(qk_qber_count<true>, grid, dim3(QBK_THREADS), est->lds_bytes, s, in, est->d_tab, est->N, M, est->D, Wn, est->Wm, cpb, counts, pool);
    else
        hipLaunchKernelGGL(qk_qber_count<false>, grid, dim3(QBK_THREADS), est->lds_bytes, s, in, est->d_tab, est->N, M, est->D, Wn, est->Wm, cpb, counts, pool);
    LAUNCHCHK();
    if (want_index || d_pool_index) {
        /* without per-frame outputs only the pool's workgroup runs: it is block n_frames of a launch of n_frames + 1, so the frames' blocks are kept and write nothing */
        const unsigned blocks = (unsigned)n_frames + (d_pool_index ? 1u : 0u);
        hipLaunchKernelGGL(qk_qber_argmax, dim3(blocks), dim3(QBK_THREADS), 0, s, counts, pool, Dsc, est->cfg.n_grid, est->d_L1, est->d_L0, est->d_q, est->d_llr, n_frames,
                           d_index, d_qber, d_llr_mag, d_pool_index);
        LAUNCHCHK();
    }
    return QLDPC_OK;
}
