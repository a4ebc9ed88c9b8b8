/*
 * qldpc_polar_list.hip -- the context and the launches of qldpc_polar_list_*: the batched CRC-aided SC list decoder.  The rules are
 * qldpc_polar_list_core.h's, the kernels and the layout of the scratch qldpc_kernels_polar_list.h's, the host mirror qldpc_polar_list_host.c's.
 *
 * A context owns everything a call touches: the frozen mask and info_pos on the device, the belief and bit levels of ceil(max_frames / 64) groups,
 * the L root rows of every frame and their encodings, the metrics and the remainders.  A call allocates nothing and waits for nothing: its kernels
 * (load, decode, roots, encode, CRC, outputs) go onto the context's stream in order.
 */
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "qldpc_hip.h"
#include "qldpc_kernels_polar_list.h"

struct qldpc_polar_list {
    int n, n_info, messages, maxq, L, P, crc_len, max_frames, device;
    uint32_t crc_poly;
    size_t groups, W;
    hipStream_t stream;
    uint32_t *d_fmask;             /* W words: 1 = frozen */
    int *d_info_pos;
    void *d_A;                     /* groups x pll_group_quads(n, L) x 64 quads of int8 or float */
    uint32_t *d_Bt;                /* groups x pll_bit_words(L, n) x 64 */
    uint32_t *d_LX, *d_LU;         /* max_frames x L x W each: the paths' root words and decisions */
    uint32_t *d_M, *d_rem;         /* max_frames x L each: the metrics (uint32 or float) and the remainders */
    size_t dev_bytes;
};

extern "C" void qldpc_polar_list_free(qldpc_polar_list *p)
{
    if (!p) return;
    (void)hipSetDevice(p->device);
    (void)hipStreamSynchronize(p->stream);                       /* the last call may still read the scratch */
    void *all[] = {p->d_fmask, p->d_info_pos, p->d_A, p->d_Bt, p->d_LX, p->d_LU, p->d_M, p->d_rem};
    for (void *q : all)
        if (q) (void)hipFree(q);
    delete p;
}

extern "C" int qldpc_polar_list_create(int log2_n, int n_info, const int *info_pos, int messages, int maxq, int list_size, int crc_len, uint32_t crc_poly,
                                       int max_frames, int device, qldpc_polar_list **out)
{
    if (!out) return QLDPC_EINVAL;
    *out = nullptr;
    /* every argument check before the first HIP call */
    if (pll_check_size(log2_n)) { qldpc_set_error("polar_list_create: log2_n=%d (1 .. %d: the scratch grows with list_size x N)", log2_n, PLL_MAX_LOG2N); return QLDPC_ESIZE; }
    if (messages != QLDPC_POLAR_I8 && messages != QLDPC_POLAR_F32) { qldpc_set_error("polar_list_create: messages=%d (QLDPC_POLAR_I8 or QLDPC_POLAR_F32)", messages); return QLDPC_EINVAL; }
    if (pl_check_maxq(messages, maxq)) { qldpc_set_error("polar_list_create: maxq=%d (1 .. %d: f gives maxq + 1, which has to fit an int8)", maxq, PL_MAX_MAXQ); return QLDPC_ESIZE; }
    if (pll_check_list(list_size)) { qldpc_set_error("polar_list_create: list_size=%d (1, 2, 4 or 8)", list_size); return QLDPC_ESIZE; }
    if (max_frames < 1 || max_frames > (1 << 24)) { qldpc_set_error("polar_list_create: max_frames=%d (1 .. %d)", max_frames, 1 << 24); return QLDPC_EINVAL; }
    const size_t W = (size_t)pl_words(log2_n);
    std::vector<uint32_t> mask(W, 0u);
    const int bad = pl_mark_info(log2_n, n_info, info_pos, mask.data());
    if (bad) {
        if (bad == PL_EINVAL) qldpc_set_error("polar_list_create: info_pos names a position twice (positions must be distinct)");
        else qldpc_set_error("polar_list_create: n_info=%d positions, each in 0 .. N - 1, are required (0 <= n_info <= N = %ld)", n_info, 1l << log2_n);
        return bad;
    }
    if (pll_check_crc(crc_len, crc_poly, n_info)) {
        qldpc_set_error("polar_list_create: crc_len=%d, crc_poly=0x%x, n_info=%d (crc_len 0 .. 32 and at most n_info; crc_poly holds the low crc_len coefficients, x^crc_len is implied)",
                        crc_len, (unsigned)crc_poly, n_info);
        return QLDPC_ESIZE;
    }
    const uint32_t valid = pl_row_mask(log2_n);
    for (size_t w = 0; w < W; w++) mask[w] = ~mask[w] & valid;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { qldpc_set_error("no HIP device visible: libqldpc has no CPU fallback"); return QLDPC_ENODEV; }
    if (device < 0 || device >= ndev) { qldpc_set_error("device %d out of range", device); return QLDPC_ENODEV; }
    HIPCHK(hipSetDevice(device));
    qldpc_polar_list *p = new (std::nothrow) qldpc_polar_list();
    if (!p) return QLDPC_ENOMEM;
    p->n = log2_n; p->n_info = n_info; p->messages = messages; p->maxq = maxq; p->L = list_size; p->crc_len = crc_len; p->crc_poly = crc_poly;
    p->P = pll_final_paths(list_size, n_info);
    p->max_frames = max_frames; p->device = device;
    p->W = W; p->groups = ((size_t)max_frames + PL_GROUP - 1) / PL_GROUP;
    const size_t esz = messages == QLDPC_POLAR_I8 ? 1 : sizeof(float), L = (size_t)list_size;
    const size_t bytes_A = 4 * esz * p->groups * pll_group_quads(log2_n, list_size) * PL_GROUP, bytes_B = sizeof(uint32_t) * p->groups * pll_bit_words(list_size, log2_n) * PL_GROUP,
                 bytes_rows = sizeof(uint32_t) * (size_t)max_frames * L * W;
    int rc = QLDPC_OK;
    auto alloc = [&](void **q, size_t bytes) {
        if (!bytes || rc) return;
        if (hipMalloc(q, bytes) != hipSuccess) { (void)hipGetLastError(); rc = QLDPC_ENOMEM; } else p->dev_bytes += bytes;
    };
    alloc((void **)&p->d_fmask, sizeof(uint32_t) * W);
    alloc((void **)&p->d_info_pos, sizeof(int) * (size_t)(n_info > 0 ? n_info : 1));
    alloc(&p->d_A, bytes_A);
    alloc((void **)&p->d_Bt, bytes_B);
    alloc((void **)&p->d_LX, bytes_rows);
    alloc((void **)&p->d_LU, bytes_rows);
    alloc((void **)&p->d_M, sizeof(uint32_t) * (size_t)max_frames * L);
    alloc((void **)&p->d_rem, sizeof(uint32_t) * (size_t)max_frames * L);
    if (rc) {
        qldpc_set_error("polar_list_create: device allocation failed (about %zu MiB for max_frames=%d, list_size=%d at N = 2^%d: lower max_frames)",
                        (bytes_A + bytes_B + 2 * bytes_rows) >> 20, max_frames, list_size, log2_n);
        qldpc_polar_list_free(p);
        return rc;
    }
    hipError_t he = hipMemcpy(p->d_fmask, mask.data(), sizeof(uint32_t) * W, hipMemcpyHostToDevice);
    if (he == hipSuccess && n_info > 0) he = hipMemcpy(p->d_info_pos, info_pos, sizeof(int) * (size_t)n_info, hipMemcpyHostToDevice);
    if (he != hipSuccess) { qldpc_set_error("polar_list_create: %s", hipGetErrorString(he)); qldpc_polar_list_free(p); return QLDPC_EHIP; }
    *out = p;
    return QLDPC_OK;
}

extern "C" size_t qldpc_polar_list_device_bytes(const qldpc_polar_list *p) { return p ? p->dev_bytes : 0; }

extern "C" int qldpc_polar_list_set_stream(qldpc_polar_list *p, void *hip_stream)
{
    if (!p) return QLDPC_EINVAL;
    p->stream = (hipStream_t)hip_stream;
    return QLDPC_OK;
}

template <class M, int L>
static void pll_launch_decode(const qldpc_polar_list *p, M m, int n_frames, unsigned groups, const uint32_t *d_frozen_u)
{
    typedef typename M::mem mem;
    typedef typename pll_metric<M>::type met;
    hipLaunchKernelGGL((pll_decode<M, L>), dim3(groups), dim3(PL_GROUP), 0, p->stream, m, p->n, n_frames, (const uint32_t *)p->d_fmask, d_frozen_u, (mem *)p->d_A,
                       p->d_Bt, (met *)p->d_M);
}

template <class M>
static int pll_run_decode(const qldpc_polar_list *p, M m, int n_frames, const void *d_llr, const uint32_t *d_frozen_u)
{
    typedef typename M::mem mem;
    const unsigned groups = (unsigned)(((size_t)n_frames + PL_GROUP - 1) / PL_GROUP);
    const size_t threads = (size_t)groups * pll_quads(p->n) * PL_GROUP;
    hipLaunchKernelGGL(pll_load<M>, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, p->stream, m, p->n, p->L, n_frames, (const mem *)d_llr, (mem *)p->d_A);
    LAUNCHCHK();
    switch (p->L) {
    case 1: pll_launch_decode<M, 1>(p, m, n_frames, groups, d_frozen_u); break;
    case 2: pll_launch_decode<M, 2>(p, m, n_frames, groups, d_frozen_u); break;
    case 4: pll_launch_decode<M, 4>(p, m, n_frames, groups, d_frozen_u); break;
    default: pll_launch_decode<M, 8>(p, m, n_frames, groups, d_frozen_u); break;
    }
    LAUNCHCHK();
    return QLDPC_OK;
}

extern "C" int qldpc_polar_list_decode_dev(qldpc_polar_list *p, int n_frames, const void *d_llr, const uint32_t *d_frozen_u, const uint32_t *d_crc, uint32_t *d_u,
                                           uint32_t *d_info, uint32_t *d_x, int32_t *d_pick, void *d_metric, uint32_t *d_list_x)
{
    if (!p) return QLDPC_EINVAL;
    if (n_frames < 0) { qldpc_set_error("polar_list_decode_dev: n_frames=%d is negative", n_frames); return QLDPC_EINVAL; }
    if (n_frames > p->max_frames) {
        qldpc_set_error("polar_list_decode_dev: n_frames=%d exceeds the context's max_frames=%d: create it larger or split the call", n_frames, p->max_frames);
        return QLDPC_ESIZE;
    }
    if (d_crc && p->crc_len == 0) { qldpc_set_error("polar_list_decode_dev: a crc row with crc_len = 0"); return QLDPC_EINVAL; }
    if (n_frames == 0) return QLDPC_OK;
    if (!d_llr) { qldpc_set_error("polar_list_decode_dev: d_llr is NULL"); return QLDPC_EINVAL; }
    HIPCHK(hipSetDevice(p->device));
    int rc;
    if (p->messages == QLDPC_POLAR_I8) rc = pll_run_decode(p, pl_msg_i8{p->maxq}, n_frames, d_llr, d_frozen_u);
    else rc = pll_run_decode(p, pl_msg_f32{}, n_frames, d_llr, d_frozen_u);
    if (rc) return rc;
    if (!(d_u || d_info || d_x || d_pick || d_metric || d_list_x)) return QLDPC_OK;
    const size_t groups = ((size_t)n_frames + PL_GROUP - 1) / PL_GROUP, L = (size_t)p->L, rows = (size_t)n_frames * L;
    size_t threads = groups * L * p->W * PL_GROUP;
    hipLaunchKernelGGL(pll_roots, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, p->stream, p->n, p->L, p->P, n_frames, (const uint32_t *)p->d_Bt, p->d_LX);
    LAUNCHCHK();
    /* u = encode(x) of every path's root word */
    const size_t tiles = p->W > PL_ENC_TILE ? p->W / PL_ENC_TILE : 1;
    hipLaunchKernelGGL(pl_encode_tiles, dim3((unsigned)(rows * tiles)), dim3(PL_ENC_LANES), 0, p->stream, p->n, (const uint32_t *)p->d_LX, p->d_LU);
    LAUNCHCHK();
    if (tiles > 1) {
        hipLaunchKernelGGL(pl_encode_columns, dim3((unsigned)(rows * PL_ENC_TILE / PL_ENC_LANES)), dim3(PL_ENC_LANES), 0, p->stream, p->n, (int)rows, p->d_LU);
        LAUNCHCHK();
    }
    hipLaunchKernelGGL(pll_crc, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, p->stream, p->n, p->L, p->P, n_frames, p->n_info, (const int *)p->d_info_pos, p->crc_len,
                       p->crc_poly, (const uint32_t *)p->d_LU, p->d_rem);
    LAUNCHCHK();
    threads = (size_t)n_frames * p->W;
    hipLaunchKernelGGL(pll_outputs, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, p->stream, p->n, p->L, p->P, n_frames, p->n_info, (const int *)p->d_info_pos,
                       (const uint32_t *)p->d_rem, d_crc, (const uint32_t *)p->d_LU, (const uint32_t *)p->d_LX, (const uint32_t *)p->d_M, d_u, d_info, d_x, d_pick,
                       (uint32_t *)d_metric, d_list_x);
    LAUNCHCHK();
    return QLDPC_OK;
}
