/*
 * qldpc_polar_list.hip -- the context and the launches of qldpc_polar_list_*: the batched CRC-aided SC list decoder.  The rules are
 * qldpc_polar_list_core.h's, the kernels and the layout of the scratch qldpc_kernels_polar_list.h's, the host mirror qldpc_polar_list_host.c's,
 * and what a context shares with the SC decoder's qldpc_polar_ctx.h's.
 *
 * A context owns everything a call touches: the frozen mask and info_pos on the device, the belief and bit levels of ceil(max_frames / 64) groups,
 * the L root rows of every frame and their encodings, the metrics and the remainders.  A call allocates nothing and waits for nothing: its kernels
 * (load, decode, roots, encode, CRC, outputs) go onto the context's stream in order.
 */
#include <hip/hip_runtime.h>

#include <cstdint>
#include <new>

#include "qldpc_kernels_polar_list.h"
#include "qldpc_polar_ctx.h"

struct qldpc_polar_list {
    pl_ctx c;
    int L, P, crc_len;
    uint32_t crc_poly;
    void *d_A;                     /* groups x pll_group_quads(n, L) x 64 quads of int8 or float */
    uint32_t *d_Bt;                /* groups x pll_bit_words(L, n) x 64 */
    uint32_t *d_LX, *d_LU;         /* max_frames x L x W each: the paths' root words and decisions */
    uint32_t *d_M, *d_rem;         /* max_frames x L each: the metrics (uint32 or float) and the remainders */
};

const pl_ctx *pl_ctx_of_list(const qldpc_polar_list *p, int *crc_len, uint32_t *crc_poly)
{
    *crc_len = p->crc_len; *crc_poly = p->crc_poly;
    return &p->c;
}

extern "C" void qldpc_polar_list_free(qldpc_polar_list *p)
{
    if (!p) return;
    pl_ctx_free(&p->c);
    delete p;
}

extern "C" int qldpc_polar_list_create(int log2_n, int n_info, const int *info_pos, int messages, int maxq, int list_size, int crc_len, uint32_t crc_poly,
                                       int max_frames, int device, qldpc_polar_list **out)
{
    if (!out) return QLDPC_EINVAL;
    *out = nullptr;
    qldpc_polar_list *p = new (std::nothrow) qldpc_polar_list();
    if (!p) return QLDPC_ENOMEM;
    const int rc = pl_ctx_create(&p->c, "polar_list_create", log2_n, PLL_MAX_LOG2N, n_info, info_pos, messages, maxq, max_frames, device, [&](int after_mask) {
        if (!after_mask && pll_check_list(list_size)) { qldpc_set_error("polar_list_create: list_size=%d (1, 2, 4 or 8)", list_size); return QLDPC_ESIZE; }
        if (after_mask && pll_check_crc(crc_len, crc_poly, n_info)) {
            qldpc_set_error("polar_list_create: crc_len=%d, crc_poly=0x%x, n_info=%d (crc_len 0 .. 32 and at most n_info; crc_poly holds the low crc_len coefficients, x^crc_len is implied)",
                            crc_len, (unsigned)crc_poly, n_info);
            return QLDPC_ESIZE;
        }
        return QLDPC_OK;
    });
    if (rc) { qldpc_polar_list_free(p); return rc; }
    p->L = list_size; p->crc_len = crc_len; p->crc_poly = crc_poly;
    p->P = pll_final_paths(list_size, n_info);
    const size_t esz = messages == QLDPC_POLAR_I8 ? 1 : sizeof(float), L = (size_t)list_size, groups = p->c.groups;
    const size_t bytes_A = 4 * esz * groups * pll_group_quads(log2_n, list_size) * PL_GROUP, bytes_B = sizeof(uint32_t) * groups * pll_bit_words(list_size, log2_n) * PL_GROUP,
                 bytes_rows = sizeof(uint32_t) * (size_t)max_frames * L * p->c.W;
    pl_ctx_alloc(&p->c, &p->d_A, bytes_A);
    pl_ctx_alloc(&p->c, &p->d_Bt, bytes_B);
    pl_ctx_alloc(&p->c, &p->d_LX, bytes_rows);
    pl_ctx_alloc(&p->c, &p->d_LU, bytes_rows);
    pl_ctx_alloc(&p->c, &p->d_M, sizeof(uint32_t) * (size_t)max_frames * L);
    pl_ctx_alloc(&p->c, &p->d_rem, sizeof(uint32_t) * (size_t)max_frames * L);
    if (p->c.alloc_failed) {
        qldpc_set_error("polar_list_create: device allocation failed (about %zu MiB for max_frames=%d, list_size=%d at N = 2^%d: lower max_frames)",
                        (bytes_A + bytes_B + 2 * bytes_rows) >> 20, max_frames, list_size, log2_n);
        qldpc_polar_list_free(p);
        return QLDPC_ENOMEM;
    }
    *out = p;
    return QLDPC_OK;
}

extern "C" size_t qldpc_polar_list_device_bytes(const qldpc_polar_list *p) { return pl_ctx_device_bytes(PL_CTX(p)); }

extern "C" int qldpc_polar_list_set_stream(qldpc_polar_list *p, void *hip_stream) { return pl_ctx_set_stream(PL_CTX(p), hip_stream); }

template <class M, int L>
static void pll_launch_decode(const qldpc_polar_list *p, M m, int n_frames, unsigned groups, const uint32_t *d_frozen_u)
{
    typedef typename M::mem mem;
    typedef typename pll_metric<M>::type met;
    hipLaunchKernelGGL((pll_decode<M, L>), dim3(groups), dim3(PL_GROUP), 0, p->c.stream, m, p->c.n, n_frames, (const uint32_t *)p->c.d_fmask, d_frozen_u, (mem *)p->d_A,
                       p->d_Bt, (met *)p->d_M);
}

template <class M>
static int pll_run_decode(const qldpc_polar_list *p, M m, int n_frames, const void *d_llr, const uint32_t *d_frozen_u)
{
    typedef typename M::mem mem;
    const unsigned groups = (unsigned)(((size_t)n_frames + PL_GROUP - 1) / PL_GROUP);
    const size_t threads = (size_t)groups * pll_quads(p->c.n) * PL_GROUP;
    hipLaunchKernelGGL(pll_load<M>, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, p->c.stream, m, p->c.n, p->L, n_frames, (const mem *)d_llr, (mem *)p->d_A);
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
    int rc = pl_ctx_check_frames(PL_CTX(p), n_frames, "polar_list_decode_dev");
    if (rc) return rc;
    if (d_crc && p->crc_len == 0) { qldpc_set_error("polar_list_decode_dev: a crc row with crc_len = 0"); return QLDPC_EINVAL; }
    if (n_frames == 0) return QLDPC_OK;
    if (!d_llr) { qldpc_set_error("polar_list_decode_dev: d_llr is NULL"); return QLDPC_EINVAL; }
    const pl_ctx *c = &p->c;
    HIPCHK(hipSetDevice(c->device));
    rc = pl_with_messages(c, [&](auto m) { return pll_run_decode(p, m, n_frames, d_llr, d_frozen_u); });
    if (rc) return rc;
    if (!(d_u || d_info || d_x || d_pick || d_metric || d_list_x)) return QLDPC_OK;
    const size_t groups = ((size_t)n_frames + PL_GROUP - 1) / PL_GROUP, L = (size_t)p->L, rows = (size_t)n_frames * L;
    size_t threads = groups * L * c->W * PL_GROUP;
    hipLaunchKernelGGL(pll_roots, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, c->stream, c->n, p->L, p->P, n_frames, (const uint32_t *)p->d_Bt, p->d_LX);
    LAUNCHCHK();
    rc = pl_launch_encode(c->stream, c->n, rows, p->d_LX, p->d_LU);      /* u = encode(x) of every path's root word */
    if (rc) return rc;
    hipLaunchKernelGGL(pll_crc, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, c->stream, c->n, p->L, p->P, n_frames, c->n_info, (const int *)c->d_info_pos, p->crc_len,
                       p->crc_poly, (const uint32_t *)p->d_LU, p->d_rem);
    LAUNCHCHK();
    threads = (size_t)n_frames * c->W;
    hipLaunchKernelGGL(pll_outputs, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, c->stream, c->n, p->L, p->P, n_frames, c->n_info, (const int *)c->d_info_pos,
                       (const uint32_t *)p->d_rem, d_crc, (const uint32_t *)p->d_LU, (const uint32_t *)p->d_LX, (const uint32_t *)p->d_M, d_u, d_info, d_x, d_pick,
                       (uint32_t *)d_metric, d_list_x);
    LAUNCHCHK();
    return QLDPC_OK;
}
