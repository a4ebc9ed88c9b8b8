/*
 * qldpc_kernels_recon_tag.h -- the kernels of the keyed tag inside a reconciliation session (qldpc_recon_decode_blocks_tagged, _decode_guess_tagged,
 * qldpc_recon_tag_blocks, qldpc_recon_verify_tag_dev).  The rule is stated in qldpc_recon_tag_core.h; these lanes and the host mirror call the same
 * functions.  Included by qldpc_recon.hip after rk_block_crc.  One workgroup of RK_LANES per block, R = the keys per block as a template argument so
 * that the R accumulators of a lane stay in registers.  No atomics: every output word has one writer.
 *
 * rk_verify_tag<R>: rk_verify with the tag fused in.  The decoded row is read once: a masked word feeds the CRC step, the flip count, the copy to
 *     res_keys and R Horner accumulators.  The partials fold in the CRC's tree, LDS holding one 64-bit value per lane and key (8 KB at R = 4) beside
 *     the CRC's table and registers.  Verdict and result columns are rk_verify's; a block that is not ok && crc == want keeps its original words and
 *     gets 2 R zero tag words, so that nothing is disclosed for a failed block.
 * rk_tag<R>: tags alone over compact key rows [n][Wk], the same lanes; a row whose `skip` entry is not 0 gets zeros (the status column of a result
 *     block is such a column: QLDPC_OK = 0 = tagged).
 */
#ifndef QLDPC_KERNELS_RECON_TAG_H
#define QLDPC_KERNELS_RECON_TAG_H

#include "qldpc_recon_tag_core.h"

/* the R field elements of block b's hash-key row (stride 0: every block reads row 0) */
template <int R>
__device__ static inline void rt_load_keys(const uint32_t *__restrict__ hash_keys, size_t hash_key_stride, int b, uint64_t (&k)[R])
{
    const uint32_t *hk = hash_keys + (size_t)b * hash_key_stride;
#pragma unroll
    for (int q = 0; q < R; q++) k[q] = ph_key(hk[2 * q], hk[2 * q + 1]);
}

/* the fold of the lanes' partials s_part[q][lane] and the close: every lane returns with tag[q] of the whole block */
template <int R>
__device__ static inline void rt_fold_block(uint64_t (*s_part)[RK_LANES], const uint64_t (&k)[R], int c, int n_bits, uint64_t (&tag)[R])
{
    const int t = (int)threadIdx.x;
    uint64_t X[R];
#pragma unroll
    for (int q = 0; q < R; q++) X[q] = rt_chunk_pow(k[q], c);
    for (int s = 1; s < RK_LANES; s <<= 1) {
        if ((t & (2 * s - 1)) == 0) {
#pragma unroll
            for (int q = 0; q < R; q++) s_part[q][t] = rt_fold(s_part[q][t], X[q], s_part[q][t + s]);
        }
#pragma unroll
        for (int q = 0; q < R; q++) X[q] = ph_mul(X[q], X[q]);
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < R; q++) tag[q] = rt_close(s_part[q][0], k[q], n_bits);
}

template <int R>
static __global__ __launch_bounds__(RK_LANES) void rk_verify_tag(const uint32_t *__restrict__ out, const uint32_t *__restrict__ key, const int *__restrict__ key_bits,
                                                                 const uint32_t *__restrict__ crc_want, const int *__restrict__ ok, const int *__restrict__ iters,
                                                                 const uint32_t *__restrict__ hash_keys, size_t hash_key_stride, uint32_t *__restrict__ res_keys,
                                                                 int *__restrict__ res, uint32_t *__restrict__ tags, int n, int Wk, int Wn)
{
    __shared__ uint32_t s_tab[256], s_reg[RK_LANES];
    __shared__ int s_cnt[RK_LANES];
    __shared__ uint64_t s_part[R][RK_LANES];
    const int b = (int)blockIdx.x, t = (int)threadIdx.x;
    const int kb = rt_key_bits(key_bits[b], Wk), nw = (kb + 31) / 32;
    const uint32_t *words = out + (size_t)b * Wn, *old = key + (size_t)b * Wk;
    uint32_t *dst = res_keys + (size_t)b * Wk;
    uint64_t k[R], h[R];
    rt_load_keys<R>(hash_keys, hash_key_stride, b, k);
#pragma unroll
    for (int q = 0; q < R; q++) h[q] = 0;
    s_tab[t] = crc_table_entry((uint32_t)t);
    __syncthreads();
    int pad;
    const int c = crc_chunk_words(nw, RK_LANES, &pad);
    uint32_t reg = 0;
    int flips = 0;
    for (int v = t * c; v < (t + 1) * c; v++) {
        const int i = v - pad;
        if (i < 0) continue;
        const uint32_t m = tail_mask(i, nw, kb);
        const uint32_t x = words[i] & m;
        reg = crc_word_step(reg, x, s_tab);
        flips += __popc((old[i] & m) ^ x);
        dst[i] = x;
#pragma unroll
        for (int q = 0; q < R; q++) h[q] = rt_step(h[q], k[q], x);
    }
    s_reg[t] = reg;
    s_cnt[t] = flips;
#pragma unroll
    for (int q = 0; q < R; q++) s_part[q][t] = h[q];
    __syncthreads();
    uint32_t X = gf_xpow(32ull * (unsigned long long)c);
    for (int s = 1; s < RK_LANES; s <<= 1) {
        if ((t & (2 * s - 1)) == 0) {
            s_reg[t] = gf_mulmod(s_reg[t], X) ^ s_reg[t + s];
            s_cnt[t] += s_cnt[t + s];
        }
        X = gf_mulmod(X, X);
        __syncthreads();
    }
    const uint32_t crc = crc_close(s_reg[0], nw);
    uint64_t tag[R];
    rt_fold_block<R>(s_part, k, c, kb, tag);
    const bool good = ok[b] && crc == crc_want[b];
    if (!good)      /* uniform per workgroup */
        for (int i = t; i < nw; i += RK_LANES) dst[i] = old[i];
    if (t == 0) {
        res[b] = good ? QLDPC_OK : QLDPC_EDECODE;
        res[n + b] = good ? s_cnt[0] : 0;
        res[2 * n + b] = iters[b];
        res[3 * n + b] = (int)crc;
#pragma unroll
        for (int q = 0; q < R; q++) ph_store_tag(tags + (size_t)b * 2 * R + 2 * q, good ? tag[q] : 0ull);
    }
}

template <int R>
static __global__ __launch_bounds__(RK_LANES) void rk_tag(const uint32_t *__restrict__ keys, const int *__restrict__ key_bits, const int *__restrict__ skip,
                                                          const uint32_t *__restrict__ hash_keys, size_t hash_key_stride, uint32_t *__restrict__ tags, int Wk)
{
    __shared__ uint64_t s_part[R][RK_LANES];
    const int b = (int)blockIdx.x, t = (int)threadIdx.x;
    if (skip && skip[b] != 0) {      /* uniform per workgroup */
        if (t < 2 * R) tags[(size_t)b * 2 * R + t] = 0u;
        return;
    }
    const int kb = rt_key_bits(key_bits[b], Wk), nw = (kb + 31) / 32;
    const uint32_t *words = keys + (size_t)b * Wk;
    uint64_t k[R], h[R];
    rt_load_keys<R>(hash_keys, hash_key_stride, b, k);
#pragma unroll
    for (int q = 0; q < R; q++) h[q] = 0;
    int pad;
    const int c = crc_chunk_words(nw, RK_LANES, &pad);
    for (int v = t * c; v < (t + 1) * c; v++) {
        const int i = v - pad;
        if (i < 0) continue;
        const uint32_t x = words[i] & tail_mask(i, nw, kb);
#pragma unroll
        for (int q = 0; q < R; q++) h[q] = rt_step(h[q], k[q], x);
    }
#pragma unroll
    for (int q = 0; q < R; q++) s_part[q][t] = h[q];
    __syncthreads();
    uint64_t tag[R];
    rt_fold_block<R>(s_part, k, c, kb, tag);
    if (t == 0) {
#pragma unroll
        for (int q = 0; q < R; q++) ph_store_tag(tags + (size_t)b * 2 * R + 2 * q, tag[q]);
    }
}

/* the launches, R chosen at run time (1 .. RT_MAX_KEYS: checked by the callers) */
static void rk_verify_tag_launch(int R, int n, hipStream_t s, const uint32_t *out, const uint32_t *key, const int *key_bits, const uint32_t *crc_want, const int *ok,
                                 const int *iters, const uint32_t *hash_keys, size_t hash_key_stride, uint32_t *res_keys, int *res, uint32_t *tags, int Wk, int Wn)
{
#define RT_VERIFY(r) hipLaunchKernelGGL(rk_verify_tag<r>, dim3((unsigned)n), dim3(RK_LANES), 0, s, out, key, key_bits, crc_want, ok, iters, hash_keys, hash_key_stride, res_keys, res, tags, n, Wk, Wn)
    switch (R) {
    case 1: RT_VERIFY(1); break;
    case 2: RT_VERIFY(2); break;
    case 3: RT_VERIFY(3); break;
    default: RT_VERIFY(4); break;
    }
#undef RT_VERIFY
}

static void rk_tag_launch(int R, int n, hipStream_t s, const uint32_t *keys, const int *key_bits, const int *skip, const uint32_t *hash_keys, size_t hash_key_stride,
                          uint32_t *tags, int Wk)
{
#define RT_TAG(r) hipLaunchKernelGGL(rk_tag<r>, dim3((unsigned)n), dim3(RK_LANES), 0, s, keys, key_bits, skip, hash_keys, hash_key_stride, tags, Wk)
    switch (R) {
    case 1: RT_TAG(1); break;
    case 2: RT_TAG(2); break;
    case 3: RT_TAG(3); break;
    default: RT_TAG(4); break;
    }
#undef RT_TAG
}

#endif /* QLDPC_KERNELS_RECON_TAG_H */
