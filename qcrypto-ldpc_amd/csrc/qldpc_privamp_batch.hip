/*
 * qldpc_privamp_batch.hip -- privacy amplification for a batch of blocks in one launch (qldpc_privamp_blocks*).
 *
 * The same hash as qldpc_privamp.hip (privAmp_doPrivAmp, subcomponents/priv_amp.c:213-218), bit for bit, by another route.  Let A be one
 * word step of the LFSR (32 bit steps of rnd_getPrngValue2_32, subcomponents/rnd.c:118-127) and R = A^numwords.  The word that meets key
 * word j in output bit i is A^(j+1) R^i seed, everything is linear over GF(2), so with <a, b> = parity(a & b)
 *
 *     out_i = XOR_j <key[j], A^(j+1) R^i seed> = <v_key, R^i seed>,       v_key = XOR_j (A^T)^(j+1) key[j]
 *
 * v_key is the Horner recurrence v <- A^T (v ^ key[j]) for j = numwords-1 .. 0, and A^T is 32 steps of the Galois form of the same LFSR
 * (x <- (x >> 1) ^ (x & 1 ? 0xe0000200 : 0)), 9 steps per word operation.  A block costs O(numwords + final_bits) word operations
 * instead of numwords x final_bits.
 *
 * pab_tables (one wave per distinct numwords of the call): R and R^(32 2^k) by square-and-multiply of 32 x 32 bit matrices, one column per
 *     lane.
 * pab_hash (grid = (chunks of 256 output words, blocks), 256 lanes): (a) every lane folds a contiguous chunk of key words, raises its
 *     partial by (A^T)^(chunk start) through the fixed table (A^T)^(2^k), the 256 partials are XOR-reduced (wave shuffles + one LDS
 *     exchange); (b) u_k = (R^T)^k v_key for k < 32 (32 ballots of one wave), then lane w jumps to x = R^(32 w) seed and its output word
 *     is bit k = <u_k, x>, MSB-first like qp_privamp.
 */
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>

#include "qldpc_hashbatch.h"
#include "qldpc_hip.h"

#define PAB_FEEDBACK 0xe0000200u
#define PAB_AT_LEVELS 19           /* chunk start < 2^24 / 32 words */
#define PAB_R_LEVELS 20            /* a block's table: level 0 = R (the u_k), level 1 + k = R^(32 2^k), k < 19: the jump to output word w < 2^19 */
#define PAB_LANES 256

/* forward LFSR, c <= 10 bit steps at once (as qldpc_privamp.hip): state = (state << 1) + parity(state & 0xe0000200) */
__host__ __device__ static inline uint32_t pab_fwd_chunk(uint32_t s, int c)
{
    const uint32_t nb = ((s >> (32 - c)) ^ (s >> (31 - c)) ^ (s >> (30 - c)) ^ (s >> (10 - c))) & ((1u << c) - 1u);
    return (s << c) | nb;
}
__host__ __device__ static inline uint32_t pab_a_step(uint32_t s)      /* A: one word of rnd_getPrngValue2_32 */
{
    s = pab_fwd_chunk(s, 10);
    s = pab_fwd_chunk(s, 10);
    s = pab_fwd_chunk(s, 10);
    return pab_fwd_chunk(s, 2);
}
/* transposed LFSR, c <= 9 bit steps at once: one step is x <- (x >> 1) ^ (x & 1 ? feedback : 0); the lowest tap (bit 9) needs 9 steps to
 * reach bit 0, so the c bits shifted out are the c low bits of x as it stands */
__host__ __device__ static inline uint32_t pab_t_chunk(uint32_t x, int c)
{
    const uint32_t low = x & ((1u << c) - 1u);
    return (x >> c) ^ (low << (32 - c)) ^ (low << (31 - c)) ^ (low << (30 - c)) ^ (low << (10 - c));
}
__host__ __device__ static inline uint32_t pab_at_step(uint32_t x)     /* A^T */
{
    x = pab_t_chunk(x, 9);
    x = pab_t_chunk(x, 9);
    x = pab_t_chunk(x, 9);
    return pab_t_chunk(x, 5);
}
/* a linear map of GF(2)^32 given by the images col[b] of the basis bits */
__host__ __device__ static inline uint32_t pab_apply(const uint32_t *col, uint32_t s)
{
    uint32_t r = 0;
#pragma unroll
    for (int b = 0; b < 32; b++) r ^= (0u - ((s >> b) & 1u)) & col[b];
    return r;
}
__host__ __device__ static inline uint32_t pab_parity(uint32_t x)
{
#ifdef __HIP_DEVICE_COMPILE__
    return (uint32_t)__popc(x) & 1u;
#else
    return (uint32_t)__builtin_parity(x);
#endif
}
__host__ __device__ static inline int pab_bits(uint32_t x)            /* number of table levels that reach x: smallest n with x < 2^n */
{
    int n = 0;
    while (x) { n++; x >>= 1; }
    return n;
}

/* one lane's part of the key fold: XOR_{j in [start, end)} (A^T)^(j+1) key[j], the last key word masked */
__host__ __device__ static inline uint32_t pab_fold_chunk(const uint32_t *key, int start, int end, int numwords, uint32_t tail_mask, const uint32_t *at_pow /* [levels][32] */)
{
    uint32_t v = 0;
    for (int j = end - 1; j >= start; j--) v = pab_at_step(v ^ (j == numwords - 1 ? key[j] & tail_mask : key[j]));
    for (int k = 0; (start >> k) != 0; k++)
        if ((start >> k) & 1) v = pab_apply(at_pow + 32 * k, v);
    return v;
}
/* output word w of a block: x = R^(32 w) seed, bit k (MSB-first) = <u[k], x> */
__host__ __device__ static inline uint32_t pab_out_word(uint32_t w, uint32_t seed, const uint32_t *u /* [32] */, const uint32_t *r_pow /* [levels][32] */)
{
    uint32_t x = seed;
    for (int k = 0; (w >> k) != 0; k++)
        if ((w >> k) & 1u) x = pab_apply(r_pow + 32 * (k + 1), x);
    uint32_t word = 0;
#pragma unroll
    for (int k = 0; k < 32; k++) word |= pab_parity(u[k] & x) << (31 - k);
    return word;
}

struct pab_desc {              /* one row per block, written by the host */
    uint32_t numwords, tail_mask, seed, final_bits;
    uint64_t key_off, out_off; /* in words from the key / output base of the call */
    uint32_t tab, pad;         /* which R table of the call */
};

/* R and R^(32 2^k) for every distinct numwords of the call: workgroup = one wave, lane b < 32 owns column b */
__global__ __launch_bounds__(64) void pab_tables(const uint32_t *__restrict__ tab_numwords, uint32_t *__restrict__ r_tabs)
{
    __shared__ uint32_t s_sq[32], s_acc[32];
    const int b = (int)threadIdx.x & 31;
    const bool own = threadIdx.x < 32;
    uint32_t e = tab_numwords[blockIdx.x];
    if (own) { s_sq[b] = pab_a_step(1u << b); s_acc[b] = 1u << b; }
    __syncthreads();
    while (e) {                                                 /* acc = A^numwords */
        if (e & 1u) {
            const uint32_t a = pab_apply(s_sq, s_acc[b]);
            __syncthreads();
            if (own) s_acc[b] = a;
        }
        const uint32_t q = pab_apply(s_sq, s_sq[b]);
        __syncthreads();
        if (own) s_sq[b] = q;
        __syncthreads();
        e >>= 1;
    }
    uint32_t *out = r_tabs + (size_t)blockIdx.x * (PAB_R_LEVELS * 32);
    for (int k = 0, lev = 0; lev < PAB_R_LEVELS; k++) {            /* s_acc = R^(2^k): kept for k = 0 and k >= 5 */
        if (own && (k == 0 || k >= 5)) out[32 * lev + b] = s_acc[b];
        if (k == 0 || k >= 5) lev++;
        const uint32_t q = pab_apply(s_acc, s_acc[b]);
        __syncthreads();
        if (own) s_acc[b] = q;
        __syncthreads();
    }
}

__global__ __launch_bounds__(PAB_LANES) void pab_hash(const pab_desc *__restrict__ descs, const uint32_t *__restrict__ keys, uint32_t *__restrict__ outs,
                                                      const uint32_t *__restrict__ at_pow, const uint32_t *__restrict__ r_tabs)
{
    __shared__ uint32_t s_at[PAB_AT_LEVELS * 32], s_r[PAB_R_LEVELS * 32], s_part[PAB_LANES / 64], s_u[32];
    const pab_desc d = descs[blockIdx.y];
    const uint32_t outwords = (d.final_bits + 31u) / 32u;
    const uint32_t w0 = blockIdx.x * PAB_LANES;
    if (w0 >= outwords) return;                                 /* the whole workgroup: the grid is as wide as the call's longest output */
    const int t = (int)threadIdx.x, numwords = (int)d.numwords;
    const int at_words = 32 * pab_bits((uint32_t)numwords - 1u), r_words = 32 * (1 + pab_bits(outwords - 1u));
    const uint32_t *r_pow = r_tabs + (size_t)d.tab * (PAB_R_LEVELS * 32);
    for (int i = t; i < at_words; i += PAB_LANES) s_at[i] = at_pow[i];
    for (int i = t; i < r_words; i += PAB_LANES) s_r[i] = r_pow[i];
    __syncthreads();

    /* (a) v_key */
    const uint32_t *key = keys + d.key_off;
    const int c = (numwords + PAB_LANES - 1) / PAB_LANES;
    const int start = min(t * c, numwords), end = min(start + c, numwords);
    uint32_t v = start < end ? pab_fold_chunk(key, start, end, numwords, d.tail_mask, s_at) : 0u;
#pragma unroll
    for (int o = 32; o; o >>= 1) v ^= __shfl_xor(v, o, 64);
    if ((t & 63) == 0) s_part[t >> 6] = v;
    __syncthreads();
    /* (b) u_k = (R^T)^k v_key: bit b of R^T u is <R e_b, u> */
    if (t < 64) {
        uint32_t u = s_part[0] ^ s_part[1] ^ s_part[2] ^ s_part[3];
        const uint32_t col = s_r[t & 31];
        for (int k = 0; k < 32; k++) {
            if (t == 0) s_u[k] = u;
            u = (uint32_t)__ballot(t < 32 && pab_parity(col & u));
        }
    }
    __syncthreads();
    const uint32_t w = w0 + (uint32_t)t;
    if (w >= outwords) return;
    uint32_t word = pab_out_word(w, d.seed, s_u, s_r);
    if (w == outwords - 1u) word &= hb_tail_mask((int)d.final_bits);
    outs[d.out_off + w] = word;
}

/* ------------------------------------------------------------------ host ---- */

static void pab_host_at_pow(uint32_t *at_pow /* [PAB_AT_LEVELS][32] */)
{
    for (int b = 0; b < 32; b++) at_pow[b] = pab_at_step(1u << b);
    for (int k = 1; k < PAB_AT_LEVELS; k++)
        for (int b = 0; b < 32; b++) at_pow[32 * k + b] = pab_apply(at_pow + 32 * (k - 1), at_pow[32 * (k - 1) + b]);
}
static void pab_host_r_pow(int numwords, int levels, uint32_t *r_pow /* [levels][32] */)
{
    uint32_t sq[32], acc[32], t[32];
    for (int b = 0; b < 32; b++) { sq[b] = pab_a_step(1u << b); acc[b] = 1u << b; }
    for (uint32_t e = (uint32_t)numwords; e; e >>= 1) {
        if (e & 1u) { for (int b = 0; b < 32; b++) t[b] = pab_apply(sq, acc[b]); memcpy(acc, t, sizeof(t)); }
        for (int b = 0; b < 32; b++) t[b] = pab_apply(sq, sq[b]);
        memcpy(sq, t, sizeof(t));
    }
    for (int k = 0, lev = 0; lev < levels; k++) {                /* acc = R^(2^k): kept for k = 0 and k >= 5, as pab_tables does */
        if (k == 0 || k >= 5) memcpy(r_pow + 32 * lev++, acc, sizeof(acc));
        for (int b = 0; b < 32; b++) t[b] = pab_apply(acc, acc[b]);
        memcpy(acc, t, sizeof(t));
    }
}

/* host mirror of part (a) of pab_hash with `lanes` lanes */
extern "C" uint32_t qldpc_privamp_key_functional(const uint32_t *key_words, int workbits, int lanes)
{
    if (!key_words || workbits <= 0 || lanes < 1) return 0;
    uint32_t at_pow[PAB_AT_LEVELS * 32];
    pab_host_at_pow(at_pow);
    const int numwords = (int)(((int64_t)workbits + 31) / 32);
    if (pab_bits((uint32_t)numwords - 1u) > PAB_AT_LEVELS) return 0;
    const int c = (numwords + lanes - 1) / lanes;
    uint32_t v = 0;
    for (int l = 0; l < lanes; l++) {
        const int64_t s64 = (int64_t)l * c;
        if (s64 >= numwords) break;
        const int start = (int)s64, end = start + c < numwords ? start + c : numwords;
        v ^= pab_fold_chunk(key_words, start, end, numwords, hb_tail_mask(workbits), at_pow);
    }
    return v;
}

/* host mirror of part (b) */
extern "C" int qldpc_privamp_expand_host(uint32_t functional, int workbits, uint32_t seed, int final_bits, uint32_t *final_words)
{
    if (workbits <= 0 || final_bits < 0 || final_bits > HB_MAX_BITS) { qldpc_set_error("privamp_expand_host: workbits=%d final_bits=%d", workbits, final_bits); return QLDPC_ESIZE; }
    if (final_bits == 0) return QLDPC_OK;
    if (!final_words) return QLDPC_EINVAL;
    const int numwords = (int)(((int64_t)workbits + 31) / 32);
    const uint32_t outwords = ((uint32_t)final_bits + 31u) / 32u;
    const int levels = 1 + pab_bits(outwords - 1u);
    uint32_t r_pow[PAB_R_LEVELS * 32];
    pab_host_r_pow(numwords, levels, r_pow);
    uint32_t u[32];
    u[0] = functional;
    for (int k = 1; k < 32; k++) {
        u[k] = 0;
        for (int b = 0; b < 32; b++) u[k] |= pab_parity(r_pow[b] & u[k - 1]) << b;
    }
    for (uint32_t w = 0; w < outwords; w++) final_words[w] = pab_out_word(w, seed, u, r_pow);
    final_words[outwords - 1] &= hb_tail_mask(final_bits);
    return QLDPC_OK;
}

struct qldpc_privamp_ctx {
    hb_stage st;                   /* the head of a call of n blocks: [n descriptor rows][n table numwords] */
    uint32_t *d_at, *d_rtabs;
    uint32_t *sort_buf;            /* max_blocks numwords, to number the distinct ones */
};

static const hb_names pab_names = {"workbits", "final_bits"};
static size_t pab_desc_words(int n) { return (size_t)n * (sizeof(pab_desc) / 4); }
static size_t pab_head_words(int n) { return pab_desc_words(n) + (size_t)n; }

extern "C" void qldpc_privamp_free(qldpc_privamp_ctx *pa)
{
    if (!pa) return;
    hb_free(&pa->st);
    free(pa->sort_buf);
    delete pa;
}

static int pab_create(qldpc_privamp_ctx *pa, int device, const hb_limits *lim)
{
    int rc = hb_create(&pa->st, device, lim, pab_head_words(1), 0, "privamp_create", &pab_names);
    if (rc) return rc;
    const size_t rtab_words = (size_t)lim->max_blocks * PAB_R_LEVELS * 32, at_words = (size_t)PAB_AT_LEVELS * 32;
    pa->sort_buf = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)lim->max_blocks);
    if (!pa->sort_buf) return QLDPC_ENOMEM;
    if ((rc = dm_alloc(&pa->st.mem, &pa->d_at, at_words)) || (rc = dm_alloc(&pa->st.mem, &pa->d_rtabs, rtab_words))) return rc;
    uint32_t at_pow[PAB_AT_LEVELS * 32];
    pab_host_at_pow(at_pow);
    HIPCHK(hipMemcpy(pa->d_at, at_pow, sizeof(at_pow), hipMemcpyHostToDevice));
    return QLDPC_OK;
}

extern "C" int qldpc_privamp_create(int device, int max_blocks, int max_key_bits, int max_final_bits, qldpc_privamp_ctx **out)
{
    if (!out) return QLDPC_EINVAL;
    *out = nullptr;
    qldpc_privamp_ctx *pa = new (std::nothrow) qldpc_privamp_ctx();
    if (!pa) return QLDPC_ENOMEM;
    const hb_limits lim = {max_blocks, max_key_bits, max_final_bits};
    const int rc = pab_create(pa, device, &lim);
    if (rc) { qldpc_privamp_free(pa); return rc; }
    *out = pa;
    return QLDPC_OK;
}

extern "C" size_t qldpc_privamp_device_bytes(const qldpc_privamp_ctx *pa) { return pa ? pa->st.mem.dev_bytes : 0; }

static int pab_cmp_u32(const void *a, const void *b)
{
    const uint32_t x = *(const uint32_t *)a, y = *(const uint32_t *)b;
    return x < y ? -1 : x > y;
}

/* the layout of the call as descriptor rows, and the numbering of the distinct numwords, into the pinned staging; *n_tabs out */
static hb_sums pab_fill(qldpc_privamp_ctx *pa, int n, const int *workbits, const uint32_t *seeds, const int *final_bits, const hb_strides *strides, int *n_tabs)
{
    const hb_row *rows = pa->st.rows;
    const hb_sums sums = hb_layout(n, workbits, final_bits, nullptr, strides, 0, pa->st.rows);
    pab_desc *descs = (pab_desc *)pa->st.h_in;
    uint32_t *tab_nw = pa->st.h_in + pab_desc_words(n);
    int nt = 0;
    for (int i = 0; i < n; i++) pa->sort_buf[i] = rows[i].key_words;
    qsort(pa->sort_buf, (size_t)n, sizeof(uint32_t), pab_cmp_u32);
    for (int i = 0; i < n; i++)
        if (!i || pa->sort_buf[i] != pa->sort_buf[i - 1]) tab_nw[nt++] = pa->sort_buf[i];
    for (int i = 0; i < n; i++) {
        int lo = 0, hi = nt - 1;                                 /* tab_nw is ascending */
        while (lo < hi) { const int mid = (lo + hi) / 2; if (tab_nw[mid] < rows[i].key_words) lo = mid + 1; else hi = mid; }
        descs[i] = pab_desc{rows[i].key_words, hb_tail_mask(workbits[i]), seeds[i], (uint32_t)final_bits[i], rows[i].key_off, rows[i].out_off, (uint32_t)lo, 0};
    }
    *n_tabs = nt;
    return sums;
}

/* widest: the words of the call's longest output row, > 0 */
static int pab_launch(qldpc_privamp_ctx *pa, int n, int n_tabs, uint32_t widest, const uint32_t *d_keys, uint32_t *d_out, hipStream_t s)
{
    const uint32_t *d_in = pa->st.d_in;
    hipLaunchKernelGGL(pab_tables, dim3((unsigned)n_tabs), dim3(64), 0, s, d_in + pab_desc_words(n), pa->d_rtabs);
    hipLaunchKernelGGL(pab_hash, dim3((widest + PAB_LANES - 1) / PAB_LANES, (unsigned)n), dim3(PAB_LANES), 0, s, (const pab_desc *)d_in, d_keys, d_out, (const uint32_t *)pa->d_at, (const uint32_t *)pa->d_rtabs);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { qldpc_set_error("privamp_blocks launch: %s", hipGetErrorString(e)); return QLDPC_EHIP; }
    return QLDPC_OK;
}

extern "C" int qldpc_privamp_blocks(qldpc_privamp_ctx *pa, int n, const uint32_t *const *key_words, const int *workbits,
                                    const uint32_t *seeds, const int *final_bits, uint32_t *const *final_words)
{
    int rc = pa ? hb_check_blocks(&pa->st.lim, n, workbits, final_bits, !seeds, "privamp_blocks", &pab_names) : QLDPC_EINVAL;
    if (rc || n == 0) return rc;
    if (!key_words || !final_words) { qldpc_set_error("privamp_blocks: NULL argument array"); return QLDPC_EINVAL; }
    hb_stage *st = &pa->st;
    if ((rc = hb_check_rows(n, final_bits, key_words, nullptr, final_words, "privamp_blocks")) || (rc = hb_begin(st))) return rc;
    int n_tabs = 0;
    const hb_sums sums = pab_fill(pa, n, workbits, seeds, final_bits, nullptr, &n_tabs);
    if (sums.widest_out == 0) return QLDPC_OK;                   /* every block asks for 0 bits */
    const size_t head = pab_head_words(n);
    return hb_run_host(st, n, key_words, st->h_in + head, head + sums.key_words, sums.out_words, final_words,
                       [&](hipStream_t s) { return pab_launch(pa, n, n_tabs, sums.widest_out, st->d_in + head, st->d_out, s); });
}

extern "C" int qldpc_privamp_blocks_dev(qldpc_privamp_ctx *pa, int n, const uint32_t *d_keys, size_t key_stride, const int *workbits,
                                        const uint32_t *seeds, const int *final_bits, uint32_t *d_out, size_t out_stride, void *hip_stream)
{
    int rc = pa ? hb_check_blocks(&pa->st.lim, n, workbits, final_bits, !seeds, "privamp_blocks_dev", &pab_names) : QLDPC_EINVAL;
    if (rc || n == 0) return rc;
    if (!d_keys || !d_out) { qldpc_set_error("privamp_blocks_dev: NULL device pointer"); return QLDPC_EINVAL; }
    const hb_strides strides = {key_stride, out_stride, 0};
    if ((rc = hb_check_strides(n, workbits, final_bits, nullptr, &strides, "privamp_blocks_dev", &pab_names)) || (rc = hb_begin(&pa->st))) return rc;
    int n_tabs = 0;
    const hb_sums sums = pab_fill(pa, n, workbits, seeds, final_bits, &strides, &n_tabs);
    if (sums.widest_out == 0) return QLDPC_OK;
    return hb_run_dev(&pa->st, pab_head_words(n), (hipStream_t)hip_stream,
                      [&](hipStream_t s) { return pab_launch(pa, n, n_tabs, sums.widest_out, d_keys, d_out, s); });
}
