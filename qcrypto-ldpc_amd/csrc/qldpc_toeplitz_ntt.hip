/*
 * qldpc_toeplitz_ntt.hip -- the Toeplitz hash as a cyclic convolution over Z_p (QLDPC_TOEPLITZ_NTT): the same words as tz_hash, bit for
 * bit, in O(L log L) for L >= n + m - 1 where the direct product takes n m.  The arithmetic, the pass decomposition and the tile geometry
 * are qldpc_toeplitz_ntt_core.h; this file holds the two pass kernels, the host mirror that walks the same tiles, and the batching.
 *
 * tzn_fwd<B, SRC>: one pass of the forward transform (decimation in frequency).  grid = (tiles of the transform, blocks of the launch),
 *     TZN_LANES lanes; a workgroup loads its tile of 2^(B+5) residues into LDS in address order (runs of >= 32 adjacent residues, a
 *     whole contiguous stretch in the lower passes), runs the b stages of its 2^b-point row transforms there, and stores the tile with
 *     the factor between passes applied.  SRC 1 / 2 (pass 0 only): the tile is unpacked from the key / seed words, L / 8 bytes read
 *     where a residue pass would read 4 L.
 * tzn_inv<B, PRODUCT, OUTPUT>: one pass of the inverse (factor, then decimation in time), the passes in the opposite order.  PRODUCT (the
 *     first one): the tile is loaded as key spectrum x seed spectrum.  OUTPUT (the last one): nothing is written back; the residues
 *     are scaled by 1 / L, reduced, and the low bits of the m outputs leave as packed words, 32 lanes per word by ballot.
 *
 * Passes are separate launches in stream order; no workgroup waits for another.  Blocks of equal L share launches (the block is the y
 * dimension of the grid, one tzn_desc row each).  The work area holds, per block in flight, the key spectrum (which becomes the product
 * and then the inverse in place) and the seed spectrum, or one seed spectrum per L when the call shares its seed; a group that does not
 * fit runs in rounds.
 */
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>

#include "qldpc_hip.h"
#include "qldpc_toeplitz_core.h"
#include "qldpc_toeplitz_int.h"
#include "qldpc_toeplitz_ntt_core.h"

#define TZN_LANES 512
#define TZN_DEFAULT_WORK ((size_t)1 << 30)

struct tzn_tab {                   /* all in Montgomery form */
    const uint32_t *w, *wi;        /* w_(2^B)^x and w_(2^B)^-x, x < 2^(B-1): the stages inside a tile */
    const uint32_t *lo, *hi;       /* w_(2^kmax)^x = lo[x mod 2^kl] hi[x >> kl]: the factors between passes */
    uint32_t kl, kmax;
};

struct tzn_desc {                  /* one row per block of a launch, and one per shared seed spectrum */
    uint32_t n, m, seed_bits, scale;
    uint64_t key_off, seed_off, out_off;      /* words from the key / seed / output base of the call */
    uint64_t a_off, b_off;                    /* residues from the base of the work area: key spectrum, seed spectrum */
};

template <int B, int SRC>
__global__ __launch_bounds__(TZN_LANES) void tzn_fwd(const tzn_desc *__restrict__ descs, const uint32_t *__restrict__ keys,
                                                     const uint32_t *__restrict__ seeds, uint32_t *__restrict__ work, tzn_tab tab,
                                                     uint32_t k, uint32_t pass, uint32_t side)
{
    __shared__ uint32_t s[1u << (B + TZN_COLS_LOG2)];
    const tzn_desc d = descs[blockIdx.y];
    const tzn_pass ps = tzn_pass_of(k, B, pass);
    const uint32_t E = 1u << ps.le, tile = blockIdx.x, t = threadIdx.x;
    uint32_t *__restrict__ x = work + ((SRC == 2 || (SRC == 0 && side)) ? d.b_off : d.a_off);
#pragma unroll 4
    for (uint32_t e = t; e < E; e += TZN_LANES) {
        uint32_t lo;
        const uint32_t g = tzn_index(ps, tile, e, &lo);
        s[e] = SRC == 1 ? tzn_key_residue(keys + d.key_off, d.n, k, g) : SRC == 2 ? tzn_seed_residue(seeds + d.seed_off, d.seed_bits, g) : x[g];
    }
    for (uint32_t lh = ps.b; lh-- > 0;) {
        __syncthreads();
        for (uint32_t u = t; u < E / 2u; u += TZN_LANES) {
            const uint32_t pos = tzn_pair(ps, u, lh);
            tzn_dif(&s[pos], &s[pos + (1u << (ps.sp + lh))], tab.w[tzn_pair_twiddle(ps, pos, lh, B)]);
        }
    }
    __syncthreads();
    for (uint32_t e = t; e < E; e += TZN_LANES) {
        uint32_t lo;
        const uint32_t g = tzn_index(ps, tile, e, &lo);
        uint32_t v = s[e];
        if (ps.sh) v = tzn_mont(v, tzn_twiddle(tab.lo, tab.hi, tab.kl, tab.kmax, tzn_factor(ps, e, lo, tab.kmax), 0));
        x[g] = v;
    }
}

template <int B, bool PRODUCT, bool OUTPUT>
__global__ __launch_bounds__(TZN_LANES) void tzn_inv(const tzn_desc *__restrict__ descs, uint32_t *__restrict__ work, uint32_t *__restrict__ outs,
                                                     tzn_tab tab, uint32_t k, uint32_t pass)
{
    __shared__ uint32_t s[1u << (B + TZN_COLS_LOG2)];
    const tzn_desc d = descs[blockIdx.y];
    const tzn_pass ps = tzn_pass_of(k, B, pass);
    const uint32_t E = 1u << ps.le, tile = blockIdx.x, t = threadIdx.x;
    uint32_t *__restrict__ x = work + d.a_off;
    const uint32_t *__restrict__ y = work + d.b_off;
#pragma unroll 4
    for (uint32_t e = t; e < E; e += TZN_LANES) {
        uint32_t lo;
        const uint32_t g = tzn_index(ps, tile, e, &lo);
        uint32_t v = x[g];
        if (PRODUCT) v = tzn_mont(v, y[g]);
        if (ps.sh) v = tzn_mont(v, tzn_twiddle(tab.lo, tab.hi, tab.kl, tab.kmax, tzn_factor(ps, e, lo, tab.kmax), 1));
        s[e] = v;
    }
    for (uint32_t lh = 0; lh < ps.b; lh++) {
        __syncthreads();
        for (uint32_t u = t; u < E / 2u; u += TZN_LANES) {
            const uint32_t pos = tzn_pair(ps, u, lh);
            tzn_dit(&s[pos], &s[pos + (1u << (ps.sp + lh))], tab.wi[tzn_pair_twiddle(ps, pos, lh, B)]);
        }
    }
    __syncthreads();
    if (!OUTPUT) {
        for (uint32_t e = t; e < E; e += TZN_LANES) {
            uint32_t lo;
            x[tzn_index(ps, tile, e, &lo)] = s[e];
        }
        return;
    }
    /* 32 adjacent positions of a tile are 32 adjacent indices from a multiple of 32 on (B >= 5), and tzn_out_base is a multiple of 32:
       a half wave holds one whole output word or none of it */
    for (uint32_t e0 = 0; e0 < E; e0 += TZN_LANES) {
        const uint32_t e = e0 + t;
        const bool in = e < E;
        uint32_t lo;
        const uint32_t i = tzn_out_index(d.n, k, tzn_index(ps, tile, in ? e : 0u, &lo));
        const bool live = in && i < d.m;
        const unsigned long long votes = __ballot(live && tzn_out_bit(s[in ? e : 0u], d.scale));
        if ((t & 31u) == 0 && live) outs[d.out_off + (i >> 5)] = tz_brev((uint32_t)(votes >> (t & 32u)));
    }
}

/* ------------------------------------------------------------------ tables ---- */

static uint32_t tzn_to_mont(uint32_t a) { return tzn_mul(a, TZN_R1); }

static size_t tzn_table_words(uint32_t B, uint32_t kmax)
{
    const uint32_t kl = tzn_table_split(kmax);
    return 2 * ((size_t)1 << (B - 1)) + ((size_t)1 << kl) + ((size_t)1 << (kmax - kl));
}

/* w, wi, lo, hi one after the other in `words` (tzn_table_words of them), by exact integer arithmetic; *tab points into `base`, the
   address the words will be read at */
static void tzn_build_tables(uint32_t B, uint32_t kmax, uint32_t *words, const uint32_t *base, tzn_tab *tab)
{
    const uint32_t kl = tzn_table_split(kmax), half = 1u << (B - 1);
    uint32_t *w = words, *wi = w + half, *lo = wi + half, *hi = lo + ((size_t)1 << kl);
    const uint32_t rb = tzn_to_mont(tzn_root(B)), rbi = tzn_to_mont(tzn_pow(tzn_root(B), TZN_P - 2u));
    w[0] = wi[0] = TZN_R1;
    for (uint32_t x = 1; x < half; x++) { w[x] = tzn_mont(w[x - 1], rb); wi[x] = tzn_mont(wi[x - 1], rbi); }
    const uint32_t r = tzn_root(kmax), rl = tzn_to_mont(r), rh = tzn_to_mont(tzn_pow(r, 1u << kl));
    lo[0] = hi[0] = TZN_R1;
    for (uint32_t x = 1; x < (1u << kl); x++) lo[x] = tzn_mont(lo[x - 1], rl);
    for (uint32_t x = 1; x < (1u << (kmax - kl)); x++) hi[x] = tzn_mont(hi[x - 1], rh);
    tab->w = base; tab->wi = base + half; tab->lo = base + 2 * (size_t)half; tab->hi = tab->lo + ((size_t)1 << kl);
    tab->kl = kl; tab->kmax = kmax;
}

/* ------------------------------------------------------------------ host mirror ---- */

/* one forward pass over the whole transform, tile by tile as tzn_fwd walks it; bits: the packed row of pass 0 (src 1 key / 2 seed) */
static void tzn_host_fwd(uint32_t *x, uint32_t *s, uint32_t k, uint32_t B, uint32_t pass, const tzn_tab &tab, int src, const uint32_t *bits, uint32_t count)
{
    const tzn_pass ps = tzn_pass_of(k, B, pass);
    const uint32_t E = 1u << ps.le;
    for (uint32_t tile = 0; tile < (1u << (k - ps.le)); tile++) {
        uint32_t lo;
        for (uint32_t e = 0; e < E; e++) {
            const uint32_t g = tzn_index(ps, tile, e, &lo);
            s[e] = src == 1 ? tzn_key_residue(bits, count, k, g) : src == 2 ? tzn_seed_residue(bits, count, g) : x[g];
        }
        for (uint32_t lh = ps.b; lh-- > 0;)
            for (uint32_t u = 0; u < E / 2u; u++) {
                const uint32_t pos = tzn_pair(ps, u, lh);
                tzn_dif(&s[pos], &s[pos + (1u << (ps.sp + lh))], tab.w[tzn_pair_twiddle(ps, pos, lh, B)]);
            }
        for (uint32_t e = 0; e < E; e++) {
            const uint32_t g = tzn_index(ps, tile, e, &lo);
            x[g] = ps.sh ? tzn_mont(s[e], tzn_twiddle(tab.lo, tab.hi, tab.kl, tab.kmax, tzn_factor(ps, e, lo, tab.kmax), 0)) : s[e];
        }
    }
}

/* one inverse pass as tzn_inv; y: the seed spectrum of the first pass, out: the words of the last one (zeroed by the caller) */
static void tzn_host_inv(uint32_t *x, const uint32_t *y, uint32_t *s, uint32_t k, uint32_t B, uint32_t pass, const tzn_tab &tab,
                         uint32_t n, uint32_t m, uint32_t *out)
{
    const tzn_pass ps = tzn_pass_of(k, B, pass);
    const uint32_t E = 1u << ps.le, scale = tzn_scale(k);
    for (uint32_t tile = 0; tile < (1u << (k - ps.le)); tile++) {
        uint32_t lo;
        for (uint32_t e = 0; e < E; e++) {
            const uint32_t g = tzn_index(ps, tile, e, &lo);
            uint32_t v = y ? tzn_mont(x[g], y[g]) : x[g];
            if (ps.sh) v = tzn_mont(v, tzn_twiddle(tab.lo, tab.hi, tab.kl, tab.kmax, tzn_factor(ps, e, lo, tab.kmax), 1));
            s[e] = v;
        }
        for (uint32_t lh = 0; lh < ps.b; lh++)
            for (uint32_t u = 0; u < E / 2u; u++) {
                const uint32_t pos = tzn_pair(ps, u, lh);
                tzn_dit(&s[pos], &s[pos + (1u << (ps.sp + lh))], tab.wi[tzn_pair_twiddle(ps, pos, lh, B)]);
            }
        for (uint32_t e = 0; e < E; e++) {
            const uint32_t g = tzn_index(ps, tile, e, &lo);
            if (!out) { x[g] = s[e]; continue; }
            const uint32_t i = tzn_out_index(n, k, g);
            if (i < m) out[i >> 5] |= tzn_out_bit(s[e], scale) << (31u - (i & 31u));
        }
    }
}

extern "C" int qldpc_toeplitz_ntt_host(const uint32_t *key_words, int key_bits, const uint32_t *seed_words, int out_bits, int pass_log2, uint32_t *out_words)
{
    if (key_bits <= 0 || out_bits < 0 || key_bits > TZ_MAX_BITS || out_bits > TZ_MAX_BITS) {
        qldpc_set_error("toeplitz_ntt_host: key_bits=%d out_bits=%d", key_bits, out_bits);
        return QLDPC_ESIZE;
    }
    if (pass_log2 < 0 || pass_log2 > TZN_MAX_LOG2) { qldpc_set_error("toeplitz_ntt_host: pass_log2=%d (0 .. %d)", pass_log2, TZN_MAX_LOG2); return QLDPC_EINVAL; }
    if (out_bits == 0) return QLDPC_OK;
    if (!key_words || !seed_words || !out_words) return QLDPC_EINVAL;
    const uint32_t B = pass_log2 ? (uint32_t)pass_log2 : (uint32_t)QLDPC_TOEPLITZ_PASS_LOG2, k = (uint32_t)tzn_log2_len(key_bits, out_bits);
    const uint32_t P = tzn_passes(k, B), n = (uint32_t)key_bits, m = (uint32_t)out_bits;
    const size_t L = (size_t)1 << k, tile = (size_t)1 << tzn_pass_of(k, B, 0).le;
    uint32_t *mem = (uint32_t *)malloc(4 * (2 * L + tile + tzn_table_words(B, k)));
    if (!mem) return QLDPC_ENOMEM;
    uint32_t *a = mem, *b = a + L, *s = b + L, *tw = s + tile;
    tzn_tab tab;
    tzn_build_tables(B, k, tw, tw, &tab);
    for (uint32_t pass = 0; pass < P; pass++) {
        tzn_host_fwd(a, s, k, B, pass, tab, pass ? 0 : 1, key_words, n);
        tzn_host_fwd(b, s, k, B, pass, tab, pass ? 0 : 2, seed_words, n + m - 1u);
    }
    memset(out_words, 0, 4 * (((size_t)m + 31) / 32));
    for (uint32_t pass = P; pass-- > 0;) tzn_host_inv(a, pass == P - 1u ? b : nullptr, s, k, B, pass, tab, n, m, pass ? nullptr : out_words);
    free(mem);
    return QLDPC_OK;
}

extern "C" size_t qldpc_toeplitz_ntt_length(int key_bits, int out_bits)
{
    if (key_bits > TZ_MAX_BITS || out_bits > TZ_MAX_BITS) return 0;
    const int k = tzn_log2_len(key_bits, out_bits);
    return k < 0 ? 0 : (size_t)1 << k;
}

extern "C" uint32_t qldpc_toeplitz_ntt_mul_host(uint32_t a, uint32_t b) { return tzn_mul(a % TZN_P, b % TZN_P); }

extern "C" uint32_t qldpc_toeplitz_ntt_root_host(int log2_len) { return log2_len < 0 || log2_len > TZN_MAX_LOG2 ? 0u : tzn_root((uint32_t)log2_len); }

/* ------------------------------------------------------------------ the context's side ---- */

struct tzn_state {
    uint32_t B, kmax;
    size_t work_res;               /* residues of the work area */
    uint32_t *d_work, *d_tab;
    tzn_tab tab;
    tzn_desc *h_desc, *d_desc;     /* max_blocks rows and one per distinct L */
    int *order;                    /* the blocks of a call sorted by L */
};

void tzn_free(qldpc_toeplitz_ctx *tz)
{
    tzn_state *st = tz->ntt;
    if (!st) return;
    free(st->order);
    delete st;
    tz->ntt = nullptr;
}

static uint32_t tzn_ctx_log2(const qldpc_toeplitz_ctx *tz)
{
    const int k = tzn_log2_len(tz->st.lim.max_key_bits, tz->st.lim.max_out_bits);
    return k < 0 ? (uint32_t)TZN_MIN_LOG2 : (uint32_t)k;
}

int tzn_create(qldpc_toeplitz_ctx *tz, int pass_log2, size_t work_bytes)
{
    tzn_state *st = new (std::nothrow) tzn_state();
    if (!st) return QLDPC_ENOMEM;
    tz->ntt = st;
    st->B = pass_log2 ? (uint32_t)pass_log2 : (uint32_t)QLDPC_TOEPLITZ_PASS_LOG2;
    st->kmax = tzn_ctx_log2(tz);
    const size_t one = (size_t)8 << st->kmax;                    /* two arrays of L residues */
    if (work_bytes == 0) {
        size_t blocks = TZN_DEFAULT_WORK / one;
        if (blocks > (size_t)tz->st.lim.max_blocks) blocks = (size_t)tz->st.lim.max_blocks;
        work_bytes = one * (blocks ? blocks : 1);
    }
    if (work_bytes < one) { qldpc_set_error("toeplitz_create_cfg: work_bytes=%zu, one block of the context's sizes takes %zu", work_bytes, one); return QLDPC_ESIZE; }
    st->work_res = work_bytes / 4;
    const size_t tw = tzn_table_words(st->B, st->kmax), rows = (size_t)tz->st.lim.max_blocks + TZN_MAX_LOG2 + 1;
    uint32_t *h_tab = (uint32_t *)malloc(4 * tw);
    st->order = (int *)malloc(sizeof(int) * (size_t)tz->st.lim.max_blocks);
    if (!h_tab || !st->order) { free(h_tab); return QLDPC_ENOMEM; }
    int rc = QLDPC_OK;
    dm_ledger *m = &tz->st.mem;
    if (dm_alloc(m, &st->d_work, st->work_res) || dm_alloc(m, &st->d_tab, tw) || dm_alloc(m, &st->d_desc, rows) || dm_alloc_pinned(m, &st->h_desc, rows)) {
        qldpc_set_error("toeplitz_create_cfg: no memory for a work area of %zu bytes", 4 * st->work_res);
        rc = QLDPC_ENOMEM;
    }
    if (!rc) {
        tzn_build_tables(st->B, st->kmax, h_tab, st->d_tab, &st->tab);
        if (hipMemcpy(st->d_tab, h_tab, 4 * tw, hipMemcpyHostToDevice) != hipSuccess) { qldpc_set_error("toeplitz_create_cfg: the tables did not reach the device"); rc = QLDPC_EHIP; }
    }
    free(h_tab);
    return rc;
}

template <int B>
static void tzn_launch_fwd(int src, dim3 grid, hipStream_t s, const tzn_desc *descs, const uint32_t *keys, const uint32_t *seeds, uint32_t *work,
                           const tzn_tab &tab, uint32_t k, uint32_t pass, uint32_t side)
{
    if (src == 1) hipLaunchKernelGGL((tzn_fwd<B, 1>), grid, dim3(TZN_LANES), 0, s, descs, keys, seeds, work, tab, k, pass, side);
    else if (src == 2) hipLaunchKernelGGL((tzn_fwd<B, 2>), grid, dim3(TZN_LANES), 0, s, descs, keys, seeds, work, tab, k, pass, side);
    else hipLaunchKernelGGL((tzn_fwd<B, 0>), grid, dim3(TZN_LANES), 0, s, descs, keys, seeds, work, tab, k, pass, side);
}

template <int B>
static void tzn_launch_inv(bool product, bool output, dim3 grid, hipStream_t s, const tzn_desc *descs, uint32_t *work, uint32_t *outs,
                           const tzn_tab &tab, uint32_t k, uint32_t pass)
{
    if (product && output) hipLaunchKernelGGL((tzn_inv<B, true, true>), grid, dim3(TZN_LANES), 0, s, descs, work, outs, tab, k, pass);
    else if (product) hipLaunchKernelGGL((tzn_inv<B, true, false>), grid, dim3(TZN_LANES), 0, s, descs, work, outs, tab, k, pass);
    else if (output) hipLaunchKernelGGL((tzn_inv<B, false, true>), grid, dim3(TZN_LANES), 0, s, descs, work, outs, tab, k, pass);
    else hipLaunchKernelGGL((tzn_inv<B, false, false>), grid, dim3(TZN_LANES), 0, s, descs, work, outs, tab, k, pass);
}

/* every pass of the forward transform of `count` rows from `descs` on: src 1 key -> a, 2 seed -> b */
static void tzn_forward(const tzn_state *st, int src, unsigned count, hipStream_t s, const tzn_desc *descs, const uint32_t *keys, const uint32_t *seeds, uint32_t k,
                        uint64_t *launches)
{
    const uint32_t P = tzn_passes(k, st->B);
    const dim3 grid(1u << (k - tzn_pass_of(k, st->B, 0).le), count);
    for (uint32_t pass = 0; pass < P; pass++, ++*launches) {
        if (st->B == QLDPC_TOEPLITZ_PASS_LOG2) tzn_launch_fwd<QLDPC_TOEPLITZ_PASS_LOG2>(pass ? 0 : src, grid, s, descs, keys, seeds, st->d_work, st->tab, k, pass, src == 2);
        else tzn_launch_fwd<QLDPC_TOEPLITZ_PASS_LOG2_SMALL>(pass ? 0 : src, grid, s, descs, keys, seeds, st->d_work, st->tab, k, pass, src == 2);
    }
}

static void tzn_inverse(const tzn_state *st, unsigned count, hipStream_t s, const tzn_desc *descs, uint32_t *outs, uint32_t k, uint64_t *launches)
{
    const uint32_t P = tzn_passes(k, st->B);
    const dim3 grid(1u << (k - tzn_pass_of(k, st->B, 0).le), count);
    for (uint32_t pass = P; pass-- > 0; ++*launches) {
        if (st->B == QLDPC_TOEPLITZ_PASS_LOG2) tzn_launch_inv<QLDPC_TOEPLITZ_PASS_LOG2>(pass == P - 1u, pass == 0, grid, s, descs, st->d_work, outs, st->tab, k, pass);
        else tzn_launch_inv<QLDPC_TOEPLITZ_PASS_LOG2_SMALL>(pass == P - 1u, pass == 0, grid, s, descs, st->d_work, outs, st->tab, k, pass);
    }
}

int tzn_blocks(qldpc_toeplitz_ctx *tz, int n, const tz_desc *rows, const int *key_bits, int shared,
               const uint32_t *d_keys, const uint32_t *d_seeds, uint32_t *d_out, hipStream_t s)
{
    tzn_state *st = tz->ntt;
    uint64_t *stats = tz->stats;
    memset(stats, 0, sizeof(tz->stats));
    /* the blocks by ascending L (a counting sort on log2 L); blocks that ask for 0 bits take no part */
    int first[TZN_MAX_LOG2 + 2] = {0};
    uint32_t held = 0;                                           /* bits a shared seed row holds for certain: the longest seed of the call */
    for (int i = 0; i < n; i++) {
        const int k = tzn_log2_len(key_bits[i], (int)rows[i].out_bits);
        if (k < 0) continue;
        first[k + 1]++;
        if (32u * rows[i].seed_words > held) held = 32u * rows[i].seed_words;
    }
    for (int k = 0; k <= TZN_MAX_LOG2; k++) first[k + 1] += first[k];
    int fill[TZN_MAX_LOG2 + 1];
    memcpy(fill, first, sizeof(fill));
    for (int i = 0; i < n; i++) {
        const int k = tzn_log2_len(key_bits[i], (int)rows[i].out_bits);
        if (k >= 0) st->order[fill[k]++] = i;
    }
    /* every descriptor row of the call first (one upload), a group's shared seed row ahead of its blocks; a block's slot in the work area is
       its place in its round */
    size_t row = 0;
    for (uint32_t k = TZN_MIN_LOG2; k <= (uint32_t)TZN_MAX_LOG2; k++) {
        const int cnt = first[k + 1] - first[k];
        if (!cnt) continue;
        const size_t L = (size_t)1 << k;
        const size_t cap = shared ? st->work_res / L - 1 : st->work_res / (2 * L);      /* >= 1: the work area holds a block of the largest L */
        if (shared) {
            tzn_desc &d = st->h_desc[row++];
            memset(&d, 0, sizeof(d));
            d.seed_bits = held < L ? held : (uint32_t)L;
            d.seed_off = rows[st->order[first[k]]].seed_off;
        }
        for (int j = 0; j < cnt; j++) {
            const int i = st->order[first[k] + j];
            const size_t slot = (size_t)j % (cap < 65535 ? cap : 65535);
            tzn_desc &d = st->h_desc[row++];
            d.n = (uint32_t)key_bits[i]; d.m = rows[i].out_bits; d.seed_bits = d.n + d.m - 1u; d.scale = tzn_scale(k);
            d.key_off = rows[i].key_off; d.seed_off = rows[i].seed_off; d.out_off = rows[i].out_off;
            d.a_off = shared ? (slot + 1) * L : 2 * slot * L;
            d.b_off = shared ? 0 : d.a_off + L;
        }
        stats[4]++;
        stats[5] = L;
    }
    if (!row) return QLDPC_OK;
    HIPCHK(hipMemcpyAsync(st->d_desc, st->h_desc, row * sizeof(tzn_desc), hipMemcpyHostToDevice, s));
    row = 0;
    for (uint32_t k = TZN_MIN_LOG2; k <= (uint32_t)TZN_MAX_LOG2; k++) {
        const int cnt = first[k + 1] - first[k];
        if (!cnt) continue;
        const size_t L = (size_t)1 << k;
        size_t cap = shared ? st->work_res / L - 1 : st->work_res / (2 * L);
        if (cap > 65535) cap = 65535;                            /* blocks are the y dimension of the grid */
        if (shared) {
            tzn_forward(st, 2, 1, s, st->d_desc + row, d_keys, d_seeds, k, &stats[0]);
            row++; stats[1]++;
        }
        for (int j = 0; j < cnt; j += (int)cap, stats[3]++) {
            const unsigned nb = (unsigned)(cnt - j < (int)cap ? cnt - j : (int)cap);
            tzn_forward(st, 1, nb, s, st->d_desc + row, d_keys, d_seeds, k, &stats[0]);
            if (!shared) tzn_forward(st, 2, nb, s, st->d_desc + row, d_keys, d_seeds, k, &stats[0]);
            tzn_inverse(st, nb, s, st->d_desc + row, d_out, k, &stats[0]);
            stats[1] += shared ? nb : 2 * nb;
            stats[2] += nb;
            row += nb;
        }
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { qldpc_set_error("toeplitz_blocks (ntt) launch: %s", hipGetErrorString(e)); return QLDPC_EHIP; }
    return QLDPC_OK;
}
