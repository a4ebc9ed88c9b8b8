/*
 * qldpc_polyhash.hip -- error verification by a universal hash for a batch of blocks in one launch (qldpc_polyhash_*): polynomial evaluation
 * over p = 2^61 - 1 with the block's length as a coefficient, 1 .. 4 independent keys per block.  The hash, its arithmetic and the
 * decomposition are qldpc_polyhash_core.h; the staging and the reuse rule of a context are qldpc_hashbatch.h's.
 *
 * ph_hash: grid = (tiles of the call's longest block, blocks), 256 lanes.  A workgroup hashes one tile of at most `tile` coefficients of one
 *     block under all NK keys.  Lane t owns the words 4t .. 4t+3 of every 16-byte-aligned row of PH_T = 1024 words: one dwordx4 load per
 *     row, the next row's load issued before this row's multiplies, and 4 NK independent accumulators h = h K + word with K = k^1024 (one
 *     ph_mul_add per key word and key).  Rows need not start on a 16-byte boundary: the tile is shifted to the boundary below it, and the
 *     rows that hold the masked last word, the length or the tile's end select per word what, if anything, is accumulated.  The table
 *     k^0 .. k^1024 of each key is built in LDS by ten doubling steps while the first load is in flight; it gives K and the lane weights.
 *     The weighted lane values are summed over the wave by shuffles and over the four waves through LDS.  A block of one tile is finished
 *     here (tag = k E); otherwise the tile's partial goes to the work area.
 * ph_fold: grid = (blocks), launched only when some block of the call has more than one tile; a workgroup folds the partials of one block,
 *     the same evaluation with one partial per lane and row and Y = k^tile in place of k.
 * Integer VALU, plain stores, no atomics and nothing that waits on another workgroup.
 */
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>

#include "qldpc_hashbatch.h"
#include "qldpc_hip.h"
#include "qldpc_polyhash_core.h"

#define PH_LANES 256u
#define PH_T (PH_LANE_WORDS * PH_LANES)      /* virtual lanes of a tile: words of a row */
#define PH_WAVES (PH_LANES / 64u)

struct ph_desc {                   /* one row per block, written by the host */
    uint32_t key_words, tail_mask, key_bits, tiles;
    uint64_t key_off, hkey_off, out_off, part_off;      /* in words from the key / hash-key / tag base of the call, in partials from the work area's */
};

/* tab[i] = x^i, i <= n (a power of two), by all lanes of the workgroup; ends behind a barrier */
__device__ static inline void ph_table(uint64_t *tab, uint32_t n, uint64_t x, uint32_t t)
{
    if (t == 0) { tab[0] = 1ull; tab[1] = x; }
    __syncthreads();
    for (uint32_t half = 1; half < n; half *= 2) {
        ph_pow_step(tab, half, n, t, PH_LANES);
        __syncthreads();
    }
}

/* the sum of v over the workgroup, in lane 0; red: PH_WAVES words of LDS that no one reads until the next barrier */
__device__ static inline uint64_t ph_sum(uint64_t v, uint64_t *red, uint32_t t)
{
    for (int off = 32; off > 0; off >>= 1) v = ph_add(v, (uint64_t)__shfl_down((unsigned long long)v, off, 64));
    if ((t & 63u) == 0) red[t >> 6] = v;
    __syncthreads();
    if (t == 0)
        for (uint32_t w = 1; w < PH_WAVES; w++) v = ph_add(v, red[w]);
    return v;
}

template <int NK>
__global__ __launch_bounds__(PH_LANES) void ph_hash(const ph_desc *__restrict__ descs, const uint32_t *__restrict__ keys, const uint32_t *__restrict__ hkeys,
                                                    uint32_t *__restrict__ outs, uint64_t *__restrict__ parts, uint32_t tile)
{
    __shared__ uint64_t s_pow[NK][PH_T + 1];
    __shared__ uint64_t s_red[NK][PH_WAVES];
    const ph_desc d = descs[blockIdx.y];
    const uint32_t tau = blockIdx.x, t = threadIdx.x;
    if (tau >= d.tiles) return;                                  /* the whole workgroup: the grid is as wide as the call's longest block */
    const uint32_t base = tau * tile, m = ph_tile_len(d.key_words + 1u, tile, tau);
    const uint32_t *__restrict__ key = keys + d.key_off;
    const uint32_t a = ph_shift(key + base), avail = ph_tile_avail(d.key_words, base, m);
    const ph_split sp = ph_rows(m, ph_tile_plain(d.key_words, base, m), a, PH_T);
    const uint4 *__restrict__ rows = (const uint4 *)(key + base - a) + t;      /* row i of this lane: rows[i * PH_LANES] */
    /* what this lane holds of row i: a fast row whole, a checked row only where its 16 bytes hold a word of the tile */
    auto load = [&](uint32_t i) {
        return i < sp.fast || ph_group_has_word(i * PH_T + PH_LANE_WORDS * t, a, avail) ? rows[(size_t)i * PH_LANES] : make_uint4(0u, 0u, 0u, 0u);
    };
    uint4 w = load(0u);                                          /* in flight while the tables are built */
    uint64_t k[NK], K[NK], h[NK][PH_LANE_WORDS];
#pragma unroll
    for (int q = 0; q < NK; q++) {
        k[q] = ph_key(hkeys[d.hkey_off + 2 * q], hkeys[d.hkey_off + 2 * q + 1]);
        if (t == 0) { s_pow[q][0] = 1ull; s_pow[q][1] = k[q]; }
    }
    __syncthreads();
    for (uint32_t half = 1; half < PH_T; half *= 2) {
#pragma unroll
        for (int q = 0; q < NK; q++) ph_pow_step(s_pow[q], half, PH_T, t, PH_LANES);
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < NK; q++) {
        K[q] = s_pow[q][PH_T];
#pragma unroll
        for (uint32_t s = 0; s < PH_LANE_WORDS; s++) h[q][s] = 0ull;
    }
    if (sp.fast > 0u && t == 0) {                                /* the a words in front of row 0 are not the tile's */
        if (a > 0u) w.x = 0u;
        if (a > 1u) w.y = 0u;
        if (a > 2u) w.z = 0u;
    }
    /* every row: the next row's load before this row's multiplies; the fast rows first, then the checked ones (two at the most) */
    for (uint32_t i = 0; i < sp.rows; i++) {
        const uint4 cur = w;
        if (i + 1u < sp.rows) w = load(i + 1u);
        const uint32_t c[PH_LANE_WORDS] = {cur.x, cur.y, cur.z, cur.w};
        if (i < sp.fast) {
#pragma unroll
            for (int q = 0; q < NK; q++)
#pragma unroll
                for (uint32_t s = 0; s < PH_LANE_WORDS; s++) h[q][s] = ph_mul_add(h[q][s], K[q], c[s]);
        } else {
#pragma unroll
            for (int q = 0; q < NK; q++)
#pragma unroll
                for (uint32_t s = 0; s < PH_LANE_WORDS; s++)
                    h[q][s] = ph_checked(h[q][s], K[q], c[s], base, i * PH_T + PH_LANE_WORDS * t + s, a, m, d.key_words, d.tail_mask, d.key_bits);
        }
    }
    uint64_t v[NK];
#pragma unroll
    for (int q = 0; q < NK; q++) {
        v[q] = 0ull;
#pragma unroll
        for (uint32_t s = 0; s < PH_LANE_WORDS; s++) v[q] = ph_add(v[q], ph_mul(h[q][s], s_pow[q][ph_weight_exp(sp.r, PH_LANE_WORDS * t + s, PH_T)]));
        v[q] = ph_sum(v[q], s_red[q], t);
    }
    if (t != 0) return;
#pragma unroll
    for (int q = 0; q < NK; q++) {
        if (d.tiles == 1u) ph_store_tag(outs + d.out_off + 2 * q, ph_mul(v[q], k[q]));
        else parts[d.part_off + (uint64_t)tau * NK + q] = v[q];
    }
}

template <int NK>
__global__ __launch_bounds__(PH_LANES) void ph_fold_tiles(const ph_desc *__restrict__ descs, const uint32_t *__restrict__ hkeys, uint32_t *__restrict__ outs,
                                                          const uint64_t *__restrict__ parts, uint32_t tile)
{
    __shared__ uint64_t s_pow[PH_LANES + 1];
    __shared__ uint64_t s_red[PH_WAVES];
    const ph_desc d = descs[blockIdx.x];
    if (d.tiles < 2u) return;                                    /* finished by ph_hash */
    const uint32_t t = threadIdx.x, m = d.tiles - 1u, r = m % PH_LANES;
    const uint64_t *__restrict__ part = parts + d.part_off;
    for (int q = 0; q < NK; q++) {
        const uint64_t k = ph_key(hkeys[d.hkey_off + 2 * q], hkeys[d.hkey_off + 2 * q + 1]);
        ph_table(s_pow, PH_LANES, ph_pow(k, tile), t);
        const uint64_t X = s_pow[PH_LANES];
        uint64_t h = 0ull;
        for (uint32_t j = t; j < m; j += PH_LANES) h = ph_mul_add(h, X, part[(uint64_t)j * NK + q]);
        const uint64_t sum = ph_sum(ph_mul(h, s_pow[ph_weight_exp(r, t, PH_LANES)]), s_red, t);
        if (t == 0) {
            const uint64_t E = ph_mul_add(sum, ph_pow(k, ph_tile_len(d.key_words + 1u, tile, m)), part[(uint64_t)m * NK + q]);
            ph_store_tag(outs + d.out_off + 2 * q, ph_mul(E, k));
        }
        __syncthreads();                                         /* the table and s_red are the next key's */
    }
}

/* ------------------------------------------------------------------ host ---- */

struct qldpc_polyhash_ctx {
    hb_stage st;                   /* the head of a call of n blocks: n descriptor rows; the payload: packed keys, then the hash keys */
    int n_keys;
    uint32_t tile;
    uint32_t max_tiles;            /* of a block of max_key_bits */
    int *tag_bits;                 /* max_blocks times 64 n_keys: the output row of every block, as the shared checks take it */
    uint64_t *d_parts;             /* max_blocks x max_tiles x n_keys partials */
};

static const hb_names ph_names = {"key_bits", "tag_bits"};
static size_t ph_desc_words(int n) { return (size_t)n * (sizeof(ph_desc) / 4); }
/* the third row of a block is its hash key: two words per key, as many as the tag has */
static uint32_t ph_hkey_words(int key_bits, int tag_bits) { (void)key_bits; return (uint32_t)tag_bits / 32u; }

extern "C" void qldpc_polyhash_free(qldpc_polyhash_ctx *ph)
{
    if (!ph) return;
    hb_free(&ph->st);                                            /* waits for the last call first */
    free(ph->tag_bits);
    delete ph;
}

extern "C" void qldpc_polyhash_cfg_default(qldpc_polyhash_cfg *cfg)
{
    if (!cfg) return;
    memset(cfg, 0, sizeof(*cfg));
    cfg->max_blocks = 64; cfg->max_key_bits = 1 << 16; cfg->n_keys = 1;
}

extern "C" int qldpc_polyhash_create_cfg(const qldpc_polyhash_cfg *cfg, qldpc_polyhash_ctx **out)
{
    if (!out) return QLDPC_EINVAL;
    *out = nullptr;
    if (!cfg) return QLDPC_EINVAL;
    if (cfg->n_keys < 1 || cfg->n_keys > PH_MAX_KEYS) { qldpc_set_error("polyhash_create_cfg: n_keys=%d (1 .. %d)", cfg->n_keys, PH_MAX_KEYS); return QLDPC_EINVAL; }
    const uint32_t tile = ph_tile_words(cfg->tile_words);
    if (!tile) { qldpc_set_error("polyhash_create_cfg: tile_words=%d (0, %d or %d)", cfg->tile_words, PH_TILE_WORDS, PH_TILE_WORDS_SMALL); return QLDPC_EINVAL; }
    qldpc_polyhash_ctx *ph = new (std::nothrow) qldpc_polyhash_ctx();
    if (!ph) return QLDPC_ENOMEM;
    ph->n_keys = cfg->n_keys; ph->tile = tile;
    const hb_limits lim = {cfg->max_blocks, cfg->max_key_bits, 64 * cfg->n_keys};
    int rc = hb_create(&ph->st, cfg->device, &lim, ph_desc_words(1), 2u * (uint32_t)cfg->n_keys, "polyhash_create", &ph_names);
    if (!rc) {
        ph->max_tiles = ph_tiles(ph_coefs(lim.max_key_bits), tile);
        const size_t parts = (size_t)lim.max_blocks * ph->max_tiles * (size_t)cfg->n_keys;
        ph->tag_bits = (int *)malloc(sizeof(int) * (size_t)lim.max_blocks);
        if (!ph->tag_bits || dm_alloc(&ph->st.mem, &ph->d_parts, parts)) rc = QLDPC_ENOMEM;
        else for (int i = 0; i < lim.max_blocks; i++) ph->tag_bits[i] = lim.max_out_bits;
    }
    if (rc) { qldpc_polyhash_free(ph); return rc; }
    *out = ph;
    return QLDPC_OK;
}

extern "C" size_t qldpc_polyhash_device_bytes(const qldpc_polyhash_ctx *ph) { return ph ? ph->st.mem.dev_bytes : 0; }

/* the layout of the call as descriptor rows into the pinned staging -> the tiles of its longest block.  strides NULL: the host form
   (one_key: every block reads the hash key at 0) */
static uint32_t ph_fill(qldpc_polyhash_ctx *ph, int n, const int *key_bits, const hb_strides *strides, int one_key, hb_sums *sums)
{
    const hb_row *rows = ph->st.rows;
    *sums = hb_layout(n, key_bits, ph->tag_bits, ph_hkey_words, strides, one_key, ph->st.rows);
    ph_desc *descs = (ph_desc *)ph->st.h_in;
    uint32_t widest = 0;
    uint64_t part_off = 0;
    for (int i = 0; i < n; i++) {
        const uint32_t tiles = ph_tiles(ph_coefs(key_bits[i]), ph->tile);
        descs[i] = ph_desc{rows[i].key_words, hb_tail_mask(key_bits[i]), (uint32_t)key_bits[i], tiles, rows[i].key_off, rows[i].extra_off, rows[i].out_off, part_off};
        part_off += (uint64_t)tiles * (uint64_t)ph->n_keys;       /* tiles <= max_tiles: inside the work area */
        if (tiles > widest) widest = tiles;
    }
    return widest;
}

template <int NK>
static void ph_launch_nk(const qldpc_polyhash_ctx *ph, int n, uint32_t widest, const uint32_t *d_keys, const uint32_t *d_hkeys, uint32_t *d_out, hipStream_t s)
{
    const ph_desc *descs = (const ph_desc *)ph->st.d_in;
    hipLaunchKernelGGL(ph_hash<NK>, dim3(widest, (unsigned)n), dim3(PH_LANES), 0, s, descs, d_keys, d_hkeys, d_out, ph->d_parts, ph->tile);
    if (widest > 1u) hipLaunchKernelGGL(ph_fold_tiles<NK>, dim3((unsigned)n), dim3(PH_LANES), 0, s, descs, d_hkeys, d_out, (const uint64_t *)ph->d_parts, ph->tile);
}

/* the blocks of a call, laid out by ph_fill; widest: the tiles of the call's longest block */
static int ph_launch(qldpc_polyhash_ctx *ph, int n, uint32_t widest, const uint32_t *d_keys, const uint32_t *d_hkeys, uint32_t *d_out, hipStream_t s)
{
    switch (ph->n_keys) {
    case 1: ph_launch_nk<1>(ph, n, widest, d_keys, d_hkeys, d_out, s); break;
    case 2: ph_launch_nk<2>(ph, n, widest, d_keys, d_hkeys, d_out, s); break;
    case 3: ph_launch_nk<3>(ph, n, widest, d_keys, d_hkeys, d_out, s); break;
    default: ph_launch_nk<4>(ph, n, widest, d_keys, d_hkeys, d_out, s); break;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { qldpc_set_error("polyhash_blocks launch: %s", hipGetErrorString(e)); return QLDPC_EHIP; }
    return QLDPC_OK;
}

extern "C" int qldpc_polyhash_blocks(qldpc_polyhash_ctx *ph, int n, const uint32_t *const *key_words, const int *key_bits,
                                     const uint32_t *const *hash_keys, uint32_t *const *tag_words)
{
    int rc = ph ? hb_check_blocks(&ph->st.lim, n, key_bits, ph->tag_bits, 0, "polyhash_blocks", &ph_names) : QLDPC_EINVAL;
    if (rc || n == 0) return rc;
    if (!key_words || !hash_keys || !tag_words) { qldpc_set_error("polyhash_blocks: NULL argument array"); return QLDPC_EINVAL; }
    hb_stage *st = &ph->st;
    if ((rc = hb_check_rows(n, ph->tag_bits, key_words, hash_keys, tag_words, "polyhash_blocks")) || (rc = hb_begin(st))) return rc;
    int one_key = 1;
    for (int i = 1; i < n; i++)
        if (hash_keys[i] != hash_keys[0]) one_key = 0;
    hb_sums sums;
    const uint32_t widest = ph_fill(ph, n, key_bits, nullptr, one_key, &sums);
    const size_t head = ph_desc_words(n), kw = sums.key_words, hw = sums.extra_words;
    uint32_t *h_hkeys = st->h_in + head + kw;
    if (one_key) memcpy(h_hkeys, hash_keys[0], 4 * hw);
    else for (int i = 0; i < n; i++) memcpy(h_hkeys + st->rows[i].extra_off, hash_keys[i], 4 * (size_t)st->rows[i].extra_words);
    return hb_run_host(st, n, key_words, st->h_in + head, head + kw + hw, sums.out_words, tag_words, [&](hipStream_t s) {
        return ph_launch(ph, n, widest, st->d_in + head, st->d_in + head + kw, st->d_out, s);
    });
}

extern "C" int qldpc_polyhash_blocks_dev(qldpc_polyhash_ctx *ph, int n, const uint32_t *d_keys, size_t key_stride, const int *key_bits,
                                         const uint32_t *d_hash_keys, size_t hash_key_stride, uint32_t *d_tags, size_t tag_stride, void *hip_stream)
{
    int rc = ph ? hb_check_blocks(&ph->st.lim, n, key_bits, ph->tag_bits, 0, "polyhash_blocks_dev", &ph_names) : QLDPC_EINVAL;
    if (rc || n == 0) return rc;
    if (!d_keys || !d_hash_keys || !d_tags) { qldpc_set_error("polyhash_blocks_dev: NULL device pointer"); return QLDPC_EINVAL; }
    const hb_strides strides = {key_stride, tag_stride, hash_key_stride};
    if ((rc = hb_check_strides(n, key_bits, ph->tag_bits, ph_hkey_words, &strides, "polyhash_blocks_dev", &ph_names)) || (rc = hb_begin(&ph->st))) return rc;
    hb_sums sums;
    const uint32_t widest = ph_fill(ph, n, key_bits, &strides, 0, &sums);
    return hb_run_dev(&ph->st, ph_desc_words(n), (hipStream_t)hip_stream, [&](hipStream_t s) {
        return ph_launch(ph, n, widest, d_keys, d_hash_keys, d_tags, s);
    });
}
