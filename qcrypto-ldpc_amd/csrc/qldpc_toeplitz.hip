/*
 * qldpc_toeplitz.hip -- Toeplitz-hash privacy amplification for a batch of blocks in one launch (qldpc_toeplitz_*).
 *
 *     y_i = XOR_{j < n} x_j t_{i+j},    i < m,    seed t of n + m - 1 bits
 *
 * an n x m GF(2) matrix-vector product per block, with no shortcut: every output bit reads the whole key (that is what makes the
 * family 2-universal, and what the LFSR hash of qldpc_privamp* lacks).  In words, with W(p) the 32 seed bits from bit p on,
 * y_i = parity(XOR_j key[j] & W(i + 32 j)).  The arithmetic is qldpc_toeplitz_core.h (bit-reversed words: one funnel shift per window).
 *
 * tz_hash: grid = (4 x groups of 32 output words, blocks), 256 lanes = 8 halves of 32 lanes.  Half h of workgroup (C, r) owns output word
 *     32 C + 4 h + r, lane s of it output bit s of that word.  All halves of a workgroup meet key word j in the same step, so key[j] is
 *     wave-uniform (scalar loads, bit-reversed on the scalar unit), and half h is then at seed word 32 C + r + 4 h + j: the halves lie
 *     4 words = 16 bytes apart in the staged seed, so each lane takes the next 4 seed words with one aligned 16-byte LDS read (a
 *     broadcast inside a half) and rolls its window through them, one funnel shift per key word.  That alignment is why a workgroup owns
 *     every 4th word (r) and not 8 adjacent ones.
 *     The seed words a workgroup needs for TZ_TILE key words (TZ_TILE + 32) are staged bit-reversed in LDS, tile after tile: neither the
 *     key nor the seed is bounded by the LDS.  The output word of a half is its 32 parities by ballot.
 */
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <new>

#include "qldpc_hip.h"
#include "qldpc_toeplitz_core.h"
#include "qldpc_toeplitz_int.h"

#define TZ_LANES 256
#define TZ_TILE 2048               /* key words per staged seed tile; a multiple of 8 */
#define TZ_SPAN 32                 /* seed words past the tile that the 8 halves of a workgroup reach (28 + 1, and 3 of padding in front) */

__global__ __launch_bounds__(TZ_LANES) void tz_hash(const tz_desc *__restrict__ descs, const uint32_t *__restrict__ keys,
                                                    const uint32_t *__restrict__ seeds, uint32_t *__restrict__ outs)
{
    /* s_w[x] = bit-reversed seed word (w0 + j0 + x - 3): the 4 words after a half's current one start at a multiple of 4 */
    __shared__ uint4 s_seed[(TZ_TILE + TZ_SPAN) / 4];
    uint32_t *s_w = (uint32_t *)s_seed;
    const tz_desc d = descs[blockIdx.y];
    const uint32_t outwords = (d.out_bits + 31u) / 32u;
    const uint32_t w0 = (blockIdx.x >> 2) * 32u + (blockIdx.x & 3u);
    if (w0 >= outwords) return;                                 /* the whole workgroup: the grid is as wide as the call's longest output */
    const uint32_t t = threadIdx.x, h = t >> 5, s = t & 31u;
    const uint32_t word = w0 + 4u * h;
    const bool wave_on = (uint32_t)__builtin_amdgcn_readfirstlane((int)word) < outwords;      /* the wave's first half */
    const uint32_t *__restrict__ key = keys + d.key_off;
    const uint32_t *__restrict__ seed = seeds + d.seed_off;
    const uint32_t last = d.key_words - 1u;
    uint32_t acc = 0;
    for (uint32_t j0 = 0; j0 < d.key_words; j0 += TZ_TILE) {
        const uint32_t tw = min((uint32_t)TZ_TILE, d.key_words - j0);
        if (j0) __syncthreads();
        for (uint32_t x = t; x < tw + TZ_SPAN; x += TZ_LANES) {
            const uint64_t g = (uint64_t)w0 + j0 + x - 3u;
            s_w[x] = (x >= 3u && g < d.seed_words) ? tz_brev(seed[g]) : 0u;      /* past the block's seed: met by masked key bits or by lanes past out_bits only */
        }
        __syncthreads();
        if (!wave_on) continue;
        /* groups of 8 key words; the key's last word goes through the masked loop */
        const uint32_t full = j0 + tw == d.key_words ? (tw - 1u) & ~7u : tw;
        uint32_t lo = s_w[4u * h + 3u];
        const uint4 *quad = s_seed + h + 1u;
        for (uint32_t jj = 0; jj < full; jj += 8u) {
            const uint4 a = quad[jj >> 2], b = quad[(jj >> 2) + 1u];
            const uint32_t *k = key + j0 + jj;
            acc = tz_fold(acc, tz_brev(k[0]), tz_window(lo, a.x, s));
            acc = tz_fold(acc, tz_brev(k[1]), tz_window(a.x, a.y, s));
            acc = tz_fold(acc, tz_brev(k[2]), tz_window(a.y, a.z, s));
            acc = tz_fold(acc, tz_brev(k[3]), tz_window(a.z, a.w, s));
            acc = tz_fold(acc, tz_brev(k[4]), tz_window(a.w, b.x, s));
            acc = tz_fold(acc, tz_brev(k[5]), tz_window(b.x, b.y, s));
            acc = tz_fold(acc, tz_brev(k[6]), tz_window(b.y, b.z, s));
            acc = tz_fold(acc, tz_brev(k[7]), tz_window(b.z, b.w, s));
            lo = b.w;
        }
        acc = tz_lane_words(acc, key, j0 + full, tw - full, last, d.tail_mask, s_w + 4u * h + 3u + full, s);
    }
    if (!wave_on) return;
    const unsigned long long votes = __ballot(32u * word + s < d.out_bits && tz_parity(acc));
    if (s == 0 && word < outwords) outs[d.out_off + word] = tz_brev((uint32_t)(votes >> (t & 32u)));
}

/* ------------------------------------------------------------------ host ---- */

/* host mirror: every output bit through tz_lane_words, the key in tiles of tile_words, the seed window rebuilt per tile as the kernel stages it */
extern "C" int qldpc_toeplitz_host(const uint32_t *key_words, int key_bits, const uint32_t *seed_words, int out_bits, int tile_words, uint32_t *out_words)
{
    if (key_bits <= 0 || out_bits < 0 || key_bits > TZ_MAX_BITS || out_bits > TZ_MAX_BITS || tile_words < 0) {
        qldpc_set_error("toeplitz_host: key_bits=%d out_bits=%d tile_words=%d", key_bits, out_bits, tile_words);
        return QLDPC_ESIZE;
    }
    if (out_bits == 0) return QLDPC_OK;
    if (!key_words || !seed_words || !out_words) return QLDPC_EINVAL;
    const uint32_t nw = ((uint32_t)key_bits + 31u) / 32u, ow = ((uint32_t)out_bits + 31u) / 32u, sw = tz_seed_words(key_bits, out_bits);
    const uint32_t tile = tile_words ? (uint32_t)tile_words : (uint32_t)TZ_TILE, mask = hb_tail_mask(key_bits);
    uint32_t *win = (uint32_t *)malloc(4 * ((size_t)(tile < nw ? tile : nw) + 1));
    if (!win) return QLDPC_ENOMEM;
    for (uint32_t w = 0; w < ow; w++) {
        uint32_t acc[32];
        memset(acc, 0, sizeof(acc));
        for (uint32_t j0 = 0; j0 < nw; j0 += tile) {
            const uint32_t tw = nw - j0 < tile ? nw - j0 : tile;
            for (uint32_t k = 0; k <= tw; k++) win[k] = w + j0 + k < sw ? tz_brev(seed_words[w + j0 + k]) : 0u;
            for (uint32_t s = 0; s < 32; s++) acc[s] = tz_lane_words(acc[s], key_words, j0, tw, nw - 1u, mask, win, s);
        }
        uint32_t word = 0;
        for (uint32_t s = 0; s < 32; s++)
            if (32u * w + s < (uint32_t)out_bits) word |= tz_parity(acc[s]) << (31 - s);
        out_words[w] = word;
    }
    free(win);
    return QLDPC_OK;
}

extern "C" size_t qldpc_toeplitz_seed_words(int key_bits, int out_bits) { return tz_seed_words(key_bits, out_bits); }

static const hb_names tz_names = {"key_bits", "out_bits"};
static size_t tz_desc_words(int n) { return (size_t)n * (sizeof(tz_desc) / 4); }

extern "C" void qldpc_toeplitz_free(qldpc_toeplitz_ctx *tz)
{
    if (!tz) return;
    hb_free(&tz->st);                                            /* waits for the last call first; the NTT state's device memory goes with the ledger */
    tzn_free(tz);
    delete tz;
}

extern "C" void qldpc_toeplitz_cfg_default(qldpc_toeplitz_cfg *cfg)
{
    if (!cfg) return;
    memset(cfg, 0, sizeof(*cfg));
    cfg->max_blocks = 64; cfg->max_key_bits = 1 << 16; cfg->max_out_bits = 1 << 16;
    cfg->method = QLDPC_TOEPLITZ_DIRECT;
}

extern "C" int qldpc_toeplitz_create_cfg(const qldpc_toeplitz_cfg *cfg, qldpc_toeplitz_ctx **out)
{
    if (!out) return QLDPC_EINVAL;
    *out = nullptr;
    if (!cfg) return QLDPC_EINVAL;
    if (cfg->method != QLDPC_TOEPLITZ_DIRECT && cfg->method != QLDPC_TOEPLITZ_NTT) { qldpc_set_error("toeplitz_create_cfg: method=%d", cfg->method); return QLDPC_EINVAL; }
    if (cfg->pass_log2 != 0 && cfg->pass_log2 != QLDPC_TOEPLITZ_PASS_LOG2_SMALL) {
        qldpc_set_error("toeplitz_create_cfg: pass_log2=%d (0 or %d)", cfg->pass_log2, QLDPC_TOEPLITZ_PASS_LOG2_SMALL);
        return QLDPC_EINVAL;
    }
    qldpc_toeplitz_ctx *tz = new (std::nothrow) qldpc_toeplitz_ctx();
    if (!tz) return QLDPC_ENOMEM;
    tz->method = cfg->method;
    const hb_limits lim = {cfg->max_blocks, cfg->max_key_bits, cfg->max_out_bits};
    int rc = hb_create(&tz->st, cfg->device, &lim, tz_desc_words(1), tz_seed_words(lim.max_key_bits, lim.max_out_bits), "toeplitz_create", &tz_names);
    if (!rc && tz->method == QLDPC_TOEPLITZ_NTT) rc = tzn_create(tz, cfg->pass_log2, cfg->work_bytes);
    if (rc) { qldpc_toeplitz_free(tz); return rc; }
    *out = tz;
    return QLDPC_OK;
}

extern "C" int qldpc_toeplitz_create(int device, int max_blocks, int max_key_bits, int max_out_bits, qldpc_toeplitz_ctx **out)
{
    qldpc_toeplitz_cfg cfg;
    qldpc_toeplitz_cfg_default(&cfg);
    cfg.device = device; cfg.max_blocks = max_blocks; cfg.max_key_bits = max_key_bits; cfg.max_out_bits = max_out_bits;
    return qldpc_toeplitz_create_cfg(&cfg, out);
}

extern "C" int qldpc_toeplitz_stats(const qldpc_toeplitz_ctx *tz, uint64_t out[8])
{
    if (!tz || !out) return QLDPC_EINVAL;
    memcpy(out, tz->stats, sizeof(tz->stats));
    return QLDPC_OK;
}

extern "C" size_t qldpc_toeplitz_device_bytes(const qldpc_toeplitz_ctx *tz) { return tz ? tz->st.mem.dev_bytes : 0; }

/* the layout of the call as descriptor rows into the pinned staging.  strides NULL: the host form (one_seed: every block reads the seed at 0) */
static hb_sums tz_fill(qldpc_toeplitz_ctx *tz, int n, const int *key_bits, const int *out_bits, const hb_strides *strides, int one_seed)
{
    const hb_row *rows = tz->st.rows;
    const hb_sums sums = hb_layout(n, key_bits, out_bits, tz_seed_words, strides, one_seed, tz->st.rows);
    tz_desc *descs = (tz_desc *)tz->st.h_in;
    for (int i = 0; i < n; i++)
        descs[i] = tz_desc{rows[i].key_words, hb_tail_mask(key_bits[i]), (uint32_t)out_bits[i], rows[i].extra_words, rows[i].key_off, rows[i].extra_off, rows[i].out_off};
    return sums;
}

/* the blocks of a call, laid out by tz_fill, by the context's method; widest: the words of the call's longest output row, > 0; shared: one seed row */
static int tz_launch(qldpc_toeplitz_ctx *tz, int n, uint32_t widest, const int *key_bits, int shared, const uint32_t *d_keys, const uint32_t *d_seeds, uint32_t *d_out, hipStream_t s)
{
    if (tz->method == QLDPC_TOEPLITZ_NTT) return tzn_blocks(tz, n, (const tz_desc *)tz->st.h_in, key_bits, shared, d_keys, d_seeds, d_out, s);
    memset(tz->stats, 0, sizeof(tz->stats));
    tz->stats[0] = 1;
    hipLaunchKernelGGL(tz_hash, dim3(4u * ((widest + 31u) / 32u), (unsigned)n), dim3(TZ_LANES), 0, s, (const tz_desc *)tz->st.d_in, d_keys, d_seeds, d_out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) { qldpc_set_error("toeplitz_blocks launch: %s", hipGetErrorString(e)); return QLDPC_EHIP; }
    return QLDPC_OK;
}

extern "C" int qldpc_toeplitz_blocks(qldpc_toeplitz_ctx *tz, int n, const uint32_t *const *key_words, const int *key_bits,
                                     const uint32_t *const *seed_words, const int *out_bits, uint32_t *const *out_words)
{
    int rc = tz ? hb_check_blocks(&tz->st.lim, n, key_bits, out_bits, 0, "toeplitz_blocks", &tz_names) : QLDPC_EINVAL;
    if (rc || n == 0) return rc;
    if (!key_words || !seed_words || !out_words) { qldpc_set_error("toeplitz_blocks: NULL argument array"); return QLDPC_EINVAL; }
    hb_stage *st = &tz->st;
    if ((rc = hb_check_rows(n, out_bits, key_words, seed_words, out_words, "toeplitz_blocks")) || (rc = hb_begin(st))) return rc;
    int one_seed = 1;
    for (int i = 1; i < n; i++)
        if (seed_words[i] != seed_words[0]) one_seed = 0;
    const hb_sums sums = tz_fill(tz, n, key_bits, out_bits, nullptr, one_seed);
    if (sums.widest_out == 0) return QLDPC_OK;                   /* every block asks for 0 bits */
    const size_t head = tz_desc_words(n), kw = sums.key_words, sw = sums.extra_words;
    uint32_t *h_seeds = st->h_in + head + kw;
    if (one_seed) memcpy(h_seeds, seed_words[0], 4 * sw);        /* the caller's one row covers the longest key_bits + out_bits - 1 of the call */
    else for (int i = 0; i < n; i++) memcpy(h_seeds + st->rows[i].extra_off, seed_words[i], 4 * (size_t)st->rows[i].extra_words);
    return hb_run_host(st, n, key_words, st->h_in + head, head + kw + sw, sums.out_words, out_words, [&](hipStream_t s) {
        return tz_launch(tz, n, sums.widest_out, key_bits, one_seed, st->d_in + head, st->d_in + head + kw, st->d_out, s);
    });
}

extern "C" int qldpc_toeplitz_blocks_dev(qldpc_toeplitz_ctx *tz, int n, const uint32_t *d_keys, size_t key_stride, const int *key_bits,
                                         const uint32_t *d_seeds, size_t seed_stride, const int *out_bits,
                                         uint32_t *d_out, size_t out_stride, void *hip_stream)
{
    int rc = tz ? hb_check_blocks(&tz->st.lim, n, key_bits, out_bits, 0, "toeplitz_blocks_dev", &tz_names) : QLDPC_EINVAL;
    if (rc || n == 0) return rc;
    if (!d_keys || !d_seeds || !d_out) { qldpc_set_error("toeplitz_blocks_dev: NULL device pointer"); return QLDPC_EINVAL; }
    const hb_strides strides = {key_stride, out_stride, seed_stride};
    if ((rc = hb_check_strides(n, key_bits, out_bits, tz_seed_words, &strides, "toeplitz_blocks_dev", &tz_names)) || (rc = hb_begin(&tz->st))) return rc;
    const hb_sums sums = tz_fill(tz, n, key_bits, out_bits, &strides, 0);
    if (sums.widest_out == 0) return QLDPC_OK;
    /* the NTT method reads the rows on the host and uploads rows of its own */
    return hb_run_dev(&tz->st, tz->method == QLDPC_TOEPLITZ_DIRECT ? tz_desc_words(n) : 0, (hipStream_t)hip_stream, [&](hipStream_t s) {
        return tz_launch(tz, n, sums.widest_out, key_bits, seed_stride == 0, d_keys, d_seeds, d_out, s);
    });
}
