/*
 * qldpc_mc.hip -- the Monte-Carlo loop of the reference harness (source -> encoder -> BSC -> decoder -> monitor, BS/src/main.cpp:335-393)
 * with nothing per bit crossing the host (qldpc_mc_*).  The frame definition is qldpc_mc_core.h: frame i is a pure function of (seed, i).
 *
 * mc_source:  one lane per info word of the packed [frame][word] layout, consecutive lanes = consecutive words of a row (the last lanes of a
 *     row run on into the next one), one Philox call per word.
 * mc_channel: one lane per codeword word: 8 Philox calls, the 32 classes of the word by two 16-byte loads from the padded class map (32 N
 *     bytes shared by all frames: L2-resident), the two thresholds wave-uniform kernel arguments; rx = cw ^ flips.  The lanes of word 0 also
 *     write the frame's |LLR| for qldpc_load_bits_dev.
 * mc_soft_channel: the quantised soft-output channel of a threshold table (qldpc_mc_core.h), one lane per four VNs: one Philox call, one class
 *     word, both threshold rows and the value row in LDS (3 KB, loaded once per workgroup), a halving search per VN, one 16-byte store of the
 *     four LLRs where the address allows it (scalars where N % 4 != 0 shifts a row or cuts its last quad); the rx word = the OR of the flip
 *     nibbles of the 8 lanes of a codeword word by xor-shuffles, stored by the first of them.  No atomics, no floating-point arithmetic.
 * mc_monitor: one wave per frame (a wave strides over the frames): be = popcount((out ^ cw) & info_mask) and the flips at channel VNs summed
 *     over the lanes by shuffles, the per-frame verdicts summed in (wave-uniform) registers over the wave's frames, then ONE atomicAdd per
 *     wave and counter from lane 0 -- plus, per frame, one on the iteration histogram and, for a failed frame, one returning add on the
 *     slot counter of the failed-frame list.
 *
 * mc_patterns: one workgroup per puncture pattern (the definition and the radix select are qldpc_mc_core.h): per key digit a histogram in LDS
 *     over keys recomputed on the fly (n_cand / 4 Philox calls per pass, nothing stored), lane 0 picks the bucket; the final pass walks the
 *     candidates in index order in chunks of 4 x 256, the rank among equal keys = a running count + a shuffle prefix over the chunk, and sets
 *     the erase bits of the row it zeroed at its start.
 * mc_expand_rows: a pattern row -> the F frame rows of its slots, the layout qldpc_load_erasures_dev reads; 16-byte stores.
 * mc_monitor_patterns: the arithmetic of mc_monitor, the waves dealt out per pattern (every frame of a wave belongs to one pattern), so ONE
 *     atomicAdd per wave and counter onto the counter row of that pattern.
 *
 * mc_source_points / mc_channel_points: the lane layouts of mc_source / mc_channel for the QBER sweep (qldpc_mc_sweep): the frame index of a slot
 *     comes from the slot table of the round instead of first + f, the channel threshold and the |LLR| of the slot from the row {threshold,
 *     |LLR|} of the slot's point (P rows of 8 bytes: L2-resident); mc_info_word and mc_flip_word unchanged, so a frame is the frame of
 *     qldpc_mc_frames_host.
 * mc_expand_points: mc_expand_rows with the erase row of a slot looked up through the slot's point.
 * mc_monitor_points: the arithmetic of mc_monitor, flips included, the waves dealt out per chunk (every frame of a wave belongs to one point):
 *     ONE atomicAdd per wave and counter onto the counter row of that point and one atomicMax for iter_max, per frame one add on the point's
 *     histogram row; no failed-frame list.
 *
 * mc_channel_weight: the fixed-weight channel of the error strata (qldpc_mc_strata, the definition is qldpc_mc_core.h), one workgroup per frame
 *     slot: per key digit a histogram in LDS over the keys of the channel-class VNs, recomputed on the fly from the padded class map (N / 4
 *     Philox calls per pass, nothing stored: at N = 65 536 the keys of a frame do not fit in LDS), lane 0 picks the bucket.  The final pass
 *     gives a lane a whole codeword word, 256 words per trip: 8 Philox calls, the 32 classes as mc_channel reads them, three masks (keys below
 *     the threshold key, keys equal to it, pinned flips); the rank of the word among equal keys = a running count + a shuffle prefix over the
 *     trip; rx = cw ^ (selected | pinned) is one plain store per word, no global atomics.  The weight, the |LLR| and the frame index of a slot
 *     come from the tables of the round ({weight, |LLR|} rows in the layout of mc_channel_points' {threshold, |LLR|}), or from the arguments
 *     for qldpc_mc_weight_frames_dev.
 *
 * No kernel waits on another wave.  The decoder and the encoder are driven through their public calls only; qldpc_engine_int.h is read for
 * the decoder's sizes, device and stream.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/qldpc.h"
#include "qldpc_engine_int.h"
#include "qldpc_mc_core.h"

#define MC_LANES 256
#define MC_MAX_WAVES 2048          /* of a monitor launch */
enum { MC_FRAMES = 0, MC_BIT_ERRORS, MC_FRAME_ERRORS, MC_UNDETECTED, MC_NOT_CONVERGED, MC_ITER_SUM, MC_ITER_MAX, MC_FLIPS, MC_CHANNEL_BITS, MC_FAIL_SLOTS,
       MC_COUNTERS };

typedef unsigned long long mc_u64;

__global__ __launch_bounds__(MC_LANES) void mc_source(uint32_t *__restrict__ info, unsigned total, unsigned Wk, int K, uint64_t seed, uint64_t first)
{
    const unsigned i = blockIdx.x * MC_LANES + threadIdx.x;
    if (i >= total) return;
    const unsigned f = i / Wk, j = i - f * Wk;
    info[i] = mc_info_word(seed, first + f, j, K);
}

__global__ __launch_bounds__(MC_LANES) void mc_channel(const uint32_t *__restrict__ cw, uint32_t *__restrict__ rx, const uint4 *__restrict__ cls,
                                                       unsigned total, unsigned Wn, uint64_t seed, uint64_t first, uint32_t t_channel, uint32_t t_pinned,
                                                       float *__restrict__ llr_mag, float mag)
{
    const unsigned i = blockIdx.x * MC_LANES + threadIdx.x;
    if (i >= total) return;
    const unsigned f = i / Wn, w = i - f * Wn;
    const uint4 a = cls[2u * w], b = cls[2u * w + 1u];
    const uint32_t cls4[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    rx[i] = cw[i] ^ mc_flip_word(seed, first + f, w, cls4, t_channel, t_pinned);
    if (w == 0 && llr_mag) llr_mag[f] = mag;
}

/* rows of 8 Wn quads (the padding past N is QLDPC_VN_PUNCTURED: LLR 0, no flip, nothing stored), total = n 8 Wn lanes: a multiple of 8, as the
 * block size is, so the 8 lanes of a codeword word leave or stay together and the shuffles below see all of them.  rx may be NULL. */
__global__ __launch_bounds__(MC_LANES) void mc_soft_channel(const uint32_t *__restrict__ cw, uint32_t *__restrict__ rx, float *__restrict__ llr,
                                                            const uint32_t *__restrict__ cls4, const mc_soft_table *__restrict__ tab, unsigned total,
                                                            unsigned Qn, unsigned N, uint64_t seed, uint64_t first, uint32_t t_pinned)
{
    static_assert(MC_LANES == MC_SOFT_MAX_LEVELS, "mc_soft_channel loads one table entry per lane");
    __shared__ uint32_t thr[2][MC_SOFT_MAX_LEVELS];
    __shared__ float value[MC_SOFT_MAX_LEVELS];
    const unsigned t = threadIdx.x;
    thr[0][t] = t < MC_SOFT_MAX_LEVELS - 1 ? tab->thr[0][t] : 0xFFFFFFFFu;
    thr[1][t] = t < MC_SOFT_MAX_LEVELS - 1 ? tab->thr[1][t] : 0xFFFFFFFFu;
    value[t] = tab->value[t];
    const uint32_t live0 = tab->live[0], live1 = tab->live[1];
    __syncthreads();
    const unsigned i = blockIdx.x * MC_LANES + t;
    if (i >= total) return;
    const unsigned f = i / Qn, q = i - f * Qn, sh = 28u - 4u * (q & 7u);
    const uint32_t c = cw[i >> 3];
    float l[4];
    uint32_t flips = mc_soft_quad(seed, first + f, q, cls4[q], (c >> sh) & 0xfu, thr[0], live0, thr[1], live1, value, t_pinned, l) << sh;
    const unsigned v = 4u * q;
    if (v < N) {
        float *p = llr + (size_t)f * N + v;
        if (v + 4u <= N && ((uintptr_t)p & 15u) == 0) *(float4 *)p = make_float4(l[0], l[1], l[2], l[3]);
        else for (unsigned b = 0; b < 4u && v + b < N; b++) p[b] = l[b];
    }
    if (!rx) return;
    for (int s = 1; s < 8; s <<= 1) flips |= (uint32_t)__shfl_xor((int)flips, s, 64);
    if ((q & 7u) == 0) rx[i >> 3] = c ^ flips;
}

__device__ static inline unsigned mc_wave_sum(unsigned x)
{
    for (int s = 32; s > 0; s >>= 1) x += __shfl_xor(x, s, 64);
    return x;
}

__global__ __launch_bounds__(MC_LANES) void mc_monitor(const uint32_t *__restrict__ out, const uint32_t *__restrict__ cw, const uint32_t *__restrict__ rx,
                                                       const uint32_t *__restrict__ info_mask, const uint32_t *__restrict__ chan_mask,
                                                       const int *__restrict__ iters, const int *__restrict__ ok, unsigned n, unsigned Wn, int n_ite,
                                                       uint64_t first, unsigned channel_vns, mc_u64 *__restrict__ ctr, mc_u64 *__restrict__ hist,
                                                       mc_u64 *__restrict__ fails, unsigned fail_cap)
{
    const unsigned lane = threadIdx.x & 63u, waves = gridDim.x * (MC_LANES / 64);
    mc_u64 s_frames = 0, s_be = 0, s_fe = 0, s_ud = 0, s_nc = 0, s_it = 0, s_mx = 0, s_fl = 0;
    for (unsigned f = blockIdx.x * (MC_LANES / 64) + (threadIdx.x >> 6); f < n; f += waves) {
        const size_t row = (size_t)f * Wn;
        unsigned be = 0, fl = 0;
        for (unsigned w = lane; w < Wn; w += 64u) {
            const uint32_t c = cw[row + w];
            be += (unsigned)__popc((out[row + w] ^ c) & info_mask[w]);
            fl += (unsigned)__popc((rx[row + w] ^ c) & chan_mask[w]);
        }
        be = mc_wave_sum(be);
        fl = mc_wave_sum(fl);
        const int it = min(max(iters[f], 0), n_ite);
        const bool good = ok[f] != 0;
        s_frames++; s_be += be; s_fl += fl; s_it += (mc_u64)it;
        s_mx = max(s_mx, (mc_u64)it);
        s_fe += be > 0; s_ud += good && be > 0; s_nc += !good;
        if (lane == 0) {
            atomicAdd(hist + it, 1ull);
            if (be > 0) {
                const mc_u64 slot = atomicAdd(ctr + MC_FAIL_SLOTS, 1ull);
                if (slot < fail_cap) fails[slot] = first + f;
            }
        }
    }
    if (lane != 0 || s_frames == 0) return;
    atomicAdd(ctr + MC_FRAMES, s_frames);
    atomicAdd(ctr + MC_ITER_SUM, s_it);
    atomicMax(ctr + MC_ITER_MAX, s_mx);
    atomicAdd(ctr + MC_CHANNEL_BITS, s_frames * channel_vns);
    if (s_fl) atomicAdd(ctr + MC_FLIPS, s_fl);
    if (s_be) atomicAdd(ctr + MC_BIT_ERRORS, s_be);
    if (s_fe) atomicAdd(ctr + MC_FRAME_ERRORS, s_fe);
    if (s_ud) atomicAdd(ctr + MC_UNDETECTED, s_ud);
    if (s_nc) atomicAdd(ctr + MC_NOT_CONVERGED, s_nc);
}

/* ---- puncture patterns ---- */
#define MC_PAT_LANES 256
static_assert(MC_PAT_LANES == MC_SEL_BINS, "mc_patterns clears one histogram bin per lane");
enum { MCP_FRAMES = 0, MCP_FRAME_ERRORS, MCP_BIT_ERRORS, MCP_UNDETECTED, MCP_NOT_CONVERGED, MCP_ITER_SUM, MCP_COUNTERS };

/* rows[blockIdx.x][Wn] = the erase row of pattern first + blockIdx.x; cand[n_cand] ascending VNs below 32 Wn; n_punct <= n_cand; key_bits 1 .. 32 */
__global__ __launch_bounds__(MC_PAT_LANES) void mc_patterns(uint32_t *__restrict__ rows, const int *__restrict__ cand, unsigned n_cand, unsigned n_punct,
                                                            int key_bits, unsigned Wn, uint64_t seed, uint64_t first)
{
    __shared__ uint32_t hist[MC_SEL_BINS];
    __shared__ uint32_t sel[2];
    __shared__ unsigned wave_eq[MC_PAT_LANES / 64];
    const unsigned t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const uint64_t p = first + blockIdx.x;
    uint32_t *row = rows + (size_t)blockIdx.x * Wn;
    for (unsigned w = t; w < Wn; w += MC_PAT_LANES) row[w] = 0u;
    if (n_punct == 0) return;
    const unsigned blocks = (n_cand + 3u) / 4u;
    uint32_t prefix = 0, mask = 0, k = n_punct, u[4];
    for (int shift = mc_select_top_shift(key_bits); shift >= 0; shift -= MC_SEL_BITS) {
        hist[t] = 0u;
        __syncthreads();
        for (unsigned q = t; q < blocks; q += MC_PAT_LANES) {
            mc_pattern_keys(seed, p, q, key_bits, u);
            for (unsigned b = 0; b < 4; b++)
                if (4u * q + b < n_cand && (u[b] & mask) == prefix) atomicAdd(&hist[(u[b] >> shift) & (MC_SEL_BINS - 1)], 1u);
        }
        __syncthreads();
        if (t == 0) { uint32_t kk = k; sel[0] = mc_select_digit(hist, &kk); sel[1] = kk; }
        __syncthreads();
        prefix |= sel[0] << shift; k = sel[1];
        mask |= (uint32_t)(MC_SEL_BINS - 1) << shift;
    }
    /* T = prefix, r = k.  The barriers above also order the zeroing of the row before the bits set below. */
    unsigned equal_base = 0;
    for (unsigned q0 = 0; q0 < blocks; q0 += MC_PAT_LANES) {
        const unsigned q = q0 + t;
        unsigned mine = 0;
        if (q < blocks) {
            mc_pattern_keys(seed, p, q, key_bits, u);
            for (unsigned b = 0; b < 4; b++) mine += 4u * q + b < n_cand && u[b] == prefix;
        }
        unsigned incl = mine;
        for (unsigned s = 1; s < 64u; s <<= 1) { const unsigned v = __shfl_up(incl, s, 64); if (lane >= s) incl += v; }
        if (lane == 63u) wave_eq[wave] = incl;
        __syncthreads();
        unsigned before = equal_base + incl - mine;
        for (unsigned w = 0; w < MC_PAT_LANES / 64; w++) { if (w < wave) before += wave_eq[w]; equal_base += wave_eq[w]; }
        if (q < blocks)
            for (unsigned b = 0; b < 4; b++) {
                if (4u * q + b >= n_cand) break;
                if (mc_pattern_takes(u[b], prefix, k, before)) { const unsigned v = (unsigned)cand[4u * q + b]; atomicOr(&row[v >> 5], 0x80000000u >> (v & 31u)); }
                before += u[b] == prefix;
            }
        __syncthreads();
    }
}

/* frames[slot][Wn] = pat[slot / F][Wn] for the `total` words of the slots, four words per lane */
__global__ __launch_bounds__(MC_LANES) void mc_expand_rows(const uint32_t *__restrict__ pat, uint32_t *__restrict__ frames, unsigned total, unsigned Wn, unsigned F)
{
    const unsigned i = (blockIdx.x * MC_LANES + threadIdx.x) * 4u;
    if (i >= total) return;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    for (unsigned j = 0; j < 4; j++)
        if (i + j < total) { const unsigned slot = (i + j) / Wn, word = (i + j) - slot * Wn; w[j] = pat[(size_t)(slot / F) * Wn + word]; }
    if (i + 4u <= total) *(uint4 *)(frames + i) = make_uint4(w[0], w[1], w[2], w[3]);
    else for (unsigned j = 0; i + j < total; j++) frames[i + j] = w[j];
}

/* wpp waves per pattern (<= F): wave (pat, sub) takes frames sub, sub + wpp, ... of the F frames of pattern slot pat */
__global__ __launch_bounds__(MC_LANES) void mc_monitor_patterns(const uint32_t *__restrict__ out, const uint32_t *__restrict__ cw, const uint32_t *__restrict__ info_mask,
                                                                const int *__restrict__ iters, const int *__restrict__ ok, unsigned n_pat, unsigned F, unsigned wpp,
                                                                unsigned Wn, int n_ite, mc_u64 *__restrict__ rows)
{
    const unsigned lane = threadIdx.x & 63u, wid = blockIdx.x * (MC_LANES / 64) + (threadIdx.x >> 6);
    if (wid >= n_pat * wpp) return;
    const unsigned pat = wid / wpp, sub = wid - pat * wpp;
    mc_u64 s_frames = 0, s_be = 0, s_fe = 0, s_ud = 0, s_nc = 0, s_it = 0;
    for (unsigned k = sub; k < F; k += wpp) {
        const unsigned f = pat * F + k;
        const size_t row = (size_t)f * Wn;
        unsigned be = 0;
        for (unsigned w = lane; w < Wn; w += 64u) be += (unsigned)__popc((out[row + w] ^ cw[row + w]) & info_mask[w]);
        be = mc_wave_sum(be);
        const int it = min(max(iters[f], 0), n_ite);
        const bool good = ok[f] != 0;
        s_frames++; s_be += be; s_it += (mc_u64)it;
        s_fe += be > 0; s_ud += good && be > 0; s_nc += !good;
    }
    if (lane != 0 || s_frames == 0) return;
    mc_u64 *r = rows + (size_t)pat * MCP_COUNTERS;
    atomicAdd(r + MCP_FRAMES, s_frames);
    atomicAdd(r + MCP_ITER_SUM, s_it);
    if (s_be) atomicAdd(r + MCP_BIT_ERRORS, s_be);
    if (s_fe) atomicAdd(r + MCP_FRAME_ERRORS, s_fe);
    if (s_ud) atomicAdd(r + MCP_UNDETECTED, s_ud);
    if (s_nc) atomicAdd(r + MCP_NOT_CONVERGED, s_nc);
}

/* ---- QBER sweep: operating points side by side in one batch ---- */
struct mc_point_row { uint32_t t_channel; float mag; };      /* of a point: floor(qber 2^32), qldpc_bsc_llr(qber) */
#define MCW_COUNTERS MC_FAIL_SLOTS                            /* a point's counter row: MC_FRAMES .. MC_CHANNEL_BITS */

__global__ __launch_bounds__(MC_LANES) void mc_source_points(uint32_t *__restrict__ info, unsigned total, unsigned Wk, int K, uint64_t seed,
                                                             const uint64_t *__restrict__ slot_frame)
{
    const unsigned i = blockIdx.x * MC_LANES + threadIdx.x;
    if (i >= total) return;
    const unsigned f = i / Wk, j = i - f * Wk;
    info[i] = mc_info_word(seed, slot_frame[f], j, K);
}

__global__ __launch_bounds__(MC_LANES) void mc_channel_points(const uint32_t *__restrict__ cw, uint32_t *__restrict__ rx, const uint4 *__restrict__ cls,
                                                              unsigned total, unsigned Wn, uint64_t seed, const uint64_t *__restrict__ slot_frame,
                                                              const uint32_t *__restrict__ slot_point, const mc_point_row *__restrict__ points,
                                                              uint32_t t_pinned, float *__restrict__ llr_mag)
{
    const unsigned i = blockIdx.x * MC_LANES + threadIdx.x;
    if (i >= total) return;
    const unsigned f = i / Wn, w = i - f * Wn;
    const mc_point_row pt = points[slot_point[f]];
    const uint4 a = cls[2u * w], b = cls[2u * w + 1u];
    const uint32_t cls4[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    rx[i] = cw[i] ^ mc_flip_word(seed, slot_frame[f], w, cls4, pt.t_channel, t_pinned);
    if (w == 0) llr_mag[f] = pt.mag;
}

/* frames[slot][Wn] = rows[slot_point[slot]][Wn] for the `total` words of the slots, four words per lane */
__global__ __launch_bounds__(MC_LANES) void mc_expand_points(const uint32_t *__restrict__ rows, uint32_t *__restrict__ frames, unsigned total, unsigned Wn,
                                                             const uint32_t *__restrict__ slot_point)
{
    const unsigned i = (blockIdx.x * MC_LANES + threadIdx.x) * 4u;
    if (i >= total) return;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    for (unsigned j = 0; j < 4; j++)
        if (i + j < total) { const unsigned slot = (i + j) / Wn, word = (i + j) - slot * Wn; w[j] = rows[(size_t)slot_point[slot] * Wn + word]; }
    if (i + 4u <= total) *(uint4 *)(frames + i) = make_uint4(w[0], w[1], w[2], w[3]);
    else for (unsigned j = 0; i + j < total; j++) frames[i + j] = w[j];
}

/* wpc waves per chunk: wave (chunk, sub) takes frames sub, sub + wpc, ... of the chunk_len frames that start at slot chunk_start; a chunk
 * belongs to one point, whose counter row [MCW_COUNTERS] and histogram row [n_ite + 1] the wave adds to */
__global__ __launch_bounds__(MC_LANES) void mc_monitor_points(const uint32_t *__restrict__ out, const uint32_t *__restrict__ cw, const uint32_t *__restrict__ rx,
                                                              const uint32_t *__restrict__ info_mask, const uint32_t *__restrict__ chan_mask,
                                                              const int *__restrict__ iters, const int *__restrict__ ok, unsigned n_chunks, unsigned wpc,
                                                              const uint32_t *__restrict__ chunk_point, const uint32_t *__restrict__ chunk_start,
                                                              const uint32_t *__restrict__ chunk_len, unsigned Wn, int n_ite, unsigned channel_vns,
                                                              mc_u64 *__restrict__ rows, mc_u64 *__restrict__ hists)
{
    const unsigned lane = threadIdx.x & 63u, wid = blockIdx.x * (MC_LANES / 64) + (threadIdx.x >> 6);
    if (wid >= n_chunks * wpc) return;
    const unsigned c = wid / wpc, sub = wid - c * wpc, point = chunk_point[c], start = chunk_start[c], len = chunk_len[c];
    mc_u64 *hist = hists + (size_t)point * (size_t)(n_ite + 1);
    mc_u64 s_frames = 0, s_be = 0, s_fe = 0, s_ud = 0, s_nc = 0, s_it = 0, s_mx = 0, s_fl = 0;
    for (unsigned k = sub; k < len; k += wpc) {
        const unsigned f = start + k;
        const size_t row = (size_t)f * Wn;
        unsigned be = 0, fl = 0;
        for (unsigned w = lane; w < Wn; w += 64u) {
            const uint32_t x = cw[row + w];
            be += (unsigned)__popc((out[row + w] ^ x) & info_mask[w]);
            fl += (unsigned)__popc((rx[row + w] ^ x) & chan_mask[w]);
        }
        be = mc_wave_sum(be);
        fl = mc_wave_sum(fl);
        const int it = min(max(iters[f], 0), n_ite);
        const bool good = ok[f] != 0;
        s_frames++; s_be += be; s_fl += fl; s_it += (mc_u64)it;
        s_mx = max(s_mx, (mc_u64)it);
        s_fe += be > 0; s_ud += good && be > 0; s_nc += !good;
        if (lane == 0) atomicAdd(hist + it, 1ull);
    }
    if (lane != 0 || s_frames == 0) return;
    mc_u64 *r = rows + (size_t)point * MCW_COUNTERS;
    atomicAdd(r + MC_FRAMES, s_frames);
    atomicAdd(r + MC_ITER_SUM, s_it);
    atomicMax(r + MC_ITER_MAX, s_mx);
    atomicAdd(r + MC_CHANNEL_BITS, s_frames * channel_vns);
    if (s_fl) atomicAdd(r + MC_FLIPS, s_fl);
    if (s_be) atomicAdd(r + MC_BIT_ERRORS, s_be);
    if (s_fe) atomicAdd(r + MC_FRAME_ERRORS, s_fe);
    if (s_ud) atomicAdd(r + MC_UNDETECTED, s_ud);
    if (s_nc) atomicAdd(r + MC_NOT_CONVERGED, s_nc);
}

/* ---- fixed-weight error strata ---- */
struct mc_stratum_row { uint32_t weight; float mag; };       /* of a stratum: its weight, qldpc_bsc_llr(design_qber) */
static_assert(sizeof(mc_stratum_row) == sizeof(mc_point_row), "a stratum row travels in the point rows of the sweep");

/* rx[slot][Wn] = cw[slot][Wn] ^ the flips of the fixed-weight frame of the slot; gridDim.x = the slots.  slot_frame == NULL: frame first + slot;
 * slot_stratum == NULL: every slot is `one`.  cls = the padded class map (past N: QLDPC_VN_PUNCTURED, never selected); key_bits 1 .. 32;
 * weight <= the channel VNs of cls */
__global__ __launch_bounds__(MC_PAT_LANES) void mc_channel_weight(const uint32_t *__restrict__ cw, uint32_t *__restrict__ rx, const uint4 *__restrict__ cls, unsigned Wn,
                                                                  uint64_t seed, uint64_t first, const uint64_t *__restrict__ slot_frame,
                                                                  const uint32_t *__restrict__ slot_stratum, const mc_stratum_row *__restrict__ strata,
                                                                  mc_stratum_row one, int key_bits, uint32_t t_pinned, float *__restrict__ llr_mag)
{
    __shared__ uint32_t hist[MC_SEL_BINS];
    __shared__ uint32_t sel[2];
    __shared__ unsigned wave_eq[MC_PAT_LANES / 64];
    const unsigned t = threadIdx.x, lane = t & 63u, wave = t >> 6, slot = blockIdx.x;
    const uint64_t frame = slot_frame ? slot_frame[slot] : first + slot;
    const mc_stratum_row st = slot_stratum ? strata[slot_stratum[slot]] : one;
    const uint32_t *cls4 = (const uint32_t *)cls;
    const unsigned quads = 8u * Wn;
    uint32_t prefix = 0, mask = 0, k = st.weight, u[4];
    for (int shift = mc_select_top_shift(key_bits); shift >= 0 && st.weight; shift -= MC_SEL_BITS) {      /* uniform over the workgroup; weight 0: T = 0, r = 0 */
        hist[t] = 0u;
        __syncthreads();
        for (unsigned g = t; g < quads; g += MC_PAT_LANES) {
            const uint32_t m = mc_weight_quad(seed, frame, g, cls4[g], 0u, u);
            for (unsigned b = 0; b < 4; b++) {
                const uint32_t key = u[b] >> (32 - key_bits);
                if (((m >> b) & 1u) && (key & mask) == prefix) atomicAdd(&hist[(key >> shift) & (MC_SEL_BINS - 1)], 1u);
            }
        }
        __syncthreads();
        if (t == 0) { uint32_t kk = k; sel[0] = mc_select_digit(hist, &kk); sel[1] = kk; }
        __syncthreads();
        prefix |= sel[0] << shift; k = sel[1];
        mask |= (uint32_t)(MC_SEL_BINS - 1) << shift;
    }
    /* T = prefix, r = k */
    const size_t row = (size_t)slot * Wn;
    unsigned equal_base = 0;
    for (unsigned w0 = 0; w0 < Wn; w0 += MC_PAT_LANES) {
        const unsigned w = w0 + t;
        uint32_t less = 0, eq = 0, pin = 0;
        if (w < Wn) {
            const uint4 a = cls[2u * w], b = cls[2u * w + 1u];
            const uint32_t c4[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
            mc_weight_masks(seed, frame, w, c4, key_bits, prefix, t_pinned, &less, &eq, &pin);
        }
        const unsigned mine = (unsigned)__popc(eq);
        unsigned incl = mine;
        for (unsigned s = 1; s < 64u; s <<= 1) { const unsigned v = __shfl_up(incl, s, 64); if (lane >= s) incl += v; }
        if (lane == 63u) wave_eq[wave] = incl;
        __syncthreads();
        unsigned before = equal_base + incl - mine;
        for (unsigned x = 0; x < MC_PAT_LANES / 64; x++) { if (x < wave) before += wave_eq[x]; equal_base += wave_eq[x]; }
        if (w < Wn) rx[row + w] = cw[row + w] ^ (mc_weight_take(less, eq, prefix, k, before) | pin);
        __syncthreads();
    }
    if (t == 0 && llr_mag) llr_mag[slot] = st.mag;
}

/* ------------------------------------------------------------------ host ---- */

struct qldpc_mc {
    qldpc_decoder *dec; qldpc_encoder *enc;      /* not owned */
    int N, K, Wn, Wk, n_ite, batch, fail_cap, device;
    unsigned channel_vns;
    uint64_t seed; double parity_ber;
    uint8_t *d_cls;                    /* [32 Wn] padded class map: qldpc_load_bits_dev reads its first N bytes, mc_channel all of it */
    uint32_t *d_info_mask, *d_chan_mask, *d_info, *d_cw, *d_rx, *d_out;
    float *d_mag; int *d_iters, *d_ok;
    mc_u64 *d_ctr;                     /* MC_COUNTERS counters, n_ite + 1 histogram bins, fail_cap frame indices */
    mc_u64 *h_ctr;                     /* pinned, MC_COUNTERS */
    hipEvent_t ev[7];                  /* the stage boundaries of a batch: source | encode | channel | load | run | fetch + monitor */
    size_t dev_bytes;
    /* puncture patterns and the search over them; the device side is allocated at first use (mc_search_reserve) */
    std::vector<uint8_t> h_cls;        /* [N] the class map, for the default candidates */
    std::vector<int> cand;             /* the candidate VNs, ascending */
    bool cand_dirty, search_ready;
    int n_fixed;                       /* VNs of the fixed puncture set of qldpc_mc_run (0 = none) */
    int *d_cand;                       /* [N] */
    uint32_t *d_pat, *d_erase, *d_fixed;   /* [batch][Wn] pattern rows, [batch][Wn] frame rows, [Wn] the fixed set */
    mc_u64 *d_rows, *h_rows;           /* [batch][MCP_COUNTERS] counter rows of a round; pinned copy */
    hipEvent_t sev[8];                 /* of a search round: patterns | expand | generate | load | erase | run | fetch + monitor */
    std::vector<qldpc_mc_pattern_stat> stats;   /* of the last search */
    /* a quantised soft-output channel in place of the BSC; the device side is allocated by the first accepted qldpc_mc_set_channel */
    bool soft;                         /* a table is in force */
    int source;                        /* QLDPC_MC_SOURCE_* */
    mc_soft_table *d_tab;
    float *d_llr;                      /* [batch][N], what qldpc_load_llr_dev takes */
    /* the QBER sweep; the device side is allocated by the first qldpc_mc_sweep (mc_sweep_reserve) */
    bool sweep_ready;
    std::vector<uint32_t> h_fixed;     /* [Wn] the fixed set of qldpc_mc_set_puncture (empty = none): a point's erase row = this OR its prefix */
    mc_u64 *d_slots, *h_slots;         /* the tables of a round and their pinned copy: [batch] 64-bit frame indices, then [batch] 32-bit words each
                                          of slot -> point, chunk -> point, chunk -> first slot, chunk -> frames */
    mc_point_row *d_points;            /* [QLDPC_MC_SWEEP_MAX_POINTS] */
    uint32_t *d_prows;                 /* [QLDPC_MC_SWEEP_MAX_POINTS][Wn] the erase rows of the points */
    mc_u64 *d_wctr, *h_wctr, *d_whist; /* [QLDPC_MC_SWEEP_MAX_POINTS][MCW_COUNTERS] counter rows, pinned copy; [..][n_ite + 1] histogram rows */
    hipEvent_t wev[8];                 /* of a sweep round: source | encode | channel | load | erase | run | fetch + monitor */
    std::vector<qldpc_mc_point_stat> wstats;    /* of the last sweep */
    /* the error strata run the sweep's rounds on the sweep's tables and device rows; rows_owner says whose counters and histograms those hold */
    int rows_owner;                    /* MC_ROWS_* */
    std::vector<qldpc_mc_stratum_stat> tstats;  /* of the last strata run */
};
enum { MC_ROWS_NONE = 0, MC_ROWS_SWEEP, MC_ROWS_STRATA };

extern "C" void qldpc_mc_cfg_default(qldpc_mc_cfg *cfg)
{
    if (!cfg) return;
    memset(cfg, 0, sizeof(*cfg));
    cfg->fail_cap = 1024;
}

extern "C" void qldpc_mc_free(qldpc_mc *mc)
{
    if (!mc) return;
    (void)hipSetDevice(mc->device);
    void *dev[] = {mc->d_cls, mc->d_info_mask, mc->d_chan_mask, mc->d_info, mc->d_cw, mc->d_rx, mc->d_out, mc->d_mag, mc->d_iters, mc->d_ok, mc->d_ctr,
                   mc->d_cand, mc->d_pat, mc->d_erase, mc->d_fixed, mc->d_rows, mc->d_tab, mc->d_llr,
                   mc->d_slots, mc->d_points, mc->d_prows, mc->d_wctr, mc->d_whist};
    for (void *p : dev) if (p) (void)hipFree(p);
    if (mc->h_ctr) (void)hipHostFree(mc->h_ctr);
    if (mc->h_rows) (void)hipHostFree(mc->h_rows);
    if (mc->h_slots) (void)hipHostFree(mc->h_slots);
    if (mc->h_wctr) (void)hipHostFree(mc->h_wctr);
    for (hipEvent_t e : mc->ev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : mc->sev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : mc->wev) if (e) (void)hipEventDestroy(e);
    delete mc;
}

template <typename T> static int mc_alloc(qldpc_mc *mc, T **p, size_t count)
{
    if (hipMalloc((void **)p, sizeof(T) * count) != hipSuccess) { *p = nullptr; qldpc_set_error("mc_create: device allocation of %zu bytes failed", sizeof(T) * count); return QLDPC_ENOMEM; }
    mc->dev_bytes += sizeof(T) * count;
    return QLDPC_OK;
}

/* the candidates a NULL list stands for: every QLDPC_VN_PINNED VN, ascending (the harness's `for a = K .. N-1`) */
static void mc_default_candidates(qldpc_mc *mc)
{
    mc->cand.clear();
    for (int v = 0; v < mc->N; v++) if (mc->h_cls[(size_t)v] == QLDPC_VN_PINNED) mc->cand.push_back(v);
    mc->cand_dirty = true;
}

static int mc_build(qldpc_mc *mc, const uint8_t *vn_class)
{
    std::vector<int> pos((size_t)mc->K);
    int rc = qldpc_encoder_info_bits_pos(mc->enc, pos.data());
    if (rc) return rc;
    const size_t Wn = (size_t)mc->Wn, B = (size_t)mc->batch;
    std::vector<uint8_t> cls(32 * Wn);
    std::vector<uint32_t> info_mask(Wn), chan_mask(Wn, 0u);
    if (mc_classes(mc->K, mc->N, pos.data(), vn_class, cls.data(), info_mask.data())) {
        qldpc_set_error("mc_create: the encoder's info_bits_pos do not fit the decoder's N = %d, or a VN class above 2", mc->N);
        return QLDPC_EINVAL;
    }
    for (int v = 0; v < mc->N; v++)
        if (cls[(size_t)v] == QLDPC_VN_CHANNEL) { chan_mask[(size_t)v >> 5] |= 0x80000000u >> (v & 31); mc->channel_vns++; }
    mc->h_cls.assign(cls.begin(), cls.begin() + mc->N);
    mc_default_candidates(mc);
    HIPCHK(hipSetDevice(mc->device));
    if ((rc = mc_alloc(mc, &mc->d_cls, 32 * Wn)) || (rc = mc_alloc(mc, &mc->d_info_mask, Wn)) || (rc = mc_alloc(mc, &mc->d_chan_mask, Wn)) ||
        (rc = mc_alloc(mc, &mc->d_info, B * (size_t)mc->Wk)) || (rc = mc_alloc(mc, &mc->d_cw, B * Wn)) || (rc = mc_alloc(mc, &mc->d_rx, B * Wn)) ||
        (rc = mc_alloc(mc, &mc->d_out, B * Wn)) || (rc = mc_alloc(mc, &mc->d_mag, B)) || (rc = mc_alloc(mc, &mc->d_iters, B)) || (rc = mc_alloc(mc, &mc->d_ok, B)) ||
        (rc = mc_alloc(mc, &mc->d_ctr, (size_t)MC_COUNTERS + (size_t)mc->n_ite + 1 + (size_t)mc->fail_cap)))
        return rc;
    if (hipHostMalloc((void **)&mc->h_ctr, sizeof(mc_u64) * MC_COUNTERS, hipHostMallocDefault) != hipSuccess) { mc->h_ctr = nullptr; return QLDPC_ENOMEM; }
    HIPCHK(hipMemcpy(mc->d_cls, cls.data(), 32 * Wn, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(mc->d_info_mask, info_mask.data(), 4 * Wn, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(mc->d_chan_mask, chan_mask.data(), 4 * Wn, hipMemcpyHostToDevice));
    for (hipEvent_t &e : mc->ev) HIPCHK(hipEventCreate(&e));
    return qldpc_encoder_reserve(mc->enc, mc->batch);
}

extern "C" int qldpc_mc_create(qldpc_decoder *dec, qldpc_encoder *enc, const uint8_t *vn_class, const qldpc_mc_cfg *cfg, qldpc_mc **out)
{
    if (!out) return QLDPC_EINVAL;
    *out = nullptr;
    if (!dec || !enc || !cfg) return QLDPC_EINVAL;
    if (cfg->reserved[0] || cfg->reserved[1]) return QLDPC_EINVAL;
    const int batch = cfg->batch ? cfg->batch : dec->cfg.max_frames;
    if (batch < 1 || batch > dec->cfg.max_frames) { qldpc_set_error("mc_create: batch=%d, the decoder holds %d frames", cfg->batch, dec->cfg.max_frames); return QLDPC_ESIZE; }
    if (cfg->fail_cap < 1) { qldpc_set_error("mc_create: fail_cap=%d (at least 1)", cfg->fail_cap); return QLDPC_ESIZE; }
    if (!(cfg->parity_ber >= 0.0 && cfg->parity_ber < 1.0)) { qldpc_set_error("mc_create: parity_ber=%g outside [0, 1)", cfg->parity_ber); return QLDPC_ESIZE; }
    if (qldpc_encoder_k(enc) != dec->K) { qldpc_set_error("mc_create: the encoder has K = %d, the decoder K = %d", qldpc_encoder_k(enc), dec->K); return QLDPC_ESIZE; }
    if ((uint64_t)batch * (uint64_t)((dec->N + 31) / 32) >= (1ull << 31)) { qldpc_set_error("mc_create: %d frames of N = %d pass 2^31 words", batch, dec->N); return QLDPC_ESIZE; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { qldpc_set_error("no HIP device visible: libqldpc has no CPU fallback"); return QLDPC_ENODEV; }
    qldpc_mc *mc = new (std::nothrow) qldpc_mc();
    if (!mc) return QLDPC_ENOMEM;
    mc->dec = dec; mc->enc = enc;
    mc->N = dec->N; mc->K = dec->K; mc->Wn = (dec->N + 31) / 32; mc->Wk = (dec->K + 31) / 32;
    mc->n_ite = dec->cfg.n_ite; mc->batch = batch; mc->fail_cap = cfg->fail_cap; mc->device = dec->device;
    mc->seed = cfg->seed; mc->parity_ber = cfg->parity_ber;
    const int rc = mc_build(mc, vn_class);
    if (rc) { qldpc_mc_free(mc); return rc; }
    *out = mc;
    return QLDPC_OK;
}

extern "C" size_t qldpc_mc_device_bytes(const qldpc_mc *mc) { return mc ? mc->dev_bytes : 0; }

static unsigned mc_blocks(size_t lanes) { return (unsigned)((lanes + MC_LANES - 1) / MC_LANES); }

/* source -> encoder -> channel for frames [first, first + n) on stream s; d_cw / d_rx / d_mag may be NULL from the right; ev != NULL: ev[1] after the
 * source, ev[2] after the encoder.  d_llr != NULL: the channel of the table instead of the BSC, LLR rows into d_llr (d_rx may then be NULL alone,
 * qber and d_mag are not used); the caller has checked n 8 Wn < 2^31 */
static int mc_generate(qldpc_mc *mc, uint64_t first, int n, double qber, uint32_t *d_info, uint32_t *d_cw, uint32_t *d_rx, float *d_mag, hipStream_t s,
                       hipEvent_t *ev = nullptr, float *d_llr = nullptr)
{
    const unsigned ti = (unsigned)n * (unsigned)mc->Wk, tn = (unsigned)n * (unsigned)mc->Wn;
    if (mc->source == QLDPC_MC_SOURCE_ZERO) HIPCHK(hipMemsetAsync(d_info, 0, sizeof(uint32_t) * ti, s));
    else {
        hipLaunchKernelGGL(mc_source, dim3(mc_blocks(ti)), dim3(MC_LANES), 0, s, d_info, ti, (unsigned)mc->Wk, mc->K, mc->seed, first);
        LAUNCHCHK();
    }
    if (ev) HIPCHK(hipEventRecord(ev[1], s));
    if (!d_cw) return QLDPC_OK;
    const int rc = qldpc_encode_packed_dev(mc->enc, d_info, d_cw, n, (void *)s);
    if (rc || (!d_rx && !d_llr)) return rc;
    if (ev) HIPCHK(hipEventRecord(ev[2], s));
    if (d_llr) {
        hipLaunchKernelGGL(mc_soft_channel, dim3(mc_blocks(8 * (size_t)tn)), dim3(MC_LANES), 0, s, (const uint32_t *)d_cw, d_rx, d_llr, (const uint32_t *)mc->d_cls,
                           (const mc_soft_table *)mc->d_tab, 8u * tn, 8u * (unsigned)mc->Wn, (unsigned)mc->N, mc->seed, first, mc_threshold(mc->parity_ber));
        LAUNCHCHK();
        return QLDPC_OK;
    }
    hipLaunchKernelGGL(mc_channel, dim3(mc_blocks(tn)), dim3(MC_LANES), 0, s, (const uint32_t *)d_cw, d_rx, (const uint4 *)mc->d_cls, tn, (unsigned)mc->Wn,
                       mc->seed, first, mc_threshold(qber), mc_threshold(mc->parity_ber), d_mag, qldpc_bsc_llr((float)qber));
    LAUNCHCHK();
    return QLDPC_OK;
}

extern "C" int qldpc_mc_frames_dev(qldpc_mc *mc, uint64_t first_frame, int n_frames, double qber, uint32_t *d_info, uint32_t *d_cw, uint32_t *d_rx)
{
    if (!mc || !d_info || (d_rx && !d_cw) || n_frames < 0) return QLDPC_EINVAL;
    if (!(qber >= 0.0 && qber < 1.0)) { qldpc_set_error("mc_frames_dev: qber=%g outside [0, 1)", qber); return QLDPC_ESIZE; }
    if ((uint64_t)n_frames * (uint64_t)mc->Wn >= (1ull << 31)) { qldpc_set_error("mc_frames_dev: %d frames of N = %d pass 2^31 words", n_frames, mc->N); return QLDPC_ESIZE; }
    if (n_frames == 0) return QLDPC_OK;
    HIPCHK(hipSetDevice(mc->device));
    return mc_generate(mc, first_frame, n_frames, qber, d_info, d_cw, d_rx, nullptr, mc->dec->stream);
}

/* the frames of a batch into the decoder, by the channel in force: generate (ev as mc_generate takes it), ev_channel, load */
static int mc_generate_load(qldpc_mc *mc, uint64_t first, int n, double qber, hipStream_t s, hipEvent_t *ev, hipEvent_t ev_channel)
{
    const int rc = mc_generate(mc, first, n, qber, mc->d_info, mc->d_cw, mc->d_rx, mc->d_mag, s, ev, mc->soft ? mc->d_llr : nullptr);
    if (rc) return rc;
    HIPCHK(hipEventRecord(ev_channel, s));
    return mc->soft ? qldpc_load_llr_dev(mc->dec, mc->d_llr, n) : qldpc_load_bits_dev(mc->dec, mc->d_rx, mc->d_mag, mc->d_cls, n);
}

/* mc_soft_channel runs n 8 Wn lanes */
static int mc_soft_lanes_check(const qldpc_mc *mc, const char *who, int n_frames)
{
    if ((uint64_t)n_frames * 8u * (uint64_t)mc->Wn < (1ull << 31)) return QLDPC_OK;
    qldpc_set_error("%s: %d frames of N = %d pass 2^31 lanes of four VNs", who, n_frames, mc->N);
    return QLDPC_ESIZE;
}

extern "C" int qldpc_mc_set_source(qldpc_mc *mc, int mode)
{
    if (!mc) return QLDPC_EINVAL;
    if (mode != QLDPC_MC_SOURCE_RANDOM && mode != QLDPC_MC_SOURCE_ZERO) { qldpc_set_error("mc_set_source: mode=%d", mode); return QLDPC_EINVAL; }
    mc->source = mode;
    return QLDPC_OK;
}

extern "C" int qldpc_mc_set_channel(qldpc_mc *mc, const qldpc_mc_channel *table)
{
    if (!mc) return QLDPC_EINVAL;
    if (!table || table->levels == 0) { mc->soft = false; return QLDPC_OK; }
    if (table->reserved[0] || table->reserved[1]) { qldpc_set_error("mc_set_channel: reserved words %d, %d must be zero", table->reserved[0], table->reserved[1]); return QLDPC_EINVAL; }
    mc_soft_table tab;
    int rc = mc_soft_table_build(table->levels, table->cum[0], table->cum[1], table->value, &tab);
    if (rc == -1) { qldpc_set_error("mc_set_channel: levels=%d outside 2 .. %d", table->levels, MC_SOFT_MAX_LEVELS); return QLDPC_ESIZE; }
    if (rc) { qldpc_set_error("mc_set_channel: a missing array, a row that decreases or an entry above 2^32"); return QLDPC_EINVAL; }
    if ((rc = mc_soft_lanes_check(mc, "mc_set_channel", mc->batch))) return rc;
    HIPCHK(hipSetDevice(mc->device));
    if ((!mc->d_tab && (rc = mc_alloc(mc, &mc->d_tab, 1))) || (!mc->d_llr && (rc = mc_alloc(mc, &mc->d_llr, (size_t)mc->batch * (size_t)mc->N)))) return rc;
    HIPCHK(hipStreamSynchronize(mc->dec->stream));      /* a queued channel kernel may still read the old table */
    HIPCHK(hipMemcpy(mc->d_tab, &tab, sizeof(tab), hipMemcpyHostToDevice));
    mc->soft = true;
    return QLDPC_OK;
}

extern "C" int qldpc_mc_llr_dev(qldpc_mc *mc, uint64_t first_frame, int n_frames, uint32_t *d_info, uint32_t *d_cw, uint32_t *d_rx, float *d_llr)
{
    if (!mc || !d_info || !d_cw || !d_llr || n_frames < 0) return QLDPC_EINVAL;
    if (!mc->soft) { qldpc_set_error("mc_llr_dev: no channel table is set (qldpc_mc_set_channel)"); return QLDPC_ESTATE; }
    const int rc = mc_soft_lanes_check(mc, "mc_llr_dev", n_frames);
    if (rc) return rc;
    if (n_frames == 0) return QLDPC_OK;
    HIPCHK(hipSetDevice(mc->device));
    return mc_generate(mc, first_frame, n_frames, 0.0, d_info, d_cw, d_rx, nullptr, mc->dec->stream, nullptr, d_llr);
}

static void mc_result(const qldpc_mc *mc, uint64_t first, qldpc_mc_result *r)
{
    const mc_u64 *c = mc->h_ctr;
    r->frames = c[MC_FRAMES]; r->bit_errors = c[MC_BIT_ERRORS]; r->frame_errors = c[MC_FRAME_ERRORS]; r->undetected = c[MC_UNDETECTED];
    r->not_converged = c[MC_NOT_CONVERGED]; r->iter_sum = c[MC_ITER_SUM]; r->iter_max = c[MC_ITER_MAX];
    r->channel_flips = c[MC_FLIPS]; r->channel_bits = c[MC_CHANNEL_BITS];
    r->next_frame = first + r->frames;
}

/* the erase rows of n frames from pattern rows that cover F slots each, into the decoder: after qldpc_load_bits_dev */
static int mc_erase(qldpc_mc *mc, const uint32_t *d_rows, int n, int F, hipStream_t s)
{
    const unsigned total = (unsigned)n * (unsigned)mc->Wn;
    hipLaunchKernelGGL(mc_expand_rows, dim3(mc_blocks(((size_t)total + 3) / 4)), dim3(MC_LANES), 0, s, d_rows, mc->d_erase, total, (unsigned)mc->Wn, (unsigned)F);
    LAUNCHCHK();
    return qldpc_load_erasures_dev(mc->dec, mc->d_erase, n);
}

extern "C" int qldpc_mc_run(qldpc_mc *mc, double qber, uint64_t first_frame, uint64_t max_frames, uint64_t max_frame_errors, qldpc_mc_result *result)
{
    if (!mc || !result) return QLDPC_EINVAL;
    memset(result, 0, sizeof(*result));
    result->next_frame = first_frame;
    if (!(qber > 0.0 && qber < 0.5)) { qldpc_set_error("mc_run: qber=%g outside (0, 0.5)", qber); return QLDPC_ESIZE; }
    HIPCHK(hipSetDevice(mc->device));
    const hipStream_t s = mc->dec->stream;
    const size_t ctr_words = (size_t)MC_COUNTERS + (size_t)mc->n_ite + 1 + (size_t)mc->fail_cap;
    mc_u64 *hist = mc->d_ctr + MC_COUNTERS, *fails = hist + mc->n_ite + 1;
    HIPCHK(hipMemsetAsync(mc->d_ctr, 0, sizeof(mc_u64) * ctr_words, s));
    memset(mc->h_ctr, 0, sizeof(mc_u64) * MC_COUNTERS);
    const auto t_start = std::chrono::steady_clock::now();
    for (uint64_t done = 0; done < max_frames;) {
        const int nb = (int)std::min<uint64_t>((uint64_t)mc->batch, max_frames - done);
        const uint64_t first = first_frame + done;
        HIPCHK(hipEventRecord(mc->ev[0], s));
        int rc = mc_generate_load(mc, first, nb, qber, s, mc->ev, mc->ev[3]);
        if (rc) return rc;
        if (mc->n_fixed && (rc = mc_erase(mc, mc->d_fixed, nb, nb, s))) return rc;      /* the fixed puncture set: one row for all nb frames */
        HIPCHK(hipEventRecord(mc->ev[4], s));
        if ((rc = qldpc_run(mc->dec))) return rc;
        HIPCHK(hipEventRecord(mc->ev[5], s));
        if ((rc = qldpc_fetch_packed_dev(mc->dec, mc->d_out))) return rc;
        if ((rc = qldpc_fetch_status_dev(mc->dec, mc->d_iters, mc->d_ok))) return rc;
        const unsigned waves = (unsigned)std::min(nb, MC_MAX_WAVES);
        hipLaunchKernelGGL(mc_monitor, dim3((waves + 3u) / 4u), dim3(MC_LANES), 0, s, (const uint32_t *)mc->d_out, (const uint32_t *)mc->d_cw, (const uint32_t *)mc->d_rx,
                           (const uint32_t *)mc->d_info_mask, (const uint32_t *)mc->d_chan_mask, (const int *)mc->d_iters, (const int *)mc->d_ok, (unsigned)nb,
                           (unsigned)mc->Wn, mc->n_ite, first, mc->channel_vns, mc->d_ctr, hist, fails, (unsigned)mc->fail_cap);
        LAUNCHCHK();
        HIPCHK(hipEventRecord(mc->ev[6], s));
        HIPCHK(hipMemcpyAsync(mc->h_ctr, mc->d_ctr, sizeof(mc_u64) * MC_COUNTERS, hipMemcpyDeviceToHost, s));      /* the one read-back of a batch */
        HIPCHK(hipStreamSynchronize(s));
        double *const stage[6] = {&result->source_ms, &result->encode_ms, &result->channel_ms, &result->load_ms, &result->decode_ms, &result->monitor_ms};
        for (int k = 0; k < 6; k++) {
            float ms = 0.0f;
            HIPCHK(hipEventElapsedTime(&ms, mc->ev[k], mc->ev[k + 1]));
            *stage[k] += (double)ms;
        }
        result->batches++;
        done += (uint64_t)nb;
        if (max_frame_errors && mc->h_ctr[MC_FRAME_ERRORS] >= max_frame_errors) break;
    }
    result->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    mc_result(mc, first_frame, result);
    return QLDPC_OK;
}

extern "C" int qldpc_mc_iter_hist(qldpc_mc *mc, uint64_t *hist, int cap)
{
    if (!mc || !hist || cap < 0) return QLDPC_EINVAL;
    const int bins = std::min(cap, mc->n_ite + 1);
    HIPCHK(hipSetDevice(mc->device));
    HIPCHK(hipStreamSynchronize(mc->dec->stream));
    if (bins) HIPCHK(hipMemcpy(hist, mc->d_ctr + MC_COUNTERS, sizeof(mc_u64) * (size_t)bins, hipMemcpyDeviceToHost));
    return mc->n_ite + 1;
}

extern "C" int qldpc_mc_failed_frames(qldpc_mc *mc, uint64_t *frames, int cap)
{
    if (!mc || cap < 0 || (cap && !frames)) return QLDPC_EINVAL;
    HIPCHK(hipSetDevice(mc->device));
    HIPCHK(hipStreamSynchronize(mc->dec->stream));
    mc_u64 slots = 0;
    HIPCHK(hipMemcpy(&slots, mc->d_ctr + MC_FAIL_SLOTS, sizeof(slots), hipMemcpyDeviceToHost));
    const int listed = (int)std::min<mc_u64>(slots, (mc_u64)mc->fail_cap);
    if (listed == 0) return 0;
    std::vector<uint64_t> all((size_t)listed);
    HIPCHK(hipMemcpy(all.data(), mc->d_ctr + MC_COUNTERS + mc->n_ite + 1, sizeof(mc_u64) * (size_t)listed, hipMemcpyDeviceToHost));
    std::sort(all.begin(), all.end());      /* the slots of a batch are handed out in arrival order */
    const int n = std::min(listed, cap);
    if (n) memcpy(frames, all.data(), sizeof(uint64_t) * (size_t)n);
    return listed;
}

/* ------------------------------------------------------------------ puncture patterns, search ---- */

/* everything the pattern calls need on the device, once; then the candidate list if it changed */
static int mc_search_reserve(qldpc_mc *mc)
{
    HIPCHK(hipSetDevice(mc->device));
    if (!mc->search_ready) {
        const size_t Wn = (size_t)mc->Wn, B = (size_t)mc->batch;
        int rc = QLDPC_OK;
        if ((!mc->d_cand && (rc = mc_alloc(mc, &mc->d_cand, (size_t)mc->N))) || (!mc->d_pat && (rc = mc_alloc(mc, &mc->d_pat, B * Wn))) ||
            (!mc->d_erase && (rc = mc_alloc(mc, &mc->d_erase, B * Wn))) || (!mc->d_fixed && (rc = mc_alloc(mc, &mc->d_fixed, Wn))) ||
            (!mc->d_rows && (rc = mc_alloc(mc, &mc->d_rows, B * MCP_COUNTERS))))
            return rc;
        if (!mc->h_rows && hipHostMalloc((void **)&mc->h_rows, sizeof(mc_u64) * B * MCP_COUNTERS, hipHostMallocDefault) != hipSuccess) { mc->h_rows = nullptr; return QLDPC_ENOMEM; }
        for (hipEvent_t &e : mc->sev) if (!e) HIPCHK(hipEventCreate(&e));
        if ((rc = qldpc_decoder_reserve(mc->dec))) return rc;      /* the decoder's erasure ballots */
        mc->search_ready = true;
    }
    if (mc->cand_dirty) {
        HIPCHK(hipStreamSynchronize(mc->dec->stream));      /* a queued pattern kernel may still read the old list */
        if (!mc->cand.empty()) HIPCHK(hipMemcpy(mc->d_cand, mc->cand.data(), sizeof(int) * mc->cand.size(), hipMemcpyHostToDevice));
        mc->cand_dirty = false;
    }
    return QLDPC_OK;
}

static int mc_pattern_args(const qldpc_mc *mc, const char *who, int n_punct, int key_bits)
{
    if (n_punct < 0 || n_punct > (int)mc->cand.size()) { qldpc_set_error("%s: n_punct=%d outside [0, %d candidates]", who, n_punct, (int)mc->cand.size()); return QLDPC_ESIZE; }
    if (key_bits < 0 || key_bits > 32) { qldpc_set_error("%s: key_bits=%d outside 0 .. 32", who, key_bits); return QLDPC_ESIZE; }
    return QLDPC_OK;
}

static int mc_vn_list_args(const qldpc_mc *mc, const char *who, const int *vn, int n)
{
    if (n < 0 || (n > 0 && !vn)) { qldpc_set_error("%s: n=%d", who, n); return QLDPC_EINVAL; }
    const int bad = mc_vn_list_check(vn, n, mc->N);
    if (bad >= 0) { qldpc_set_error("%s: entry %d = %d is not ascending, distinct and inside [0, %d)", who, bad, vn[bad], mc->N); return QLDPC_EINVAL; }
    return QLDPC_OK;
}

extern "C" int qldpc_mc_set_candidates(qldpc_mc *mc, const int *vn, int n)
{
    if (!mc) return QLDPC_EINVAL;
    if (!vn) { mc_default_candidates(mc); return QLDPC_OK; }
    const int rc = mc_vn_list_args(mc, "mc_set_candidates", vn, n);
    if (rc) return rc;
    mc->cand.assign(vn, vn + n);
    mc->cand_dirty = true;
    return QLDPC_OK;
}

static void mc_launch_patterns(qldpc_mc *mc, uint64_t first, int n, int n_punct, int key_bits, uint32_t *d_rows, hipStream_t s)
{
    hipLaunchKernelGGL(mc_patterns, dim3((unsigned)n), dim3(MC_PAT_LANES), 0, s, d_rows, (const int *)mc->d_cand, (unsigned)mc->cand.size(), (unsigned)n_punct,
                       mc_key_bits(key_bits), (unsigned)mc->Wn, mc->seed, first);
}

extern "C" int qldpc_mc_patterns_dev(qldpc_mc *mc, uint64_t first_pattern, int n_patterns, int n_punct, int key_bits, uint32_t *d_erase)
{
    if (!mc || n_patterns < 0 || (n_patterns && !d_erase)) return QLDPC_EINVAL;
    int rc = mc_pattern_args(mc, "mc_patterns_dev", n_punct, key_bits);
    if (rc || (rc = mc_search_reserve(mc)) || n_patterns == 0) return rc;
    mc_launch_patterns(mc, first_pattern, n_patterns, n_punct, key_bits, d_erase, mc->dec->stream);
    LAUNCHCHK();
    return QLDPC_OK;
}

extern "C" int qldpc_mc_pattern_vns(qldpc_mc *mc, uint64_t pattern, int n_punct, int key_bits, int *vn)
{
    if (!mc || (n_punct > 0 && !vn)) return QLDPC_EINVAL;
    int rc = mc_pattern_args(mc, "mc_pattern_vns", n_punct, key_bits);
    if (rc || (rc = qldpc_mc_pattern_host(mc->seed, pattern, (int)mc->cand.size(), n_punct, key_bits, vn))) return rc;
    for (int i = 0; i < n_punct; i++) vn[i] = mc->cand[(size_t)vn[i]];
    return QLDPC_OK;
}

extern "C" int qldpc_mc_set_puncture(qldpc_mc *mc, const int *vn, int n)
{
    if (!mc) return QLDPC_EINVAL;
    int rc = mc_vn_list_args(mc, "mc_set_puncture", vn, n);
    if (rc) return rc;
    if (n == 0) { mc->n_fixed = 0; mc->h_fixed.clear(); return QLDPC_OK; }
    if ((rc = mc_search_reserve(mc))) return rc;
    std::vector<uint32_t> row((size_t)mc->Wn);
    mc_vn_list_row(vn, n, mc->N, row.data());
    HIPCHK(hipStreamSynchronize(mc->dec->stream));
    HIPCHK(hipMemcpy(mc->d_fixed, row.data(), sizeof(uint32_t) * row.size(), hipMemcpyHostToDevice));
    mc->n_fixed = n;
    mc->h_fixed.swap(row);      /* the sweep builds its points' erase rows on the host */
    return QLDPC_OK;
}

extern "C" int qldpc_mc_search(qldpc_mc *mc, double qber, const qldpc_mc_search_cfg *cfg, uint64_t first_pattern, uint64_t max_patterns, qldpc_mc_search_result *res)
{
    if (!mc || !cfg || !res) return QLDPC_EINVAL;
    memset(res, 0, sizeof(*res));
    res->goal = res->best = UINT64_MAX;
    res->next_pattern = first_pattern;
    if (cfg->reserved[0] || cfg->reserved[1]) { qldpc_set_error("mc_search: reserved fields %d, %d must be zero", cfg->reserved[0], cfg->reserved[1]); return QLDPC_EINVAL; }
    if (!(qber > 0.0 && qber < 0.5)) { qldpc_set_error("mc_search: qber=%g outside (0, 0.5)", qber); return QLDPC_ESIZE; }
    if (cfg->frames_per_pattern < 1 || cfg->frames_per_pattern > mc->batch) { qldpc_set_error("mc_search: frames_per_pattern=%d outside [1, batch=%d]", cfg->frames_per_pattern, mc->batch); return QLDPC_ESIZE; }
    int rc = mc_pattern_args(mc, "mc_search", cfg->n_punct, cfg->key_bits);
    if (rc || (rc = mc_search_reserve(mc))) return rc;
    const hipStream_t s = mc->dec->stream;
    const unsigned F = (unsigned)cfg->frames_per_pattern, Wn = (unsigned)mc->Wn;
    const uint64_t per_round = (uint64_t)mc->batch / F;
    mc->stats.clear();
    const auto t_start = std::chrono::steady_clock::now();
    for (uint64_t done = 0; done < max_patterns;) {
        const int np = (int)std::min<uint64_t>(per_round, max_patterns - done), nb = np * (int)F;
        const uint64_t p0 = first_pattern + done, frame0 = cfg->first_frame + p0 * F;      /* frame k of pattern p = first_frame + p F + k */
        HIPCHK(hipEventRecord(mc->sev[0], s));
        mc_launch_patterns(mc, p0, np, cfg->n_punct, cfg->key_bits, mc->d_pat, s);
        LAUNCHCHK();
        HIPCHK(hipEventRecord(mc->sev[1], s));
        const unsigned total = (unsigned)nb * Wn;
        hipLaunchKernelGGL(mc_expand_rows, dim3(mc_blocks(((size_t)total + 3) / 4)), dim3(MC_LANES), 0, s, (const uint32_t *)mc->d_pat, mc->d_erase, total, Wn, F);
        LAUNCHCHK();
        HIPCHK(hipEventRecord(mc->sev[2], s));
        if ((rc = mc_generate_load(mc, frame0, nb, qber, s, nullptr, mc->sev[3]))) return rc;
        HIPCHK(hipEventRecord(mc->sev[4], s));
        if ((rc = qldpc_load_erasures_dev(mc->dec, mc->d_erase, nb))) return rc;
        HIPCHK(hipEventRecord(mc->sev[5], s));
        if ((rc = qldpc_run(mc->dec))) return rc;
        HIPCHK(hipEventRecord(mc->sev[6], s));
        if ((rc = qldpc_fetch_packed_dev(mc->dec, mc->d_out))) return rc;
        if ((rc = qldpc_fetch_status_dev(mc->dec, mc->d_iters, mc->d_ok))) return rc;
        HIPCHK(hipMemsetAsync(mc->d_rows, 0, sizeof(mc_u64) * (size_t)np * MCP_COUNTERS, s));
        const unsigned wpp = std::min(F, std::max(1u, (unsigned)MC_MAX_WAVES / (unsigned)np)), waves = (unsigned)np * wpp;
        hipLaunchKernelGGL(mc_monitor_patterns, dim3((waves + 3u) / 4u), dim3(MC_LANES), 0, s, (const uint32_t *)mc->d_out, (const uint32_t *)mc->d_cw,
                           (const uint32_t *)mc->d_info_mask, (const int *)mc->d_iters, (const int *)mc->d_ok, (unsigned)np, F, wpp, Wn, mc->n_ite, mc->d_rows);
        LAUNCHCHK();
        HIPCHK(hipEventRecord(mc->sev[7], s));
        HIPCHK(hipMemcpyAsync(mc->h_rows, mc->d_rows, sizeof(mc_u64) * (size_t)np * MCP_COUNTERS, hipMemcpyDeviceToHost, s));      /* the one read-back of a round */
        HIPCHK(hipStreamSynchronize(s));
        double *const stage[7] = {&res->pattern_ms, &res->expand_ms, &res->generate_ms, &res->load_ms, &res->erase_ms, &res->decode_ms, &res->monitor_ms};
        for (int k = 0; k < 7; k++) {
            float ms = 0.0f;
            HIPCHK(hipEventElapsedTime(&ms, mc->sev[k], mc->sev[k + 1]));
            *stage[k] += (double)ms;
        }
        for (int i = 0; i < np; i++) {
            const mc_u64 *c = mc->h_rows + (size_t)i * MCP_COUNTERS;
            qldpc_mc_pattern_stat st = {p0 + (uint64_t)i, c[MCP_FRAMES], c[MCP_FRAME_ERRORS], c[MCP_BIT_ERRORS], c[MCP_UNDETECTED], c[MCP_NOT_CONVERGED], c[MCP_ITER_SUM]};
            mc->stats.push_back(st);
            if (st.frame_errors == 0 && res->goal == UINT64_MAX) res->goal = st.pattern;
            if (res->best == UINT64_MAX || st.frame_errors < res->best_frame_errors || (st.frame_errors == res->best_frame_errors && st.bit_errors < res->best_bit_errors)) {
                res->best = st.pattern; res->best_frame_errors = st.frame_errors; res->best_bit_errors = st.bit_errors;
            }
        }
        res->batches++;
        res->patterns += (uint64_t)np; res->frames += (uint64_t)nb;
        done += (uint64_t)np;
        if (cfg->stop_at_goal && res->goal != UINT64_MAX) break;
    }
    res->next_pattern = first_pattern + res->patterns;
    res->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    return QLDPC_OK;
}

extern "C" int qldpc_mc_search_stats(qldpc_mc *mc, qldpc_mc_pattern_stat *rows, int cap)
{
    if (!mc || cap < 0 || (cap && !rows)) return QLDPC_EINVAL;
    const size_t n = std::min((size_t)cap, mc->stats.size());
    if (n) memcpy(rows, mc->stats.data(), sizeof(qldpc_mc_pattern_stat) * n);
    return (int)mc->stats.size();
}

/* ------------------------------------------------------------------ QBER sweep ---- */

/* everything the sweep needs on the device, once */
static int mc_sweep_reserve(qldpc_mc *mc)
{
    HIPCHK(hipSetDevice(mc->device));
    if (mc->sweep_ready) return QLDPC_OK;
    const size_t Wn = (size_t)mc->Wn, B = (size_t)mc->batch, P = QLDPC_MC_SWEEP_MAX_POINTS, bins = (size_t)mc->n_ite + 1;
    int rc = QLDPC_OK;
    if ((!mc->d_slots && (rc = mc_alloc(mc, &mc->d_slots, 3 * B))) || (!mc->d_points && (rc = mc_alloc(mc, &mc->d_points, P))) ||
        (!mc->d_prows && (rc = mc_alloc(mc, &mc->d_prows, P * Wn))) || (!mc->d_erase && (rc = mc_alloc(mc, &mc->d_erase, B * Wn))) ||
        (!mc->d_wctr && (rc = mc_alloc(mc, &mc->d_wctr, P * MCW_COUNTERS))) || (!mc->d_whist && (rc = mc_alloc(mc, &mc->d_whist, P * bins))))
        return rc;
    if (!mc->h_slots && hipHostMalloc((void **)&mc->h_slots, sizeof(mc_u64) * 3 * B, hipHostMallocDefault) != hipSuccess) { mc->h_slots = nullptr; return QLDPC_ENOMEM; }
    if (!mc->h_wctr && hipHostMalloc((void **)&mc->h_wctr, sizeof(mc_u64) * P * MCW_COUNTERS, hipHostMallocDefault) != hipSuccess) { mc->h_wctr = nullptr; return QLDPC_ENOMEM; }
    for (hipEvent_t &e : mc->wev) if (!e) HIPCHK(hipEventCreate(&e));
    if ((rc = qldpc_decoder_reserve(mc->dec))) return rc;      /* the decoder's erasure ballots */
    mc->sweep_ready = true;
    return QLDPC_OK;
}

/* every argument check of qldpc_mc_sweep: nothing is touched before all of them pass */
static int mc_sweep_args(const qldpc_mc *mc, const qldpc_mc_sweep_cfg *cfg)
{
    if (cfg->reserved[0] || cfg->reserved[1]) { qldpc_set_error("mc_sweep: reserved fields %d, %d must be zero", cfg->reserved[0], cfg->reserved[1]); return QLDPC_EINVAL; }
    if (mc->soft) { qldpc_set_error("mc_sweep: a channel table is in force (qldpc_mc_set_channel); the sweep's points are points of the BSC"); return QLDPC_ESTATE; }
    if (cfg->n_points < 1 || cfg->n_points > QLDPC_MC_SWEEP_MAX_POINTS) { qldpc_set_error("mc_sweep: n_points=%d outside 1 .. %d", cfg->n_points, QLDPC_MC_SWEEP_MAX_POINTS); return QLDPC_ESIZE; }
    if (cfg->chunk < 0 || cfg->chunk > mc->batch) { qldpc_set_error("mc_sweep: chunk=%d outside [0, batch=%d]", cfg->chunk, mc->batch); return QLDPC_ESIZE; }
    if (cfg->max_frames == 0) { qldpc_set_error("mc_sweep: max_frames=0"); return QLDPC_ESIZE; }
    if (!cfg->points || cfg->n_order < 0 || (cfg->n_order > 0 && !cfg->punct_order)) { qldpc_set_error("mc_sweep: a missing array (points, or punct_order with n_order=%d)", cfg->n_order); return QLDPC_EINVAL; }
    std::vector<bool> seen((size_t)mc->N, false);
    for (int i = 0; i < cfg->n_order; i++) {
        const int v = cfg->punct_order[i];
        if (v < 0 || v >= mc->N || seen[(size_t)v]) { qldpc_set_error("mc_sweep: punct_order[%d] = %d is repeated or outside [0, %d)", i, v, mc->N); return QLDPC_EINVAL; }
        seen[(size_t)v] = true;
    }
    for (int q = 0; q < cfg->n_points; q++) {
        const qldpc_mc_point &pt = cfg->points[q];
        if (pt.reserved) { qldpc_set_error("mc_sweep: reserved field %d of point %d must be zero", pt.reserved, q); return QLDPC_EINVAL; }
        if (!(pt.qber > 0.0 && pt.qber < 0.5)) { qldpc_set_error("mc_sweep: qber=%g of point %d outside (0, 0.5)", pt.qber, q); return QLDPC_ESIZE; }
        if (pt.n_punct < 0 || pt.n_punct > cfg->n_order) { qldpc_set_error("mc_sweep: n_punct=%d of point %d outside [0, n_order=%d]", pt.n_punct, q, cfg->n_order); return QLDPC_ESIZE; }
    }
    return QLDPC_OK;
}

/* the rounds of qldpc_mc_sweep and of qldpc_mc_strata: P rows side by side in one batch, each over frames first_frame + k with its own counter
 * row, histogram row and stop rule; per round the deal, the slot tables, generate / encode / channel / load / erase / run / fetch / monitor and
 * ONE read-back of the P counter rows, which stay in h_wctr.  The caller has checked every argument and reserved the device side. */
struct mc_rounds_job {
    int P, C;
    uint64_t first_frame, max_frames, max_fe;
    const mc_point_row *rows;          /* [P] {threshold, |LLR|} of the sweep's points, or the strata's {weight, |LLR|} in the same layout */
    const uint32_t *erows;             /* [P][Wn] the erase rows, NULL = nothing is erased */
    int weight_key_bits;               /* 0: the BSC of the rows' thresholds (mc_channel_points); 1 .. 32: the rows' fixed weights (mc_channel_weight) */
    int owner;                         /* MC_ROWS_*: whose rows the device holds from here on */
};

static int mc_rounds(qldpc_mc *mc, const mc_rounds_job &job, uint64_t *last_round /* [P] */, qldpc_mc_sweep_result *res)
{
    const hipStream_t s = mc->dec->stream;
    const int P = job.P, C = job.C, S = mc->batch / C;
    const unsigned Wn = (unsigned)mc->Wn, Wk = (unsigned)mc->Wk;
    const size_t B = (size_t)mc->batch, bins = (size_t)mc->n_ite + 1;
    const uint64_t max_frames = job.max_frames, max_fe = job.max_fe;
    const bool any_erase = job.erows != nullptr;
    const mc_stratum_row no_row = {0u, 0.0f};      /* mc_channel_weight reads the rows of the round */
    /* the tables of a round inside the one buffer */
    uint64_t *const h_frame = (uint64_t *)mc->h_slots;
    uint32_t *const h_point = (uint32_t *)(mc->h_slots + B), *const h_cpoint = h_point + B, *const h_cstart = h_cpoint + B, *const h_clen = h_cstart + B;
    const uint64_t *const d_frame = (const uint64_t *)mc->d_slots;
    const uint32_t *const d_point = (const uint32_t *)(mc->d_slots + B), *const d_cpoint = d_point + B, *const d_cstart = d_cpoint + B, *const d_clen = d_cstart + B;

    HIPCHK(hipStreamSynchronize(s));      /* a queued kernel may still read the rows of an earlier call */
    HIPCHK(hipMemcpy(mc->d_points, job.rows, sizeof(mc_point_row) * (size_t)P, hipMemcpyHostToDevice));
    if (any_erase) HIPCHK(hipMemcpy(mc->d_prows, job.erows, sizeof(uint32_t) * (size_t)P * Wn, hipMemcpyHostToDevice));
    mc->rows_owner = job.owner;
    HIPCHK(hipMemsetAsync(mc->d_wctr, 0, sizeof(mc_u64) * (size_t)P * MCW_COUNTERS, s));
    HIPCHK(hipMemsetAsync(mc->d_whist, 0, sizeof(mc_u64) * (size_t)P * bins, s));

    std::vector<uint64_t> done((size_t)P, 0), fe((size_t)P, 0);
    std::vector<int> give((size_t)P);
    int rc = QLDPC_OK;
    const auto t_start = std::chrono::steady_clock::now();
    for (uint64_t round = 0;; round++) {
        const int n_chunks = mc_sweep_deal(P, C, S, max_frames, max_fe, done.data(), fe.data(), give.data());
        if (n_chunks == 0) break;      /* no point is open */
        unsigned nb = 0, nc = 0;
        for (int q = 0; q < P; q++)
            for (int j = 0; j < give[(size_t)q]; j++, nc++) {
                const uint64_t k0 = done[(size_t)q] + (uint64_t)j * (uint64_t)C;
                const unsigned len = (unsigned)std::min<uint64_t>((uint64_t)C, max_frames - k0);
                h_cpoint[nc] = (uint32_t)q; h_cstart[nc] = nb; h_clen[nc] = len;
                for (unsigned i = 0; i < len; i++, nb++) { h_frame[nb] = job.first_frame + k0 + i; h_point[nb] = (uint32_t)q; }
                last_round[q] = round;
            }
        const unsigned ti = nb * Wk, tn = nb * Wn;
        HIPCHK(hipEventRecord(mc->wev[0], s));
        HIPCHK(hipMemcpyAsync(mc->d_slots, mc->h_slots, sizeof(mc_u64) * 3 * B, hipMemcpyHostToDevice, s));      /* pinned: the host rewrites it after the sync below */
        if (mc->source == QLDPC_MC_SOURCE_ZERO) HIPCHK(hipMemsetAsync(mc->d_info, 0, sizeof(uint32_t) * ti, s));
        else {
            hipLaunchKernelGGL(mc_source_points, dim3(mc_blocks(ti)), dim3(MC_LANES), 0, s, mc->d_info, ti, Wk, mc->K, mc->seed, d_frame);
            LAUNCHCHK();
        }
        HIPCHK(hipEventRecord(mc->wev[1], s));
        if ((rc = qldpc_encode_packed_dev(mc->enc, mc->d_info, mc->d_cw, (int)nb, (void *)s))) return rc;
        HIPCHK(hipEventRecord(mc->wev[2], s));
        if (job.weight_key_bits)
            hipLaunchKernelGGL(mc_channel_weight, dim3(nb), dim3(MC_PAT_LANES), 0, s, (const uint32_t *)mc->d_cw, mc->d_rx, (const uint4 *)mc->d_cls, Wn, mc->seed, (uint64_t)0,
                               d_frame, d_point, (const mc_stratum_row *)mc->d_points, no_row, job.weight_key_bits, mc_threshold(mc->parity_ber), mc->d_mag);
        else
            hipLaunchKernelGGL(mc_channel_points, dim3(mc_blocks(tn)), dim3(MC_LANES), 0, s, (const uint32_t *)mc->d_cw, mc->d_rx, (const uint4 *)mc->d_cls, tn, Wn, mc->seed,
                               d_frame, d_point, (const mc_point_row *)mc->d_points, mc_threshold(mc->parity_ber), mc->d_mag);
        LAUNCHCHK();
        HIPCHK(hipEventRecord(mc->wev[3], s));
        if ((rc = qldpc_load_bits_dev(mc->dec, mc->d_rx, mc->d_mag, mc->d_cls, (int)nb))) return rc;
        HIPCHK(hipEventRecord(mc->wev[4], s));
        if (any_erase) {
            hipLaunchKernelGGL(mc_expand_points, dim3(mc_blocks(((size_t)tn + 3) / 4)), dim3(MC_LANES), 0, s, (const uint32_t *)mc->d_prows, mc->d_erase, tn, Wn, d_point);
            LAUNCHCHK();
            if ((rc = qldpc_load_erasures_dev(mc->dec, mc->d_erase, (int)nb))) return rc;
        }
        HIPCHK(hipEventRecord(mc->wev[5], s));
        if ((rc = qldpc_run(mc->dec))) return rc;
        HIPCHK(hipEventRecord(mc->wev[6], s));
        if ((rc = qldpc_fetch_packed_dev(mc->dec, mc->d_out))) return rc;
        if ((rc = qldpc_fetch_status_dev(mc->dec, mc->d_iters, mc->d_ok))) return rc;
        const unsigned wpc = std::min((unsigned)C, std::max(1u, (unsigned)MC_MAX_WAVES / nc)), waves = nc * wpc;
        hipLaunchKernelGGL(mc_monitor_points, dim3((waves + 3u) / 4u), dim3(MC_LANES), 0, s, (const uint32_t *)mc->d_out, (const uint32_t *)mc->d_cw, (const uint32_t *)mc->d_rx,
                           (const uint32_t *)mc->d_info_mask, (const uint32_t *)mc->d_chan_mask, (const int *)mc->d_iters, (const int *)mc->d_ok, nc, wpc, d_cpoint, d_cstart,
                           d_clen, Wn, mc->n_ite, mc->channel_vns, mc->d_wctr, mc->d_whist);
        LAUNCHCHK();
        HIPCHK(hipEventRecord(mc->wev[7], s));
        HIPCHK(hipMemcpyAsync(mc->h_wctr, mc->d_wctr, sizeof(mc_u64) * (size_t)P * MCW_COUNTERS, hipMemcpyDeviceToHost, s));      /* the one read-back of a round */
        HIPCHK(hipStreamSynchronize(s));
        double *const stage[7] = {&res->source_ms, &res->encode_ms, &res->channel_ms, &res->load_ms, &res->erase_ms, &res->decode_ms, &res->monitor_ms};
        for (int k = 0; k < 7; k++) {
            float ms = 0.0f;
            HIPCHK(hipEventElapsedTime(&ms, mc->wev[k], mc->wev[k + 1]));
            *stage[k] += (double)ms;
        }
        for (int q = 0; q < P; q++) { done[(size_t)q] = mc->h_wctr[(size_t)q * MCW_COUNTERS + MC_FRAMES]; fe[(size_t)q] = mc->h_wctr[(size_t)q * MCW_COUNTERS + MC_FRAME_ERRORS]; }
        res->rounds++; res->batches++;
    }
    for (int q = 0; q < P; q++) res->frames += mc->h_wctr[(size_t)q * MCW_COUNTERS + MC_FRAMES];
    res->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    return QLDPC_OK;
}

extern "C" int qldpc_mc_sweep(qldpc_mc *mc, const qldpc_mc_sweep_cfg *cfg, qldpc_mc_sweep_result *res)
{
    if (!mc || !cfg || !res) return QLDPC_EINVAL;
    memset(res, 0, sizeof(*res));
    int rc = mc_sweep_args(mc, cfg);
    if (rc || (rc = mc_sweep_reserve(mc))) return rc;
    const int P = cfg->n_points;
    const size_t Wn = (size_t)mc->Wn;
    /* per sweep: the point rows and the erase rows (fixed set OR prefix), built here once */
    std::vector<mc_point_row> prow((size_t)P);
    std::vector<uint32_t> erows((size_t)P * Wn, 0u);
    bool any_erase = false;
    for (int q = 0; q < P; q++) {
        prow[(size_t)q].t_channel = mc_threshold(cfg->points[q].qber);
        prow[(size_t)q].mag = qldpc_bsc_llr((float)cfg->points[q].qber);
        uint32_t *row = erows.data() + (size_t)q * Wn;
        if (mc->n_fixed) memcpy(row, mc->h_fixed.data(), sizeof(uint32_t) * Wn);
        for (int i = 0; i < cfg->points[q].n_punct; i++) { const int v = cfg->punct_order[i]; row[v >> 5] |= 0x80000000u >> (v & 31); }
        any_erase = any_erase || mc->n_fixed || cfg->points[q].n_punct > 0;
    }
    mc->wstats.assign((size_t)P, qldpc_mc_point_stat());
    for (int q = 0; q < P; q++) { mc->wstats[(size_t)q].qber = cfg->points[q].qber; mc->wstats[(size_t)q].n_punct = cfg->points[q].n_punct; }
    const mc_rounds_job job = {P, cfg->chunk ? cfg->chunk : std::min(64, mc->batch), cfg->first_frame, cfg->max_frames, cfg->max_frame_errors, prow.data(),
                               any_erase ? erows.data() : nullptr, 0, MC_ROWS_SWEEP};
    std::vector<uint64_t> last((size_t)P, 0);
    if ((rc = mc_rounds(mc, job, last.data(), res))) return rc;
    for (int q = 0; q < P; q++) {
        const mc_u64 *c = mc->h_wctr + (size_t)q * MCW_COUNTERS;
        qldpc_mc_point_stat &st = mc->wstats[(size_t)q];
        st.frames = c[MC_FRAMES]; st.frame_errors = c[MC_FRAME_ERRORS]; st.bit_errors = c[MC_BIT_ERRORS]; st.undetected = c[MC_UNDETECTED];
        st.not_converged = c[MC_NOT_CONVERGED]; st.iter_sum = c[MC_ITER_SUM]; st.iter_max = c[MC_ITER_MAX];
        st.channel_flips = c[MC_FLIPS]; st.channel_bits = c[MC_CHANNEL_BITS];
        st.closed_by = st.frames >= cfg->max_frames ? QLDPC_MC_CLOSED_MAX_FRAMES : QLDPC_MC_CLOSED_MAX_FE;
        st.last_round = last[(size_t)q];
    }
    return QLDPC_OK;
}

extern "C" int qldpc_mc_sweep_stats(qldpc_mc *mc, qldpc_mc_point_stat *rows, int cap)
{
    if (!mc || cap < 0 || (cap && !rows)) return QLDPC_EINVAL;
    const size_t n = std::min((size_t)cap, mc->wstats.size());
    if (n) memcpy(rows, mc->wstats.data(), sizeof(qldpc_mc_point_stat) * n);
    return (int)mc->wstats.size();
}

extern "C" int qldpc_mc_sweep_hist(qldpc_mc *mc, int point, uint64_t *hist, int cap)
{
    if (!mc || cap < 0 || (cap && !hist)) return QLDPC_EINVAL;
    if (point < 0 || (size_t)point >= mc->wstats.size()) { qldpc_set_error("mc_sweep_hist: point=%d, the last sweep had %d", point, (int)mc->wstats.size()); return QLDPC_ESIZE; }
    if (mc->rows_owner != MC_ROWS_SWEEP) { qldpc_set_error("mc_sweep_hist: the device rows hold a later qldpc_mc_strata run"); return QLDPC_ESTATE; }
    const int bins = std::min(cap, mc->n_ite + 1);
    HIPCHK(hipSetDevice(mc->device));
    HIPCHK(hipStreamSynchronize(mc->dec->stream));
    if (bins) HIPCHK(hipMemcpy(hist, mc->d_whist + (size_t)point * (size_t)(mc->n_ite + 1), sizeof(mc_u64) * (size_t)bins, hipMemcpyDeviceToHost));
    return mc->n_ite + 1;
}

/* ------------------------------------------------------------------ fixed-weight error strata ---- */

static int mc_weight_args(const qldpc_mc *mc, const char *who, int weight, int key_bits)
{
    if (weight < 0 || (unsigned)weight > mc->channel_vns) { qldpc_set_error("%s: weight=%d outside [0, %u channel VNs]", who, weight, mc->channel_vns); return QLDPC_ESIZE; }
    if (key_bits < 0 || key_bits > 32) { qldpc_set_error("%s: key_bits=%d outside 0 .. 32", who, key_bits); return QLDPC_ESIZE; }
    return QLDPC_OK;
}

extern "C" int qldpc_mc_weight_frames_dev(qldpc_mc *mc, uint64_t first_frame, int n_frames, int weight, int key_bits, uint32_t *d_info, uint32_t *d_cw, uint32_t *d_rx)
{
    if (!mc || !d_info || (d_rx && !d_cw) || n_frames < 0) return QLDPC_EINVAL;
    int rc = mc_weight_args(mc, "mc_weight_frames_dev", weight, key_bits);
    if (rc) return rc;
    if ((uint64_t)n_frames * (uint64_t)mc->Wn >= (1ull << 31)) { qldpc_set_error("mc_weight_frames_dev: %d frames of N = %d pass 2^31 words", n_frames, mc->N); return QLDPC_ESIZE; }
    if (n_frames == 0) return QLDPC_OK;
    HIPCHK(hipSetDevice(mc->device));
    const hipStream_t s = mc->dec->stream;
    if ((rc = mc_generate(mc, first_frame, n_frames, 0.0, d_info, d_cw, nullptr, nullptr, s)) || !d_rx) return rc;      /* source and encoder */
    const mc_stratum_row one = {(uint32_t)weight, 0.0f};
    hipLaunchKernelGGL(mc_channel_weight, dim3((unsigned)n_frames), dim3(MC_PAT_LANES), 0, s, (const uint32_t *)d_cw, d_rx, (const uint4 *)mc->d_cls, (unsigned)mc->Wn, mc->seed,
                       first_frame, (const uint64_t *)nullptr, (const uint32_t *)nullptr, (const mc_stratum_row *)nullptr, one,
                       mc_key_bits(key_bits), mc_threshold(mc->parity_ber), (float *)nullptr);
    LAUNCHCHK();
    return QLDPC_OK;
}

/* every argument check of qldpc_mc_strata: nothing is touched before all of them pass */
static int mc_strata_args(const qldpc_mc *mc, const qldpc_mc_strata_cfg *cfg)
{
    if (cfg->reserved[0] || cfg->reserved[1]) { qldpc_set_error("mc_strata: reserved fields %d, %d must be zero", cfg->reserved[0], cfg->reserved[1]); return QLDPC_EINVAL; }
    if (mc->soft) { qldpc_set_error("mc_strata: a channel table is in force (qldpc_mc_set_channel); error weights are weights of the BSC"); return QLDPC_ESTATE; }
    if (cfg->n_strata < 1 || cfg->n_strata > QLDPC_MC_SWEEP_MAX_POINTS) { qldpc_set_error("mc_strata: n_strata=%d outside 1 .. %d", cfg->n_strata, QLDPC_MC_SWEEP_MAX_POINTS); return QLDPC_ESIZE; }
    if (!(cfg->design_qber > 0.0 && cfg->design_qber < 0.5)) { qldpc_set_error("mc_strata: design_qber=%g outside (0, 0.5)", cfg->design_qber); return QLDPC_ESIZE; }
    if (cfg->chunk < 0 || cfg->chunk > mc->batch) { qldpc_set_error("mc_strata: chunk=%d outside [0, batch=%d]", cfg->chunk, mc->batch); return QLDPC_ESIZE; }
    if (cfg->max_frames == 0) { qldpc_set_error("mc_strata: max_frames=0"); return QLDPC_ESIZE; }
    if (!cfg->weights) { qldpc_set_error("mc_strata: a missing array (weights)"); return QLDPC_EINVAL; }
    for (int q = 0; q < cfg->n_strata; q++) {
        const int rc = mc_weight_args(mc, "mc_strata", cfg->weights[q], cfg->key_bits);
        if (rc) return rc;
    }
    return QLDPC_OK;
}

extern "C" int qldpc_mc_strata(qldpc_mc *mc, const qldpc_mc_strata_cfg *cfg, qldpc_mc_strata_result *res)
{
    if (!mc || !cfg || !res) return QLDPC_EINVAL;
    memset(res, 0, sizeof(*res));
    int rc = mc_strata_args(mc, cfg);
    if (rc || (rc = mc_sweep_reserve(mc))) return rc;
    const int P = cfg->n_strata;
    const size_t Wn = (size_t)mc->Wn;
    /* per call: the stratum rows in the layout of the point rows, and the fixed set as every stratum's erase row */
    std::vector<mc_point_row> prow((size_t)P);
    std::vector<uint32_t> erows;
    const float mag = qldpc_bsc_llr((float)cfg->design_qber);
    for (int q = 0; q < P; q++) { prow[(size_t)q].t_channel = (uint32_t)cfg->weights[q]; prow[(size_t)q].mag = mag; }
    if (mc->n_fixed) for (int q = 0; q < P; q++) erows.insert(erows.end(), mc->h_fixed.begin(), mc->h_fixed.begin() + (ptrdiff_t)Wn);
    mc->tstats.assign((size_t)P, qldpc_mc_stratum_stat());
    for (int q = 0; q < P; q++) mc->tstats[(size_t)q].weight = cfg->weights[q];
    const mc_rounds_job job = {P, cfg->chunk ? cfg->chunk : std::min(64, mc->batch), cfg->first_frame, cfg->max_frames, cfg->max_frame_errors, prow.data(),
                               mc->n_fixed ? erows.data() : nullptr, mc_key_bits(cfg->key_bits), MC_ROWS_STRATA};
    std::vector<uint64_t> last((size_t)P, 0);
    if ((rc = mc_rounds(mc, job, last.data(), res))) return rc;
    for (int q = 0; q < P; q++) {
        const mc_u64 *c = mc->h_wctr + (size_t)q * MCW_COUNTERS;
        qldpc_mc_stratum_stat &st = mc->tstats[(size_t)q];
        st.frames = c[MC_FRAMES]; st.frame_errors = c[MC_FRAME_ERRORS]; st.bit_errors = c[MC_BIT_ERRORS]; st.undetected = c[MC_UNDETECTED];
        st.not_converged = c[MC_NOT_CONVERGED]; st.iter_sum = c[MC_ITER_SUM]; st.iter_max = c[MC_ITER_MAX];
        st.channel_flips = c[MC_FLIPS]; st.channel_bits = c[MC_CHANNEL_BITS];
        st.closed_by = st.frames >= cfg->max_frames ? QLDPC_MC_CLOSED_MAX_FRAMES : QLDPC_MC_CLOSED_MAX_FE;
        st.last_round = last[(size_t)q];
    }
    return QLDPC_OK;
}

extern "C" int qldpc_mc_strata_stats(qldpc_mc *mc, qldpc_mc_stratum_stat *rows, int cap)
{
    if (!mc || cap < 0 || (cap && !rows)) return QLDPC_EINVAL;
    const size_t n = std::min((size_t)cap, mc->tstats.size());
    if (n) memcpy(rows, mc->tstats.data(), sizeof(qldpc_mc_stratum_stat) * n);
    return (int)mc->tstats.size();
}

extern "C" int qldpc_mc_strata_hist(qldpc_mc *mc, int stratum, uint64_t *hist, int cap)
{
    if (!mc || cap < 0 || (cap && !hist)) return QLDPC_EINVAL;
    if (stratum < 0 || (size_t)stratum >= mc->tstats.size()) { qldpc_set_error("mc_strata_hist: stratum=%d, the last run had %d", stratum, (int)mc->tstats.size()); return QLDPC_ESIZE; }
    if (mc->rows_owner != MC_ROWS_STRATA) { qldpc_set_error("mc_strata_hist: the device rows hold a later qldpc_mc_sweep"); return QLDPC_ESTATE; }
    const int bins = std::min(cap, mc->n_ite + 1);
    HIPCHK(hipSetDevice(mc->device));
    HIPCHK(hipStreamSynchronize(mc->dec->stream));
    if (bins) HIPCHK(hipMemcpy(hist, mc->d_whist + (size_t)stratum * (size_t)(mc->n_ite + 1), sizeof(mc_u64) * (size_t)bins, hipMemcpyDeviceToHost));
    return mc->n_ite + 1;
}
