/*
 * qldpc_mc.hip -- the Monte-Carlo loop of the reference harness (source -> encoder -> BSC -> decoder -> monitor, BS/src/main.cpp:335-393)
 * with nothing per bit crossing the host (qldpc_mc_*), and what runs around it: the puncture-pattern search, the quantised soft-output channels, the
 * QBER sweep, the same sweep over points of a table channel and the fixed-weight error strata.  The frame definition is qldpc_mc_core.h: frame i is a pure function of (seed, i).
 *
 * Three things are stated once and used by every path:
 *   mc_slots           how the slots of a launch get their frame index and their row {threshold or weight, |LLR|}: frame first + f and one row by value
 *                      (qldpc_mc_run, the search, the frame calls), or the slot tables and the rows of a round (qldpc_mc_sweep, qldpc_mc_strata:
 *                      P rows of 8 bytes, L2-resident).  mc_source, mc_channel, mc_expand_rows and mc_channel_weight take it.
 *   mc_frame_verdict,  the work of a monitor wave on one frame: be = popcount((out ^ cw) & info_mask) and, where wanted, the flips at channel VNs summed
 *   mc_tally           over the lanes by shuffles, the clamped iteration count, the syndrome verdict; and the verdicts of a wave's frames summed in
 *                      (wave-uniform) registers, then ONE atomic per wave and counter from lane 0 onto a counter row.  One counter enum: a pattern's
 *                      row is a prefix of a point's, a point's a prefix of the run's.
 *   mc_select,         the radix select of qldpc_mc_core.h by one workgroup: per key digit a histogram in LDS over keys recomputed on the fly (the pass is
 *   mc_equal_scan      the caller's, nothing is stored), lane 0 picks the bucket; and for the final pass, which walks the keys in index order a trip of 256
 *                      lanes at a time, the rank among equal keys = a running count + a shuffle prefix over the trip.
 *
 * mc_source:  one lane per info word of the packed [frame][word] layout, consecutive lanes = consecutive words of a row (the last lanes of a
 *     row run on into the next one), one Philox call per word.
 * mc_channel: one lane per codeword word: 8 Philox calls, the 32 classes of the word by two 16-byte loads from the padded class map (32 N
 *     bytes shared by all frames: L2-resident), the channel threshold from the slot's row; rx = cw ^ flips.  The lanes of word 0 also write the
 *     slot's |LLR| for qldpc_load_bits_dev.
 * mc_soft_channel: the quantised soft-output channel of a threshold table (qldpc_mc_core.h), one lane per four VNs: one Philox call, one class
 *     word, both threshold rows and the value row in LDS (3 KB, loaded once per workgroup), a halving search per VN, one 16-byte store of the
 *     four LLRs where the address allows it (scalars where N % 4 != 0 shifts a row or cuts its last quad); the rx word = the OR of the flip
 *     nibbles of the 8 lanes of a codeword word by xor-shuffles, stored by the first of them.  No atomics, no floating-point arithmetic.
 * mc_soft_channel_slots: the same lane (mc_soft_lane) on the slots of a round of qldpc_mc_sweep_tables: slot f is frame sl.frame_of(f) and draws
 *     through table sl.row[f] of the P tables of the call, so a workgroup must stay inside ONE slot to load that table into LDS once:
 *     grid = (slots, ceil(8 Wn / 256)), blockIdx.x the slot.  What the shape costs for short codes: the last workgroup of a slot is ragged (N = 1 008:
 *     8 Wn = 256 quads, one full workgroup per frame; N = 1 998: 504 quads, two workgroups, 8 lanes of the second idle; the worst case, 8 Wn = 264,
 *     leaves 248 of 512 lanes idle), and every workgroup loads its 3 KB table for at most 1 024 VNs = 4 KB of LLRs, as the workgroups of
 *     mc_soft_channel do -- but from one of P tables (P x 3 KB, L2-resident up to a thousand points) instead of always the same one.
 * mc_channel_weight: the fixed-weight channel of the error strata (the definition is qldpc_mc_core.h), one workgroup per frame slot: the select over
 *     the keys of the channel-class VNs, recomputed from the padded class map (N / 4 Philox calls per pass: at N = 65 536 the keys of a frame do not
 *     fit in LDS).  The final pass gives a lane a whole codeword word: 8 Philox calls, the 32 classes as mc_channel reads them, three masks (keys
 *     below the threshold key, keys equal to it, pinned flips); rx = cw ^ (selected | pinned) is one plain store per word, no global atomics.
 * mc_patterns: one workgroup per puncture pattern (the definition is qldpc_mc_core.h): the select over the keys of the candidates (n_cand / 4 Philox
 *     calls per pass); the final pass walks the candidates in chunks of 4 x 256 and sets the erase bits of the row it zeroed at its start.
 * mc_expand_rows: the erase row of every slot -> the frame rows qldpc_load_erasures_dev reads; 16-byte stores.  The row of a slot is row slot / F
 *     (a pattern row covers the F frames of its slots) or comes from the slot's entry in the row table of a round.
 * mc_monitor: one wave per frame (a wave strides over the frames), flips included -- plus, per frame, one add on the iteration histogram and, for a
 *     failed frame, one returning add on the slot counter of the failed-frame list.
 * mc_monitor_patterns: the waves dealt out per pattern (every frame of a wave belongs to one pattern), so the tally of a wave goes onto the counter
 *     row of that pattern; no flips, rx is not read.
 * mc_monitor_points: the waves dealt out per chunk (every frame of a wave belongs to one point or stratum), flips included: the tally onto the counter
 *     row of that point, per frame one add on the point's histogram row; no failed-frame list.
 * mc_blind_cand, mc_blind_advance, mc_blind_advance_append: the blind reconciliation rounds (qldpc_mc_blind).  One lane per word of the candidate rows
 *     chan_mask & ~known; one wave per frame for the verdict, tallied onto the counter row of the round (or of the frames that end open) together with
 *     popcount(known), and the open flag of every slot; then the open slots appended to the next pool in slot order: a workgroup takes 64 slots, counts the
 *     open flags before them, ballots its own and copies {frame index, known | asked} row by row, a wave per entry.  Plain stores, no returning atomics.
 * mc_guess_keep, mc_guess_slots, mc_guess_resolve: the guessing rounds (qldpc_mc_guess), around the two kernels of qldpc_kernels_guess.h and the blind rounds'
 *     candidate rows, verdicts and ordered append, which they reuse.  One wave per failed frame keeps the verdict of its first decode with its pool entry; one
 *     lane per trial slot writes the slot's frame index; one wave per source of a trial launch tallies the winner's decode (or, without a winner, the verdict
 *     kept) onto the row of the rescued (or open) frames and sums the trials' iterations.
 *
 * No kernel waits on another wave.  The decoder and the encoder are driven through their public calls only; qldpc_engine_int.h is read for
 * the decoder's sizes, device and stream.  On the host every buffer is allocated into the loop's ledger (qldpc_devmem.h); the three loops share the event array, the generate + load, fetch and expand helpers and the end of a round (mc_round_end).
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
#include "qldpc_guess_core.h"

#define MC_LANES 256
#define MC_MAX_WAVES 2048          /* of a monitor launch */
/* one counter row for every monitor: a pattern's row is the first MC_PATTERN_COUNTERS of it, a point's or a stratum's the first MC_POINT_COUNTERS, the
 * run's all of it */
enum { MC_FRAMES = 0, MC_FRAME_ERRORS, MC_BIT_ERRORS, MC_UNDETECTED, MC_NOT_CONVERGED, MC_ITER_SUM, MC_PATTERN_COUNTERS,
       MC_ITER_MAX = MC_PATTERN_COUNTERS, MC_FLIPS, MC_CHANNEL_BITS, MC_POINT_COUNTERS,
       MC_FAIL_SLOTS = MC_POINT_COUNTERS, MC_COUNTERS };

typedef unsigned long long mc_u64;

/* the row of an operating point {floor(qber 2^32), qldpc_bsc_llr(qber)} or of a stratum {its weight, qldpc_bsc_llr(design_qber)} */
struct mc_row { uint32_t t; float mag; };

/* how the slots of a launch get their frame index and their row: from the tables of a round (P rows of 8 bytes: L2-resident) where there are
 * tables, else frame first + f and the one row handed over by value */
struct mc_slots {
    const uint64_t *frame; uint64_t first;      /* frame != NULL: frame[f] */
    const uint32_t *row; const mc_row *rows;    /* row != NULL: rows[row[f]] */
    mc_row one;
    __device__ uint64_t frame_of(unsigned f) const { return frame ? frame[f] : first + f; }
    __device__ mc_row row_of(unsigned f) const { return row ? rows[row[f]] : one; }
    /* for mc_expand_rows, which needs the index alone: without a table F consecutive slots share a row */
    __device__ unsigned row_index(unsigned f, unsigned F) const { return row ? row[f] : f / F; }
};

__global__ __launch_bounds__(MC_LANES) void mc_source(uint32_t *__restrict__ info, unsigned total, unsigned Wk, int K, uint64_t seed, mc_slots sl)
{
    const unsigned i = blockIdx.x * MC_LANES + threadIdx.x;
    if (i >= total) return;
    const unsigned f = i / Wk, j = i - f * Wk;
    info[i] = mc_info_word(seed, sl.frame_of(f), j, K);
}

/* the BSC of the slot's row: its threshold for the channel VNs, its |LLR| for qldpc_load_bits_dev (llr_mag may be NULL) */
__global__ __launch_bounds__(MC_LANES) void mc_channel(const uint32_t *__restrict__ cw, uint32_t *__restrict__ rx, const uint4 *__restrict__ cls,
                                                       unsigned total, unsigned Wn, uint64_t seed, mc_slots sl, uint32_t t_pinned, float *__restrict__ llr_mag)
{
    const unsigned i = blockIdx.x * MC_LANES + threadIdx.x;
    if (i >= total) return;
    const unsigned f = i / Wn, w = i - f * Wn;
    const mc_row r = sl.row_of(f);
    const uint4 a = cls[2u * w], b = cls[2u * w + 1u];
    const uint32_t cls4[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    rx[i] = cw[i] ^ mc_flip_word(seed, sl.frame_of(f), w, cls4, r.t, t_pinned);
    if (w == 0 && llr_mag) llr_mag[f] = r.mag;
}

/* the table of a workgroup of the two soft channels, in LDS; load() is called by every lane of the workgroup and ends behind a barrier */
struct mc_soft_lds {
    uint32_t thr[2][MC_SOFT_MAX_LEVELS];
    float value[MC_SOFT_MAX_LEVELS];
    uint32_t live[2];
    __device__ void load(const mc_soft_table *__restrict__ tab)
    {
        static_assert(MC_LANES == MC_SOFT_MAX_LEVELS, "the soft channels load one table entry per lane");
        const unsigned t = threadIdx.x;
        thr[0][t] = t < MC_SOFT_MAX_LEVELS - 1 ? tab->thr[0][t] : 0xFFFFFFFFu;
        thr[1][t] = t < MC_SOFT_MAX_LEVELS - 1 ? tab->thr[1][t] : 0xFFFFFFFFu;
        value[t] = tab->value[t];
        if (t < 2) live[t] = tab->live[t];
        __syncthreads();
    }
};

/* quad q (of Qn = 8 Wn: the padding past N is QLDPC_VN_PUNCTURED: LLR 0, no flip, nothing stored) of frame slot f, which is frame `frame`: the
 * four LLRs by ONE 16-byte store where the address allows it, scalars where N % 4 != 0 shifts the row or cuts its last quad; the rx word (rx may be
 * NULL) = the OR of the flip nibbles of the 8 lanes of a codeword word, stored by the first of them.  The 8 lanes of a word call it together. */
__device__ static inline void mc_soft_lane(const mc_soft_lds &tab, const uint32_t *__restrict__ cw, uint32_t *__restrict__ rx, float *__restrict__ llr,
                                           const uint32_t *__restrict__ cls4, unsigned f, unsigned q, unsigned Qn, unsigned N, uint64_t seed, uint64_t frame,
                                           uint32_t t_pinned)
{
    const unsigned w = (f * Qn + q) >> 3, sh = 28u - 4u * (q & 7u);
    const uint32_t c = cw[w];
    float l[4];
    uint32_t flips = mc_soft_quad(seed, frame, q, cls4[q], (c >> sh) & 0xfu, tab.thr[0], tab.live[0], tab.thr[1], tab.live[1], tab.value, t_pinned, l) << sh;
    const unsigned v = 4u * q;
    if (v < N) {
        float *p = llr + (size_t)f * N + v;
        if (v + 4u <= N && ((uintptr_t)p & 15u) == 0) *(float4 *)p = make_float4(l[0], l[1], l[2], l[3]);
        else for (unsigned b = 0; b < 4u && v + b < N; b++) p[b] = l[b];
    }
    if (!rx) return;
    for (int s = 1; s < 8; s <<= 1) flips |= (uint32_t)__shfl_xor((int)flips, s, 64);
    if ((q & 7u) == 0) rx[w] = c ^ flips;
}

/* one table for every frame: rows of 8 Wn quads, total = n 8 Wn lanes: a multiple of 8, as the block size is, so the 8 lanes of a codeword
 * word leave or stay together and the shuffles of mc_soft_lane see all of them.  rx may be NULL. */
__global__ __launch_bounds__(MC_LANES) void mc_soft_channel(const uint32_t *__restrict__ cw, uint32_t *__restrict__ rx, float *__restrict__ llr,
                                                            const uint32_t *__restrict__ cls4, const mc_soft_table *__restrict__ tab, unsigned total,
                                                            unsigned Qn, unsigned N, uint64_t seed, uint64_t first, uint32_t t_pinned)
{
    __shared__ mc_soft_lds lds;
    lds.load(tab);
    const unsigned i = blockIdx.x * MC_LANES + threadIdx.x;
    if (i >= total) return;
    const unsigned f = i / Qn;
    mc_soft_lane(lds, cw, rx, llr, cls4, f, i - f * Qn, Qn, N, seed, first + f, t_pinned);
}

/* a table per slot: grid = (slots, ceil(Qn / MC_LANES)) -- the slots in x, whose limit a batch cannot reach; y stays below 65 536 up to N = 2^26 --;
 * slot blockIdx.x is frame sl.frame_of(slot) through table tabs[sl.row[slot]] (sl has both tables).  Qn = 8 Wn is a multiple of 8, so the 8 lanes
 * of a codeword word leave or stay together here too. */
__global__ __launch_bounds__(MC_LANES) void mc_soft_channel_slots(const uint32_t *__restrict__ cw, uint32_t *__restrict__ rx, float *__restrict__ llr,
                                                                  const uint32_t *__restrict__ cls4, const mc_soft_table *__restrict__ tabs, unsigned Qn,
                                                                  unsigned N, uint64_t seed, mc_slots sl, uint32_t t_pinned)
{
    __shared__ mc_soft_lds lds;
    const unsigned f = blockIdx.x, q = blockIdx.y * MC_LANES + threadIdx.x;
    lds.load(tabs + sl.row[f]);
    if (q >= Qn) return;
    mc_soft_lane(lds, cw, rx, llr, cls4, f, q, Qn, N, seed, sl.frame_of(f), t_pinned);
}

__device__ static inline unsigned mc_wave_sum(unsigned x)
{
    for (int s = 32; s > 0; s >>= 1) x += __shfl_xor(x, s, 64);
    return x;
}

/* ---- the monitors: one verdict per frame, one tally per wave ---- */

/* what a monitor reads of a decoded batch, the same for all three */
struct mc_decoded {
    const uint32_t *out, *cw, *rx, *info_mask, *chan_mask;      /* [n][Wn] decoded, sent and received rows; [Wn] masks of the info and the channel VNs */
    const int *iters, *ok;
    unsigned Wn; int n_ite;
};

struct mc_verdict { unsigned be, fl; int it; bool good; };

/* frame f by one wave, the result in every lane: be = popcount((out ^ cw) & info_mask), FLIPS: fl = the flips at channel VNs (else rx is not read
 * and fl = 0), the iteration count clamped to the histogram */
template <bool FLIPS> __device__ static inline mc_verdict mc_frame_verdict(const mc_decoded &d, unsigned f)
{
    const size_t row = (size_t)f * d.Wn;
    unsigned be = 0, fl = 0;
    for (unsigned w = threadIdx.x & 63u; w < d.Wn; w += 64u) {
        const uint32_t c = d.cw[row + w];
        be += (unsigned)__popc((d.out[row + w] ^ c) & d.info_mask[w]);
        if (FLIPS) fl += (unsigned)__popc((d.rx[row + w] ^ c) & d.chan_mask[w]);
    }
    be = mc_wave_sum(be);
    if (FLIPS) fl = mc_wave_sum(fl);
    return {be, fl, min(max(d.iters[f], 0), d.n_ite), d.ok[f] != 0};
}

/* the verdicts of a wave's frames summed in (wave-uniform) registers, then ONE atomic per wave and counter from lane 0 onto a counter row:
 * FLIPS = false the MC_PATTERN_COUNTERS of a pattern, true the MC_POINT_COUNTERS of a point or of the run */
template <bool FLIPS> struct mc_tally {
    mc_u64 frames = 0, be = 0, fe = 0, ud = 0, nc = 0, it = 0, mx = 0, fl = 0;
    __device__ void add(const mc_verdict &v)
    {
        frames++; be += v.be; fl += v.fl; it += (mc_u64)v.it;
        mx = max(mx, (mc_u64)v.it);
        fe += v.be > 0; ud += v.good && v.be > 0; nc += !v.good;
    }
    __device__ void flush(mc_u64 *row, unsigned channel_vns = 0) const
    {
        if ((threadIdx.x & 63u) != 0 || frames == 0) return;
        atomicAdd(row + MC_FRAMES, frames);
        atomicAdd(row + MC_ITER_SUM, it);
        if (FLIPS) {
            atomicMax(row + MC_ITER_MAX, mx);
            atomicAdd(row + MC_CHANNEL_BITS, frames * channel_vns);
            if (fl) atomicAdd(row + MC_FLIPS, fl);
        }
        if (be) atomicAdd(row + MC_BIT_ERRORS, be);
        if (fe) atomicAdd(row + MC_FRAME_ERRORS, fe);
        if (ud) atomicAdd(row + MC_UNDETECTED, ud);
        if (nc) atomicAdd(row + MC_NOT_CONVERGED, nc);
    }
};

/* one wave per frame (a wave strides over the n frames); per frame one add on the histogram and, for a failed frame, one returning add on the
 * slot counter of the failed-frame list */
__global__ __launch_bounds__(MC_LANES) void mc_monitor(mc_decoded d, unsigned n, uint64_t first, unsigned channel_vns, mc_u64 *__restrict__ ctr,
                                                       mc_u64 *__restrict__ hist, mc_u64 *__restrict__ fails, unsigned fail_cap)
{
    const unsigned lane = threadIdx.x & 63u, waves = gridDim.x * (MC_LANES / 64);
    mc_tally<true> sum;
    for (unsigned f = blockIdx.x * (MC_LANES / 64) + (threadIdx.x >> 6); f < n; f += waves) {
        const mc_verdict v = mc_frame_verdict<true>(d, f);
        sum.add(v);
        if (lane == 0) {
            atomicAdd(hist + v.it, 1ull);
            if (v.be > 0) {
                const mc_u64 slot = atomicAdd(ctr + MC_FAIL_SLOTS, 1ull);
                if (slot < fail_cap) fails[slot] = first + f;
            }
        }
    }
    sum.flush(ctr, channel_vns);
}

/* wpp waves per pattern (<= F): wave (pat, sub) takes frames sub, sub + wpp, ... of the F frames of pattern slot pat, so every frame of a wave
 * belongs to one pattern, whose counter row [MC_PATTERN_COUNTERS] the wave adds to; rx is not read */
__global__ __launch_bounds__(MC_LANES) void mc_monitor_patterns(mc_decoded d, unsigned n_pat, unsigned F, unsigned wpp, mc_u64 *__restrict__ rows)
{
    const unsigned wid = blockIdx.x * (MC_LANES / 64) + (threadIdx.x >> 6);
    if (wid >= n_pat * wpp) return;
    const unsigned pat = wid / wpp, sub = wid - pat * wpp;
    mc_tally<false> sum;
    for (unsigned k = sub; k < F; k += wpp) sum.add(mc_frame_verdict<false>(d, pat * F + k));
    sum.flush(rows + (size_t)pat * MC_PATTERN_COUNTERS);
}

/* wpc waves per chunk: wave (chunk, sub) takes frames sub, sub + wpc, ... of the chunk_len frames that start at slot chunk_start; a chunk
 * belongs to one point, whose counter row [MC_POINT_COUNTERS] and histogram row [n_ite + 1] the wave adds to; no failed-frame list */
__global__ __launch_bounds__(MC_LANES) void mc_monitor_points(mc_decoded d, unsigned n_chunks, unsigned wpc, const uint32_t *__restrict__ chunk_point,
                                                              const uint32_t *__restrict__ chunk_start, const uint32_t *__restrict__ chunk_len,
                                                              unsigned channel_vns, mc_u64 *__restrict__ rows, mc_u64 *__restrict__ hists)
{
    const unsigned lane = threadIdx.x & 63u, wid = blockIdx.x * (MC_LANES / 64) + (threadIdx.x >> 6);
    if (wid >= n_chunks * wpc) return;
    const unsigned c = wid / wpc, sub = wid - c * wpc, point = chunk_point[c], start = chunk_start[c], len = chunk_len[c];
    mc_u64 *hist = hists + (size_t)point * (size_t)(d.n_ite + 1);
    mc_tally<true> sum;
    for (unsigned k = sub; k < len; k += wpc) {
        const mc_verdict v = mc_frame_verdict<true>(d, start + k);
        sum.add(v);
        if (lane == 0) atomicAdd(hist + v.it, 1ull);
    }
    sum.flush(rows + (size_t)point * MC_POINT_COUNTERS, channel_vns);
}

/* ---- blind reconciliation rounds: candidate rows, verdicts per round, ordered append to the next pool ---- */

/* the counter row of a round: a point's row and the key bits its frames asked for */
enum { MC_DISCLOSED = MC_POINT_COUNTERS, MC_BLIND_COUNTERS };
#define MC_APPEND_SLOTS 64         /* slots of a launch per workgroup of mc_blind_advance_append: one ballot */

/* cand[f][w] = chan_mask[w] & ~known[f][w]: the channel VNs frame f does not know yet (known == NULL: it knows none); take[f] = the frame is open */
__global__ __launch_bounds__(MC_LANES) void mc_blind_cand(const uint32_t *__restrict__ chan_mask, const uint32_t *__restrict__ known, const int *__restrict__ ok,
                                                          uint32_t *__restrict__ cand, int *__restrict__ take, unsigned total, unsigned Wn)
{
    const unsigned i = blockIdx.x * MC_LANES + threadIdx.x;
    if (i >= total) return;
    const unsigned f = i / Wn, w = i - f * Wn;
    cand[i] = chan_mask[w] & ~(known ? known[i] : 0u);
    if (w == 0) take[f] = !ok[f];
}

/* one wave per frame (a wave strides over the n frames of a launch at one level).  A frame that closed is tallied onto row_closed; an open one onto
 * row_open where this was the last round (row_open != NULL), else it goes on and is tallied when it ends.  The tally of a row includes the known bits
 * of its frames (known == NULL: none).  open[f] = the frame is open, for mc_blind_advance_append.  level_count != NULL: the pool this launch was taken from
 * now holds `left` entries */
__global__ __launch_bounds__(MC_LANES) void mc_blind_advance(mc_decoded d, unsigned n, const uint32_t *__restrict__ known, unsigned channel_vns,
                                                             mc_u64 *__restrict__ row_closed, mc_u64 *__restrict__ row_open, int *__restrict__ open,
                                                             mc_u64 *__restrict__ level_count, mc_u64 left)
{
    const unsigned lane = threadIdx.x & 63u, waves = gridDim.x * (MC_LANES / 64);
    mc_tally<true> closed, ended;
    mc_u64 asked_closed = 0, asked_ended = 0;
    for (unsigned f = blockIdx.x * (MC_LANES / 64) + (threadIdx.x >> 6); f < n; f += waves) {
        const mc_verdict v = mc_frame_verdict<true>(d, f);      /* the same in every lane */
        if (lane == 0) open[f] = !v.good;
        if (!v.good && !row_open) continue;
        unsigned k = 0;
        if (known) {
            for (unsigned w = lane; w < d.Wn; w += 64u) k += (unsigned)__popc(known[(size_t)f * d.Wn + w]);
            k = mc_wave_sum(k);
        }
        if (v.good) { closed.add(v); asked_closed += k; }
        else { ended.add(v); asked_ended += k; }
    }
    closed.flush(row_closed, channel_vns);
    if (row_open) ended.flush(row_open, channel_vns);
    if (lane == 0 && asked_closed) atomicAdd(row_closed + MC_DISCLOSED, asked_closed);
    if (lane == 0 && asked_ended) atomicAdd(row_open + MC_DISCLOSED, asked_ended);
    if (level_count && blockIdx.x == 0 && threadIdx.x == 0) *level_count = left;
}

/* the open slots of a launch, in ascending slot order, become entries base, base + 1, ... of a pool (or of the list of the frames that end open):
 * dst_frame[e] = the slot's frame index, dst_known[e][Wn] = known | weak of the slot (either may be NULL: no bits).  Workgroup b takes slots
 * 64 b .. 64 b + 63: its lanes count the open flags before them, every wave ballots the 64 flags, and wave j copies the open slots number j, j + 4, ...
 * of them.  Entries at `cap` and beyond are not written (the pools never get there, see mc_blind_next; the list keeps the first cap).  The last
 * workgroup writes the new count, base + the open slots of the launch */
__global__ __launch_bounds__(MC_LANES) void mc_blind_advance_append(const int *__restrict__ open, unsigned n, mc_slots sl, const uint32_t *__restrict__ known,
                                                                    const uint32_t *__restrict__ weak, unsigned Wn, uint64_t *__restrict__ dst_frame,
                                                                    uint32_t *__restrict__ dst_known, mc_u64 base, mc_u64 cap, mc_u64 *__restrict__ dst_count)
{
    static_assert(MC_APPEND_SLOTS == 64, "mc_blind_advance_append ballots one wave of flags");
    __shared__ unsigned part[MC_LANES / 64];
    const unsigned t = threadIdx.x, lane = t & 63u, wave = t >> 6, f0 = blockIdx.x * MC_APPEND_SLOTS;
    unsigned c = 0;
    for (unsigned i = t; i < f0; i += MC_LANES) c += open[i] != 0;
    c = mc_wave_sum(c);
    if (lane == 0) part[wave] = c;
    __syncthreads();
    unsigned before = 0;
    for (unsigned w = 0; w < MC_LANES / 64; w++) before += part[w];
    const unsigned long long flags = __ballot(f0 + lane < n && open[min(f0 + lane, n - 1u)] != 0);
    unsigned k = 0;
    for (unsigned long long m = flags; m; m &= m - 1ull, k++) {
        if ((k & (MC_LANES / 64 - 1u)) != wave) continue;
        const unsigned f = f0 + (unsigned)__ffsll(m) - 1u;
        const mc_u64 e = base + before + k;
        if (e >= cap) continue;
        const size_t src = (size_t)f * Wn, dst = (size_t)e * Wn;
        for (unsigned w = lane; w < Wn; w += 64u) dst_known[dst + w] = (known ? known[src + w] : 0u) | (weak ? weak[src + w] : 0u);
        if (lane == 0) dst_frame[e] = sl.frame_of(f);
    }
    if (blockIdx.x == gridDim.x - 1 && t == 0) *dst_count = base + before + (unsigned)__popcll(flags);
}

/* ---- guessing rounds: the verdicts kept with a pooled frame, the slot table of a trial launch, the verdicts of its sources ---- */

/* the counter rows of a call [MC_GUESS_ROWS][MC_BLIND_COUNTERS] (closed at once, rescued, open; nothing is disclosed), then the counts and sums */
enum { MC_GUESS_ROWS = 3, MC_G_POOL = MC_GUESS_ROWS * MC_BLIND_COUNTERS, MC_G_OPEN, MC_G_N_OK, MC_G_AMBIGUOUS, MC_G_TRIAL_ITER, MC_GUESS_WORDS };
#define MC_GUESS_VERDICT 4         /* words of the verdict kept with a pooled frame: be, fl, it, spare */
static_assert(MC_GUESS_MAX_BITS == QLDPC_GUESS_MAX_BITS && GS_MAX_BITS == QLDPC_GUESS_MAX_BITS, "one limit on the guess bits");

/* one wave per frame of a fresh launch: verd[f] = the verdict of a failed frame's decode, what its row shows should it stay open */
__global__ __launch_bounds__(MC_LANES) void mc_guess_keep(mc_decoded d, unsigned n, uint32_t *__restrict__ verd)
{
    const unsigned lane = threadIdx.x & 63u, waves = gridDim.x * (MC_LANES / 64);
    for (unsigned f = blockIdx.x * (MC_LANES / 64) + (threadIdx.x >> 6); f < n; f += waves) {
        if (d.ok[f] != 0) continue;      /* the same in every lane */
        const mc_verdict v = mc_frame_verdict<true>(d, f);
        if (lane == 0) *(uint4 *)(verd + (size_t)f * MC_GUESS_VERDICT) = make_uint4(v.be, v.fl, (unsigned)v.it, 0u);
    }
}

/* trial slot s T + t is the frame of source s */
__global__ __launch_bounds__(MC_LANES) void mc_guess_slots(const uint64_t *__restrict__ src_frame, uint64_t *__restrict__ slot_frame, unsigned total, int g)
{
    const unsigned i = blockIdx.x * MC_LANES + threadIdx.x;
    if (i < total) slot_frame[i] = src_frame[i >> g];
}

/* one wave per source of a trial launch (a wave strides over the n_src sources), behind qk_guess_pick: a source with a winner is tallied onto
 * row_rescued by the verdict of the winner's decode, with its n_ok and its ambiguity flag onto the sums; one without onto row_open by the verdict
 * kept from its first decode (verd[s]).  The clamped iterations of all its T trials go onto the sums.  open[s] = no winner, for
 * mc_blind_advance_append; the pool the sources were taken from now holds `left` entries */
__global__ __launch_bounds__(MC_LANES) void mc_guess_resolve(mc_decoded d, unsigned n_src, int g, const int *__restrict__ winner, const int *__restrict__ n_ok,
                                                             const int *__restrict__ ambiguous, const uint32_t *__restrict__ verd, unsigned channel_vns,
                                                             mc_u64 *__restrict__ row_rescued, mc_u64 *__restrict__ row_open, mc_u64 *__restrict__ sums,
                                                             int *__restrict__ open, mc_u64 left)
{
    const unsigned lane = threadIdx.x & 63u, waves = gridDim.x * (MC_LANES / 64), T = 1u << g;
    mc_tally<true> rescued, ended;
    mc_u64 nok = 0, amb = 0, it = 0;
    for (unsigned s = blockIdx.x * (MC_LANES / 64) + (threadIdx.x >> 6); s < n_src; s += waves) {
        unsigned its = 0;
        for (unsigned t = lane; t < T; t += 64u) its += (unsigned)min(max(d.iters[s * T + t], 0), d.n_ite);
        it += mc_wave_sum(its);
        const int w = winner[s];      /* the same in every lane */
        if (lane == 0) open[s] = w < 0;
        if (w >= 0) {
            rescued.add(mc_frame_verdict<true>(d, s * T + (unsigned)w));
            nok += (mc_u64)n_ok[s]; amb += ambiguous[s] != 0;
        } else {
            const uint4 k = *(const uint4 *)(verd + (size_t)s * MC_GUESS_VERDICT);
            ended.add(mc_verdict{k.x, k.y, (int)k.z, false});
        }
    }
    rescued.flush(row_rescued, channel_vns);
    ended.flush(row_open, channel_vns);
    if (lane == 0) {
        if (nok) atomicAdd(sums + (MC_G_N_OK - MC_G_POOL), nok);
        if (amb) atomicAdd(sums + (MC_G_AMBIGUOUS - MC_G_POOL), amb);
        if (it) atomicAdd(sums + (MC_G_TRIAL_ITER - MC_G_POOL), it);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) sums[0] = left;
}

/* ---- the radix select of qldpc_mc_core.h by one workgroup of MC_PAT_LANES lanes ---- */
#define MC_PAT_LANES 256
static_assert(MC_PAT_LANES == MC_SEL_BINS, "mc_select clears one histogram bin per lane");

struct mc_selected { uint32_t T, r; };      /* the threshold key, and how many of the keys equal to it are taken */

/* rank k (1-based) among keys of key_bits bits, in every lane: per digit a histogram in LDS, lane 0 picks the bucket, the choice goes round through
 * LDS.  pass(count) is one histogram pass of the whole workgroup: it calls count(key) once for every key, recomputed on the fly (nothing is
 * stored).  k = 0, uniform over the workgroup: no pass, T = 0, r = 0.  Every lane of the workgroup calls it; it ends behind a barrier. */
template <typename Pass> __device__ static inline mc_selected mc_select(int key_bits, uint32_t k, Pass pass)
{
    __shared__ uint32_t hist[MC_SEL_BINS];
    __shared__ uint32_t sel[2];
    const unsigned t = threadIdx.x;
    uint32_t prefix = 0, mask = 0;
    if (k == 0) return {0u, 0u};
    for (int shift = mc_select_top_shift(key_bits); shift >= 0; shift -= MC_SEL_BITS) {
        hist[t] = 0u;
        __syncthreads();
        pass([&](uint32_t key) { if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & (MC_SEL_BINS - 1)], 1u); });
        __syncthreads();
        if (t == 0) { uint32_t kk = k; sel[0] = mc_select_digit(hist, &kk); sel[1] = kk; }
        __syncthreads();
        prefix |= sel[0] << shift; k = sel[1];
        mask |= (uint32_t)(MC_SEL_BINS - 1) << shift;
    }
    return {prefix, k};
}

/* the final pass walks the keys in index order, MC_PAT_LANES lanes per trip: before(mine) = the keys equal to T that precede this lane's `mine`
 * of them, over all the trips so far = a running count + a shuffle prefix over the trip.  Every lane calls it once per trip. */
struct mc_equal_scan {
    unsigned base = 0;
    __device__ unsigned before(unsigned mine)
    {
        __shared__ unsigned wave_eq[MC_PAT_LANES / 64];
        const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
        unsigned incl = mine;
        for (unsigned s = 1; s < 64u; s <<= 1) { const unsigned v = __shfl_up(incl, s, 64); if (lane >= s) incl += v; }
        __syncthreads();      /* the trip before has read wave_eq */
        if (lane == 63u) wave_eq[wave] = incl;
        __syncthreads();
        unsigned b = base + incl - mine;
        for (unsigned w = 0; w < MC_PAT_LANES / 64; w++) { if (w < wave) b += wave_eq[w]; base += wave_eq[w]; }
        return b;
    }
};

/* ---- puncture patterns ---- */

/* rows[blockIdx.x][Wn] = the erase row of pattern first + blockIdx.x; cand[n_cand] ascending VNs below 32 Wn; n_punct <= n_cand; key_bits 1 .. 32 */
__global__ __launch_bounds__(MC_PAT_LANES) void mc_patterns(uint32_t *__restrict__ rows, const int *__restrict__ cand, unsigned n_cand, unsigned n_punct,
                                                            int key_bits, unsigned Wn, uint64_t seed, uint64_t first)
{
    const unsigned t = threadIdx.x;
    const uint64_t p = first + blockIdx.x;
    uint32_t *row = rows + (size_t)blockIdx.x * Wn;
    for (unsigned w = t; w < Wn; w += MC_PAT_LANES) row[w] = 0u;
    if (n_punct == 0) return;
    const unsigned blocks = (n_cand + 3u) / 4u;
    uint32_t u[4];
    const mc_selected s = mc_select(key_bits, n_punct, [&](auto count) {      /* n_cand / 4 Philox calls per pass */
        for (unsigned q = t; q < blocks; q += MC_PAT_LANES) {
            mc_pattern_keys(seed, p, q, key_bits, u);
            for (unsigned b = 0; b < 4; b++)
                if (4u * q + b < n_cand) count(u[b]);
        }
    });
    /* the barriers of the select also order the zeroing of the row before the bits set below */
    mc_equal_scan scan;
    for (unsigned q0 = 0; q0 < blocks; q0 += MC_PAT_LANES) {
        const unsigned q = q0 + t;
        unsigned mine = 0;
        if (q < blocks) {
            mc_pattern_keys(seed, p, q, key_bits, u);
            for (unsigned b = 0; b < 4; b++) mine += 4u * q + b < n_cand && u[b] == s.T;
        }
        unsigned before = scan.before(mine);
        if (q < blocks)
            for (unsigned b = 0; b < 4; b++) {
                if (4u * q + b >= n_cand) break;
                if (mc_pattern_takes(u[b], s.T, s.r, before)) { const unsigned v = (unsigned)cand[4u * q + b]; atomicOr(&row[v >> 5], 0x80000000u >> (v & 31u)); }
                before += u[b] == s.T;
            }
    }
}

/* frames[slot][Wn] = pat[the slot's row][Wn] for the `total` words of the slots, four words per lane; without a row table F slots per row */
__global__ __launch_bounds__(MC_LANES) void mc_expand_rows(const uint32_t *__restrict__ pat, uint32_t *__restrict__ frames, unsigned total, unsigned Wn, mc_slots sl,
                                                           unsigned F)
{
    const unsigned i = (blockIdx.x * MC_LANES + threadIdx.x) * 4u;
    if (i >= total) return;
    uint32_t w[4] = {0u, 0u, 0u, 0u};
    for (unsigned j = 0; j < 4; j++)
        if (i + j < total) { const unsigned slot = (i + j) / Wn, word = (i + j) - slot * Wn; w[j] = pat[(size_t)sl.row_index(slot, F) * Wn + word]; }
    if (i + 4u <= total) *(uint4 *)(frames + i) = make_uint4(w[0], w[1], w[2], w[3]);
    else for (unsigned j = 0; i + j < total; j++) frames[i + j] = w[j];
}

/* ---- fixed-weight error strata ---- */

/* rx[slot][Wn] = cw[slot][Wn] ^ the flips of the fixed-weight frame of the slot, its weight = the t of the slot's row; gridDim.x = the slots.
 * cls = the padded class map (past N: QLDPC_VN_PUNCTURED, never selected); key_bits 1 .. 32; weight <= the channel VNs of cls */
__global__ __launch_bounds__(MC_PAT_LANES) void mc_channel_weight(const uint32_t *__restrict__ cw, uint32_t *__restrict__ rx, const uint4 *__restrict__ cls, unsigned Wn,
                                                                  uint64_t seed, mc_slots sl, int key_bits, uint32_t t_pinned, float *__restrict__ llr_mag)
{
    const unsigned t = threadIdx.x, slot = blockIdx.x;
    const uint64_t frame = sl.frame_of(slot);
    const mc_row st = sl.row_of(slot);
    const uint32_t *cls4 = (const uint32_t *)cls;
    const unsigned quads = 8u * Wn;
    const mc_selected s = mc_select(key_bits, st.t, [&](auto count) {      /* the keys of the channel VNs: N / 4 Philox calls per pass */
        uint32_t u[4];
        for (unsigned g = t; g < quads; g += MC_PAT_LANES) {
            const uint32_t m = mc_weight_quad(seed, frame, g, cls4[g], 0u, u);
            for (unsigned b = 0; b < 4; b++)
                if ((m >> b) & 1u) count(u[b] >> (32 - key_bits));
        }
    });
    const size_t row = (size_t)slot * Wn;
    mc_equal_scan scan;
    for (unsigned w0 = 0; w0 < Wn; w0 += MC_PAT_LANES) {
        const unsigned w = w0 + t;
        uint32_t less = 0, eq = 0, pin = 0;
        if (w < Wn) {
            const uint4 a = cls[2u * w], b = cls[2u * w + 1u];
            const uint32_t c4[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
            mc_weight_masks(seed, frame, w, c4, key_bits, s.T, t_pinned, &less, &eq, &pin);
        }
        const unsigned before = scan.before((unsigned)__popc(eq));
        if (w < Wn) rx[row + w] = cw[row + w] ^ (mc_weight_take(less, eq, s.T, s.r, before) | pin);
    }
    if (t == 0 && llr_mag) llr_mag[slot] = st.mag;
}

/* ------------------------------------------------------------------ host ---- */

struct qldpc_mc {
    qldpc_decoder *dec; qldpc_encoder *enc;      /* not owned */
    int N, K, Wn, Wk, n_ite, batch, fail_cap, device;
    unsigned channel_vns;
    uint64_t seed; double parity_ber;
    dm_ledger mem;                                 /* everything the loop allocates (qldpc_devmem.h) */
    uint8_t *d_cls;                    /* [32 Wn] padded class map: qldpc_load_bits_dev reads its first N bytes, mc_channel all of it */
    uint32_t *d_info_mask, *d_chan_mask, *d_info, *d_cw, *d_rx, *d_out;
    float *d_mag; int *d_iters, *d_ok;
    mc_u64 *d_ctr;                     /* MC_COUNTERS counters, n_ite + 1 histogram bins, fail_cap frame indices */
    mc_u64 *h_ctr;                     /* pinned, MC_COUNTERS */
    hipEvent_t ev[9];                  /* the stage boundaries of a batch or a round, in the order of the loop's stage list */
    /* puncture patterns and the search over them; the device side is allocated at first use (mc_search_reserve) */
    std::vector<uint8_t> h_cls;        /* [N] the class map, for the default candidates */
    std::vector<int> cand;             /* the candidate VNs, ascending */
    bool cand_dirty, search_ready;
    int n_fixed;                       /* VNs of the fixed puncture set of qldpc_mc_run (0 = none) */
    int *d_cand;                       /* [N] */
    uint32_t *d_pat, *d_erase, *d_fixed;   /* [batch][Wn] pattern rows, [batch][Wn] frame rows, [Wn] the fixed set */
    mc_u64 *d_rows, *h_rows;           /* [batch][MC_PATTERN_COUNTERS] counter rows of a round; pinned copy */
    std::vector<qldpc_mc_pattern_stat> stats;   /* of the last search */
    /* a quantised soft-output channel in place of the BSC; the device side is allocated by the first accepted qldpc_mc_set_channel */
    bool soft;                         /* a table is in force */
    int source;                        /* QLDPC_MC_SOURCE_* */
    mc_soft_table *d_tab;
    float *d_llr;                      /* [batch][N], what qldpc_load_llr_dev takes; shared with the table sweep, allocated by whichever comes first */
    mc_soft_table *d_tabs;             /* [tabs_cap] the tables of the points of a qldpc_mc_sweep_tables call, grown to the largest P so far */
    size_t tabs_cap;
    /* the QBER sweep; the device side is allocated by the first qldpc_mc_sweep (mc_sweep_reserve) */
    bool sweep_ready;
    std::vector<uint32_t> h_fixed;     /* [Wn] the fixed set of qldpc_mc_set_puncture (empty = none): a point's erase row = this OR its prefix */
    mc_u64 *d_slots, *h_slots;         /* the tables of a round and their pinned copy: [batch] 64-bit frame indices, then [batch] 32-bit words each
                                          of slot -> point, chunk -> point, chunk -> first slot, chunk -> frames */
    mc_row *d_points;                  /* [QLDPC_MC_SWEEP_MAX_POINTS] */
    uint32_t *d_prows;                 /* [QLDPC_MC_SWEEP_MAX_POINTS][Wn] the erase rows of the points */
    mc_u64 *d_wctr, *h_wctr, *d_whist; /* [QLDPC_MC_SWEEP_MAX_POINTS][MC_POINT_COUNTERS] counter rows, pinned copy; [..][n_ite + 1] histogram rows */
    std::vector<qldpc_mc_point_stat> wstats;    /* of the last sweep */
    /* the error strata run the sweep's rounds on the sweep's tables and device rows; rows_owner says whose counters and histograms those hold */
    int rows_owner;                    /* MC_ROWS_* */
    std::vector<qldpc_mc_stratum_stat> tstats;  /* of the last strata run */
    /* the blind reconciliation rounds; the device side is allocated by the first qldpc_mc_blind (mc_blind_reserve), the pools for the deepest max_rounds so far */
    bool blind_ready;
    int blind_levels;                  /* the levels the pools are allocated for */
    uint64_t *d_pframe;                /* [blind_levels][2 batch - 1] frame indices, pool r at row r - 1 */
    uint32_t *d_pknown;                /* [blind_levels][2 batch - 1][Wn] known rows */
    uint64_t *d_oframe; uint32_t *d_oknown;   /* [fail_cap], [fail_cap][Wn]: the frames that ended open, in the order of the launches */
    uint32_t *d_bcand, *d_bweak;       /* [batch][Wn] candidate rows, asked rows */
    int *d_btake, *d_bopen;            /* [batch] what qldpc_fetch_weakest_dev takes, the open flags of a launch */
    mc_u64 *d_bctr, *h_bctr;           /* MC_BLIND_WORDS: the counter rows of a call [R + 2][MC_BLIND_COUNTERS], then R + 2 counts: [r] = the entries of pool r
                                          (1 .. R), [R + 1] = the frames that ended open; pinned copy */
    std::vector<qldpc_mc_blind_round_stat> bstats;   /* of the last blind call */
    /* the guessing rounds; the device side is allocated by the first qldpc_mc_guess (mc_guess_reserve), for every g.  The launch scratch d_bcand, d_bweak,
       d_btake, d_bopen is shared with the blind rounds, allocated by whichever comes first */
    bool guess_ready;
    uint64_t *d_gframe;                /* [MC_GUESS_POOL_CAP] the pool: frame indices, ... */
    uint32_t *d_gweak, *d_ghard, *d_gverd;   /* ... [cap][Wn] guess rows, [cap][Wn] hard rows, [cap][MC_GUESS_VERDICT] the verdicts of the first decodes */
    uint32_t *d_gkeep;                 /* [batch][MC_GUESS_VERDICT] the verdicts of a fresh launch */
    uint64_t *d_gslot;                 /* [batch] the frame of every trial slot */
    uint32_t *d_gknown, *d_gvalue;     /* [batch][Wn] the trial rows */
    int *d_gwin, *d_gnok, *d_gamb;     /* [batch / 2 + 1] per source of a trial launch */
    uint32_t *d_gout;                  /* [batch / 2 + 1][Wn] the winners' rows */
    uint64_t *d_goframe; uint32_t *d_goweak;   /* [fail_cap], [fail_cap][Wn]: the frames that ended open, in the order of the launches */
    mc_u64 *d_gctr, *h_gctr;           /* MC_GUESS_WORDS; pinned copy */
    std::vector<qldpc_mc_blind_round_stat> gstats;   /* of the last guess call */
};
#define MC_BLIND_WORDS ((size_t)(MC_BLIND_MAX_ROUNDS + 2) * (MC_BLIND_COUNTERS + 1))
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
    dm_free_all(&mc->mem);
    for (hipEvent_t e : mc->ev) if (e) (void)hipEventDestroy(e);
    delete mc;
}

/* *p = count elements on the device, in the loop's ledger; a buffer that is already there stays (the reserves are lazy and share d_erase) */
template <typename T> static int mc_lazy(qldpc_mc *mc, T **p, size_t count)
{
    if (*p) return QLDPC_OK;
    const int rc = dm_alloc(&mc->mem, p, count);
    if (rc) qldpc_set_error("mc_create: device allocation of %zu bytes failed", sizeof(T) * count);
    return rc;
}
/* the pinned counterpart */
template <typename T> static int mc_lazy_pinned(qldpc_mc *mc, T **p, size_t count) { return *p ? (int)QLDPC_OK : dm_alloc_pinned(&mc->mem, p, count); }

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
    if ((rc = mc_lazy(mc, &mc->d_cls, 32 * Wn)) || (rc = mc_lazy(mc, &mc->d_info_mask, Wn)) || (rc = mc_lazy(mc, &mc->d_chan_mask, Wn)) ||
        (rc = mc_lazy(mc, &mc->d_info, B * (size_t)mc->Wk)) || (rc = mc_lazy(mc, &mc->d_cw, B * Wn)) || (rc = mc_lazy(mc, &mc->d_rx, B * Wn)) ||
        (rc = mc_lazy(mc, &mc->d_out, B * Wn)) || (rc = mc_lazy(mc, &mc->d_mag, B)) || (rc = mc_lazy(mc, &mc->d_iters, B)) || (rc = mc_lazy(mc, &mc->d_ok, B)) ||
        (rc = mc_lazy(mc, &mc->d_ctr, (size_t)MC_COUNTERS + (size_t)mc->n_ite + 1 + (size_t)mc->fail_cap)) || (rc = mc_lazy_pinned(mc, &mc->h_ctr, MC_COUNTERS)))
        return rc;
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

extern "C" size_t qldpc_mc_device_bytes(const qldpc_mc *mc) { return mc ? mc->mem.dev_bytes : 0; }

static unsigned mc_blocks(size_t lanes) { return (unsigned)((lanes + MC_LANES - 1) / MC_LANES); }

/* the slots of frames first, first + 1, ... with one row {t, mag} for all of them */
static mc_slots mc_range(uint64_t first, uint32_t t = 0u, float mag = 0.0f) { return {nullptr, first, nullptr, nullptr, {t, mag}}; }
static mc_slots mc_bsc_range(uint64_t first, double qber) { return mc_range(first, mc_threshold(qber), qldpc_bsc_llr((float)qber)); }

/* source -> encoder -> channel for the n frames of sl on stream s; d_cw / d_rx / d_mag may be NULL from the right; ev != NULL: ev[1] after the
 * source, ev[2] after the encoder.  The channel: d_llr != NULL a table's, LLR rows into d_llr (d_rx may then be NULL alone; d_mag is not used; the
 * caller has checked n 8 Wn < 2^31): the one table d_tab where sl gives frame first + f, the slot's of d_tabs where sl has both slot tables; else
 * weight_bits != 0 the fixed weights of sl's rows with keys of weight_bits bits; else the BSC of sl's rows */
static int mc_generate(qldpc_mc *mc, const mc_slots &sl, int n, uint32_t *d_info, uint32_t *d_cw, uint32_t *d_rx, float *d_mag, hipStream_t s,
                       hipEvent_t *ev = nullptr, float *d_llr = nullptr, int weight_bits = 0)
{
    const unsigned ti = (unsigned)n * (unsigned)mc->Wk, tn = (unsigned)n * (unsigned)mc->Wn, Wn = (unsigned)mc->Wn;
    if (weight_bits < 0 || weight_bits > 32 || (d_llr && (!sl.frame != !sl.row || weight_bits))) {      /* a caller's mistake, not the user's */
        qldpc_set_error("mc_generate: weight_bits=%d outside 0 .. 32, or a table channel with one slot table of two or with a weight", weight_bits);
        return QLDPC_EINVAL;
    }
    if (mc->source == QLDPC_MC_SOURCE_ZERO) HIPCHK(hipMemsetAsync(d_info, 0, sizeof(uint32_t) * ti, s));
    else {
        hipLaunchKernelGGL(mc_source, dim3(mc_blocks(ti)), dim3(MC_LANES), 0, s, d_info, ti, (unsigned)mc->Wk, mc->K, mc->seed, sl);
        LAUNCHCHK();
    }
    if (ev) HIPCHK(hipEventRecord(ev[1], s));
    if (!d_cw) return QLDPC_OK;
    const int rc = qldpc_encode_packed_dev(mc->enc, d_info, d_cw, n, (void *)s);
    if (rc || (!d_rx && !d_llr)) return rc;
    if (ev) HIPCHK(hipEventRecord(ev[2], s));
    const uint32_t t_pinned = mc_threshold(mc->parity_ber);
    if (d_llr && sl.row)
        hipLaunchKernelGGL(mc_soft_channel_slots, dim3((unsigned)n, mc_blocks(8 * (size_t)Wn)), dim3(MC_LANES), 0, s, (const uint32_t *)d_cw, d_rx, d_llr,
                           (const uint32_t *)mc->d_cls, (const mc_soft_table *)mc->d_tabs, 8u * Wn, (unsigned)mc->N, mc->seed, sl, t_pinned);
    else if (d_llr)
        hipLaunchKernelGGL(mc_soft_channel, dim3(mc_blocks(8 * (size_t)tn)), dim3(MC_LANES), 0, s, (const uint32_t *)d_cw, d_rx, d_llr, (const uint32_t *)mc->d_cls,
                           (const mc_soft_table *)mc->d_tab, 8u * tn, 8u * Wn, (unsigned)mc->N, mc->seed, sl.first, t_pinned);
    else if (weight_bits)
        hipLaunchKernelGGL(mc_channel_weight, dim3((unsigned)n), dim3(MC_PAT_LANES), 0, s, (const uint32_t *)d_cw, d_rx, (const uint4 *)mc->d_cls, Wn, mc->seed, sl,
                           weight_bits, t_pinned, d_mag);
    else
        hipLaunchKernelGGL(mc_channel, dim3(mc_blocks(tn)), dim3(MC_LANES), 0, s, (const uint32_t *)d_cw, d_rx, (const uint4 *)mc->d_cls, tn, Wn, mc->seed, sl, t_pinned,
                           d_mag);
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
    return mc_generate(mc, mc_bsc_range(first_frame, qber), n_frames, d_info, d_cw, d_rx, nullptr, mc->dec->stream);
}

/* the frames of a batch into the decoder, by the channel in force (a table, else weight_bits as mc_generate takes it) or, `tables`, by the slots'
 * tables whatever is in force: generate (ev as mc_generate takes it), ev_channel, load */
static int mc_generate_load(qldpc_mc *mc, const mc_slots &sl, int n, hipStream_t s, hipEvent_t *ev, hipEvent_t ev_channel, int weight_bits = 0, bool tables = false)
{
    const bool soft = mc->soft || tables;
    const int rc = mc_generate(mc, sl, n, mc->d_info, mc->d_cw, mc->d_rx, mc->d_mag, s, ev, soft ? mc->d_llr : nullptr, weight_bits);
    if (rc) return rc;
    HIPCHK(hipEventRecord(ev_channel, s));
    return soft ? qldpc_load_llr_dev(mc->dec, mc->d_llr, n) : qldpc_load_bits_dev(mc->dec, mc->d_rx, mc->d_mag, mc->d_cls, n);
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
    if ((rc = mc_lazy(mc, &mc->d_tab, 1)) || (rc = mc_lazy(mc, &mc->d_llr, (size_t)mc->batch * (size_t)mc->N))) return rc;
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
    return mc_generate(mc, mc_range(first_frame), n_frames, d_info, d_cw, d_rx, nullptr, mc->dec->stream, nullptr, d_llr);
}

/* the erase rows of n frames into mc->d_erase, the layout qldpc_load_erasures_dev reads: the row of a slot by sl's row table, or d_rows[slot / F] */
static int mc_expand(qldpc_mc *mc, const uint32_t *d_rows, const mc_slots &sl, int n, int F, hipStream_t s)
{
    const unsigned total = (unsigned)n * (unsigned)mc->Wn;
    hipLaunchKernelGGL(mc_expand_rows, dim3(mc_blocks(((size_t)total + 3) / 4)), dim3(MC_LANES), 0, s, d_rows, mc->d_erase, total, (unsigned)mc->Wn, sl, (unsigned)F);
    LAUNCHCHK();
    return QLDPC_OK;
}

/* ... and into the decoder: after qldpc_load_bits_dev */
static int mc_erase(qldpc_mc *mc, const uint32_t *d_rows, const mc_slots &sl, int n, int F, hipStream_t s)
{
    const int rc = mc_expand(mc, d_rows, sl, n, F, s);
    return rc ? rc : qldpc_load_erasures_dev(mc->dec, mc->d_erase, n);
}

/* the decoder's words and verdicts of the n frames it holds, where the monitors read them */
static int mc_fetch(qldpc_mc *mc)
{
    const int rc = qldpc_fetch_packed_dev(mc->dec, mc->d_out);
    return rc ? rc : qldpc_fetch_status_dev(mc->dec, mc->d_iters, mc->d_ok);
}

static mc_decoded mc_decoded_of(const qldpc_mc *mc)
{
    return {mc->d_out, mc->d_cw, mc->d_rx, mc->d_info_mask, mc->d_chan_mask, mc->d_iters, mc->d_ok, (unsigned)mc->Wn, mc->n_ite};
}

/* the end of a batch or a round, behind its monitor: ev[n], the ONE read-back (`words` counters from d to the pinned h), and the time between
 * ev[k] and ev[k + 1] added to *stage[k] for the n stages */
static int mc_round_end(qldpc_mc *mc, mc_u64 *h, const mc_u64 *d, size_t words, double *const *stage, int n, hipStream_t s)
{
    HIPCHK(hipEventRecord(mc->ev[n], s));
    HIPCHK(hipMemcpyAsync(h, d, sizeof(mc_u64) * words, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    for (int k = 0; k < n; k++) {
        float ms = 0.0f;
        HIPCHK(hipEventElapsedTime(&ms, mc->ev[k], mc->ev[k + 1]));
        *stage[k] += (double)ms;
    }
    return QLDPC_OK;
}

/* frames .. channel_bits of a result or a stat row from a counter row of MC_POINT_COUNTERS */
template <typename S> static void mc_counters_out(S *st, const mc_u64 *c)
{
    st->frames = c[MC_FRAMES]; st->bit_errors = c[MC_BIT_ERRORS]; st->frame_errors = c[MC_FRAME_ERRORS]; st->undetected = c[MC_UNDETECTED];
    st->not_converged = c[MC_NOT_CONVERGED]; st->iter_sum = c[MC_ITER_SUM]; st->iter_max = c[MC_ITER_MAX];
    st->channel_flips = c[MC_FLIPS]; st->channel_bits = c[MC_CHANNEL_BITS];
}

/* the stat rows of the last call, for the *_stats getters: copies min(cap, their number), returns their number */
template <typename S> static int mc_stats_out(const std::vector<S> &all, S *rows, int cap)
{
    if (cap < 0 || (cap && !rows)) return QLDPC_EINVAL;
    const size_t n = std::min((size_t)cap, all.size());
    if (n) memcpy(rows, all.data(), sizeof(S) * n);
    return (int)all.size();
}

/* a histogram row [n_ite + 1] on the device, for the *_hist getters: copies min(cap, n_ite + 1) bins, returns n_ite + 1 */
static int mc_hist_out(qldpc_mc *mc, const mc_u64 *d_hist, uint64_t *hist, int cap)
{
    const int bins = std::min(cap, mc->n_ite + 1);
    HIPCHK(hipSetDevice(mc->device));
    HIPCHK(hipStreamSynchronize(mc->dec->stream));
    if (bins) HIPCHK(hipMemcpy(hist, d_hist, sizeof(mc_u64) * (size_t)bins, hipMemcpyDeviceToHost));
    return mc->n_ite + 1;
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
    double *const stage[6] = {&result->source_ms, &result->encode_ms, &result->channel_ms, &result->load_ms, &result->decode_ms, &result->monitor_ms};
    const auto t_start = std::chrono::steady_clock::now();
    for (uint64_t done = 0; done < max_frames;) {
        const int nb = (int)std::min<uint64_t>((uint64_t)mc->batch, max_frames - done);
        const uint64_t first = first_frame + done;
        HIPCHK(hipEventRecord(mc->ev[0], s));
        int rc = mc_generate_load(mc, mc_bsc_range(first, qber), nb, s, mc->ev, mc->ev[3]);
        if (rc) return rc;
        if (mc->n_fixed && (rc = mc_erase(mc, mc->d_fixed, mc_range(0), nb, nb, s))) return rc;      /* the fixed puncture set: one row for all nb frames */
        HIPCHK(hipEventRecord(mc->ev[4], s));
        if ((rc = qldpc_run(mc->dec))) return rc;
        HIPCHK(hipEventRecord(mc->ev[5], s));
        if ((rc = mc_fetch(mc))) return rc;
        const unsigned waves = (unsigned)std::min(nb, MC_MAX_WAVES);
        hipLaunchKernelGGL(mc_monitor, dim3((waves + 3u) / 4u), dim3(MC_LANES), 0, s, mc_decoded_of(mc), (unsigned)nb, first, mc->channel_vns, mc->d_ctr, hist, fails,
                           (unsigned)mc->fail_cap);
        LAUNCHCHK();
        if ((rc = mc_round_end(mc, mc->h_ctr, mc->d_ctr, MC_COUNTERS, stage, 6, s))) return rc;
        result->batches++;
        done += (uint64_t)nb;
        if (max_frame_errors && mc->h_ctr[MC_FRAME_ERRORS] >= max_frame_errors) break;
    }
    result->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    mc_counters_out(result, mc->h_ctr);
    result->next_frame = first_frame + result->frames;
    return QLDPC_OK;
}

extern "C" int qldpc_mc_iter_hist(qldpc_mc *mc, uint64_t *hist, int cap)
{
    if (!mc || !hist || cap < 0) return QLDPC_EINVAL;
    return mc_hist_out(mc, mc->d_ctr + MC_COUNTERS, hist, cap);
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
        if ((rc = mc_lazy(mc, &mc->d_cand, (size_t)mc->N)) || (rc = mc_lazy(mc, &mc->d_pat, B * Wn)) || (rc = mc_lazy(mc, &mc->d_erase, B * Wn)) ||
            (rc = mc_lazy(mc, &mc->d_fixed, Wn)) || (rc = mc_lazy(mc, &mc->d_rows, B * MC_PATTERN_COUNTERS)) ||
            (rc = mc_lazy_pinned(mc, &mc->h_rows, B * MC_PATTERN_COUNTERS)) || (rc = qldpc_decoder_reserve(mc->dec)))      /* the decoder's erasure ballots */
            return rc;
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
    const unsigned F = (unsigned)cfg->frames_per_pattern;
    const uint64_t per_round = (uint64_t)mc->batch / F;
    mc->stats.clear();
    double *const stage[7] = {&res->pattern_ms, &res->expand_ms, &res->generate_ms, &res->load_ms, &res->erase_ms, &res->decode_ms, &res->monitor_ms};
    const auto t_start = std::chrono::steady_clock::now();
    for (uint64_t done = 0; done < max_patterns;) {
        const int np = (int)std::min<uint64_t>(per_round, max_patterns - done), nb = np * (int)F;
        const uint64_t p0 = first_pattern + done, frame0 = cfg->first_frame + p0 * F;      /* frame k of pattern p = first_frame + p F + k */
        HIPCHK(hipEventRecord(mc->ev[0], s));
        mc_launch_patterns(mc, p0, np, cfg->n_punct, cfg->key_bits, mc->d_pat, s);
        LAUNCHCHK();
        HIPCHK(hipEventRecord(mc->ev[1], s));
        if ((rc = mc_expand(mc, mc->d_pat, mc_range(0), nb, (int)F, s))) return rc;
        HIPCHK(hipEventRecord(mc->ev[2], s));
        if ((rc = mc_generate_load(mc, mc_bsc_range(frame0, qber), nb, s, nullptr, mc->ev[3]))) return rc;
        HIPCHK(hipEventRecord(mc->ev[4], s));
        if ((rc = qldpc_load_erasures_dev(mc->dec, mc->d_erase, nb))) return rc;
        HIPCHK(hipEventRecord(mc->ev[5], s));
        if ((rc = qldpc_run(mc->dec))) return rc;
        HIPCHK(hipEventRecord(mc->ev[6], s));
        if ((rc = mc_fetch(mc))) return rc;
        HIPCHK(hipMemsetAsync(mc->d_rows, 0, sizeof(mc_u64) * (size_t)np * MC_PATTERN_COUNTERS, s));
        const unsigned wpp = std::min(F, std::max(1u, (unsigned)MC_MAX_WAVES / (unsigned)np)), waves = (unsigned)np * wpp;
        hipLaunchKernelGGL(mc_monitor_patterns, dim3((waves + 3u) / 4u), dim3(MC_LANES), 0, s, mc_decoded_of(mc), (unsigned)np, F, wpp, mc->d_rows);
        LAUNCHCHK();
        if ((rc = mc_round_end(mc, mc->h_rows, mc->d_rows, (size_t)np * MC_PATTERN_COUNTERS, stage, 7, s))) return rc;
        for (int i = 0; i < np; i++) {
            const mc_u64 *c = mc->h_rows + (size_t)i * MC_PATTERN_COUNTERS;
            qldpc_mc_pattern_stat st = {p0 + (uint64_t)i, c[MC_FRAMES], c[MC_FRAME_ERRORS], c[MC_BIT_ERRORS], c[MC_UNDETECTED], c[MC_NOT_CONVERGED], c[MC_ITER_SUM]};
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
    if (!mc) return QLDPC_EINVAL;
    return mc_stats_out(mc->stats, rows, cap);
}

/* ------------------------------------------------------------------ QBER sweep and error strata: rows side by side in one batch ---- */

/* everything the rounds need on the device, once */
static int mc_sweep_reserve(qldpc_mc *mc)
{
    HIPCHK(hipSetDevice(mc->device));
    if (mc->sweep_ready) return QLDPC_OK;
    const size_t Wn = (size_t)mc->Wn, B = (size_t)mc->batch, P = QLDPC_MC_SWEEP_MAX_POINTS, bins = (size_t)mc->n_ite + 1;
    int rc = QLDPC_OK;
    if ((rc = mc_lazy(mc, &mc->d_slots, 3 * B)) || (rc = mc_lazy(mc, &mc->d_points, P)) || (rc = mc_lazy(mc, &mc->d_prows, P * Wn)) ||
        (rc = mc_lazy(mc, &mc->d_erase, B * Wn)) || (rc = mc_lazy(mc, &mc->d_wctr, P * MC_POINT_COUNTERS)) || (rc = mc_lazy(mc, &mc->d_whist, P * bins)) ||
        (rc = mc_lazy_pinned(mc, &mc->h_slots, 3 * B)) || (rc = mc_lazy_pinned(mc, &mc->h_wctr, P * MC_POINT_COUNTERS)) ||
        (rc = qldpc_decoder_reserve(mc->dec)))      /* the decoder's erasure ballots */
        return rc;
    mc->sweep_ready = true;
    return QLDPC_OK;
}

/* what qldpc_mc_sweep and qldpc_mc_strata check of their cfg in common, in the order both check it.  refused_soft = the caller's whole error text
 * for a channel table in force; design_qber: the strata have one, the sweep passes NULL */
static int mc_rounds_args(const qldpc_mc *mc, const char *who, const int reserved[2], const char *refused_soft, const char *n_name, int n,
                          const double *design_qber, int chunk, uint64_t max_frames)
{
    if (reserved[0] || reserved[1]) { qldpc_set_error("%s: reserved fields %d, %d must be zero", who, reserved[0], reserved[1]); return QLDPC_EINVAL; }
    if (mc->soft) { qldpc_set_error("%s", refused_soft); return QLDPC_ESTATE; }
    if (n < 1 || n > QLDPC_MC_SWEEP_MAX_POINTS) { qldpc_set_error("%s: %s=%d outside 1 .. %d", who, n_name, n, QLDPC_MC_SWEEP_MAX_POINTS); return QLDPC_ESIZE; }
    if (design_qber && !(*design_qber > 0.0 && *design_qber < 0.5)) { qldpc_set_error("%s: design_qber=%g outside (0, 0.5)", who, *design_qber); return QLDPC_ESIZE; }
    if (chunk < 0 || chunk > mc->batch) { qldpc_set_error("%s: chunk=%d outside [0, batch=%d]", who, chunk, mc->batch); return QLDPC_ESIZE; }
    if (max_frames == 0) { qldpc_set_error("%s: max_frames=0", who); return QLDPC_ESIZE; }
    return QLDPC_OK;
}

/* every argument check of qldpc_mc_sweep: nothing is touched before all of them pass */
static int mc_sweep_args(const qldpc_mc *mc, const qldpc_mc_sweep_cfg *cfg)
{
    const int rc = mc_rounds_args(mc, "mc_sweep", cfg->reserved,
                                  "mc_sweep: a channel table is in force (qldpc_mc_set_channel); the sweep's points are points of the BSC", "n_points",
                                  cfg->n_points, nullptr, cfg->chunk, cfg->max_frames);
    if (rc) return rc;
    if (!cfg->points || cfg->n_order < 0 || (cfg->n_order > 0 && !cfg->punct_order)) { qldpc_set_error("mc_sweep: a missing array (points, or punct_order with n_order=%d)", cfg->n_order); return QLDPC_EINVAL; }
    std::vector<uint8_t> seen((size_t)mc->N, 0);
    const int bad = mc_punct_order_check(cfg->punct_order, cfg->n_order, mc->N, seen.data());
    if (bad >= 0) { qldpc_set_error("mc_sweep: punct_order[%d] = %d is repeated or outside [0, %d)", bad, cfg->punct_order[bad], mc->N); return QLDPC_EINVAL; }
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
    const mc_row *rows;                /* [P] {threshold, |LLR|} of the sweep's points, or {weight, |LLR|} of the strata; NULL with tabs */
    const uint32_t *erows;             /* [P][Wn] the erase rows, NULL = nothing is erased */
    int weight_key_bits;               /* 0: the BSC of the rows' thresholds (mc_channel); 1 .. 32: the rows' fixed weights (mc_channel_weight) */
    int owner;                         /* MC_ROWS_*: whose rows the device holds from here on */
    const mc_soft_table *tabs;         /* [P] the tables of the points of a table sweep (mc_soft_channel_slots; d_tabs holds P, d_llr is there), else NULL */
};

static int mc_rounds(qldpc_mc *mc, const mc_rounds_job &job, uint64_t *last_round /* [P] */, qldpc_mc_sweep_result *res)
{
    const hipStream_t s = mc->dec->stream;
    const int P = job.P, C = job.C, S = mc->batch / C;
    const size_t B = (size_t)mc->batch, Wn = (size_t)mc->Wn, bins = (size_t)mc->n_ite + 1;
    const uint64_t max_frames = job.max_frames, max_fe = job.max_fe;
    /* the tables of a round inside the one buffer */
    uint64_t *const h_frame = (uint64_t *)mc->h_slots;
    uint32_t *const h_point = (uint32_t *)(mc->h_slots + B), *const h_cpoint = h_point + B, *const h_cstart = h_cpoint + B, *const h_clen = h_cstart + B;
    const uint32_t *const d_point = (const uint32_t *)(mc->d_slots + B), *const d_cpoint = d_point + B, *const d_cstart = d_cpoint + B, *const d_clen = d_cstart + B;
    const mc_slots sl = {(const uint64_t *)mc->d_slots, 0, d_point, mc->d_points, {0u, 0.0f}};

    HIPCHK(hipStreamSynchronize(s));      /* a queued kernel may still read the rows of an earlier call */
    if (job.rows) HIPCHK(hipMemcpy(mc->d_points, job.rows, sizeof(mc_row) * (size_t)P, hipMemcpyHostToDevice));
    if (job.tabs) HIPCHK(hipMemcpy(mc->d_tabs, job.tabs, sizeof(mc_soft_table) * (size_t)P, hipMemcpyHostToDevice));
    if (job.erows) HIPCHK(hipMemcpy(mc->d_prows, job.erows, sizeof(uint32_t) * (size_t)P * Wn, hipMemcpyHostToDevice));
    mc->rows_owner = job.owner;
    HIPCHK(hipMemsetAsync(mc->d_wctr, 0, sizeof(mc_u64) * (size_t)P * MC_POINT_COUNTERS, s));
    HIPCHK(hipMemsetAsync(mc->d_whist, 0, sizeof(mc_u64) * (size_t)P * bins, s));

    std::vector<uint64_t> done((size_t)P, 0), fe((size_t)P, 0);
    std::vector<int> give((size_t)P);
    int rc = QLDPC_OK;
    double *const stage[7] = {&res->source_ms, &res->encode_ms, &res->channel_ms, &res->load_ms, &res->erase_ms, &res->decode_ms, &res->monitor_ms};
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
        HIPCHK(hipEventRecord(mc->ev[0], s));
        HIPCHK(hipMemcpyAsync(mc->d_slots, mc->h_slots, sizeof(mc_u64) * 3 * B, hipMemcpyHostToDevice, s));      /* pinned: the host rewrites it after the sync below */
        if ((rc = mc_generate_load(mc, sl, (int)nb, s, mc->ev, mc->ev[3], job.weight_key_bits, job.tabs != nullptr))) return rc;
        HIPCHK(hipEventRecord(mc->ev[4], s));
        if (job.erows && (rc = mc_erase(mc, mc->d_prows, sl, (int)nb, 1, s))) return rc;
        HIPCHK(hipEventRecord(mc->ev[5], s));
        if ((rc = qldpc_run(mc->dec))) return rc;
        HIPCHK(hipEventRecord(mc->ev[6], s));
        if ((rc = mc_fetch(mc))) return rc;
        const unsigned wpc = std::min((unsigned)C, std::max(1u, (unsigned)MC_MAX_WAVES / nc)), waves = nc * wpc;
        hipLaunchKernelGGL(mc_monitor_points, dim3((waves + 3u) / 4u), dim3(MC_LANES), 0, s, mc_decoded_of(mc), nc, wpc, d_cpoint, d_cstart, d_clen, mc->channel_vns,
                           mc->d_wctr, mc->d_whist);
        LAUNCHCHK();
        if ((rc = mc_round_end(mc, mc->h_wctr, mc->d_wctr, (size_t)P * MC_POINT_COUNTERS, stage, 7, s))) return rc;
        for (int q = 0; q < P; q++) { done[(size_t)q] = mc->h_wctr[(size_t)q * MC_POINT_COUNTERS + MC_FRAMES]; fe[(size_t)q] = mc->h_wctr[(size_t)q * MC_POINT_COUNTERS + MC_FRAME_ERRORS]; }
        res->rounds++; res->batches++;
    }
    for (int q = 0; q < P; q++) res->frames += mc->h_wctr[(size_t)q * MC_POINT_COUNTERS + MC_FRAMES];
    res->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    return QLDPC_OK;
}

/* row q of the last rounds into the stat row of a point or a stratum */
template <typename S> static void mc_row_out(const qldpc_mc *mc, int q, uint64_t max_frames, uint64_t last_round, S *st)
{
    mc_counters_out(st, mc->h_wctr + (size_t)q * MC_POINT_COUNTERS);
    st->closed_by = st->frames >= max_frames ? QLDPC_MC_CLOSED_MAX_FRAMES : QLDPC_MC_CLOSED_MAX_FE;
    st->last_round = last_round;
}

/* histogram row `row` of the last rounds, for qldpc_mc_sweep_hist and qldpc_mc_strata_hist */
static int mc_row_hist(qldpc_mc *mc, int row, uint64_t *hist, int cap)
{
    return mc_hist_out(mc, mc->d_whist + (size_t)row * (size_t)(mc->n_ite + 1), hist, cap);
}

/* erows[P][Wn] = the erase rows of the points of a sweep, BSC points or table points: the fixed set of qldpc_mc_set_puncture OR the first n_punct
 * VNs of the order.  Returns whether any row erases anything */
template <typename Pt> static bool mc_point_erows(const qldpc_mc *mc, const Pt *points, int P, const int *punct_order, std::vector<uint32_t> *erows)
{
    const size_t Wn = (size_t)mc->Wn;
    bool any = mc->n_fixed != 0;
    erows->assign((size_t)P * Wn, 0u);
    for (int q = 0; q < P; q++) {
        uint32_t *row = erows->data() + (size_t)q * Wn;
        if (mc->n_fixed) memcpy(row, mc->h_fixed.data(), sizeof(uint32_t) * Wn);
        for (int i = 0; i < points[q].n_punct; i++) { const int v = punct_order[i]; row[v >> 5] |= 0x80000000u >> (v & 31); }
        any = any || points[q].n_punct > 0;
    }
    return any;
}

extern "C" int qldpc_mc_sweep(qldpc_mc *mc, const qldpc_mc_sweep_cfg *cfg, qldpc_mc_sweep_result *res)
{
    if (!mc || !cfg || !res) return QLDPC_EINVAL;
    memset(res, 0, sizeof(*res));
    int rc = mc_sweep_args(mc, cfg);
    if (rc || (rc = mc_sweep_reserve(mc))) return rc;
    const int P = cfg->n_points;
    /* per sweep: the point rows and the erase rows, built here once */
    std::vector<mc_row> prow((size_t)P);
    std::vector<uint32_t> erows;
    for (int q = 0; q < P; q++) prow[(size_t)q] = {mc_threshold(cfg->points[q].qber), qldpc_bsc_llr((float)cfg->points[q].qber)};
    const bool any_erase = mc_point_erows(mc, cfg->points, P, cfg->punct_order, &erows);
    mc->wstats.assign((size_t)P, qldpc_mc_point_stat());
    for (int q = 0; q < P; q++) { mc->wstats[(size_t)q].qber = cfg->points[q].qber; mc->wstats[(size_t)q].n_punct = cfg->points[q].n_punct; }
    const mc_rounds_job job = {P, cfg->chunk ? cfg->chunk : std::min(64, mc->batch), cfg->first_frame, cfg->max_frames, cfg->max_frame_errors, prow.data(),
                               any_erase ? erows.data() : nullptr, 0, MC_ROWS_SWEEP, nullptr};
    std::vector<uint64_t> last((size_t)P, 0);
    if ((rc = mc_rounds(mc, job, last.data(), res))) return rc;
    for (int q = 0; q < P; q++) mc_row_out(mc, q, cfg->max_frames, last[(size_t)q], &mc->wstats[(size_t)q]);
    return QLDPC_OK;
}

/* the sweep over points of table channels: the rounds of qldpc_mc_sweep with the slot's table in place of the slot's threshold */
extern "C" int qldpc_mc_sweep_tables(qldpc_mc *mc, const qldpc_mc_sweep_tables_cfg *cfg, qldpc_mc_sweep_result *res)
{
    if (!mc || !cfg || !res) return QLDPC_EINVAL;
    memset(res, 0, sizeof(*res));
    int rc = qldpc_mc_sweep_tables_check_host(mc->N, mc->batch, cfg);      /* every argument check, mc_soft_lanes_check's among them */
    if (rc || (rc = mc_sweep_reserve(mc))) return rc;
    const int P = cfg->n_points;
    std::vector<mc_soft_table> tabs((size_t)P);
    for (int q = 0; q < P; q++) {
        const qldpc_mc_channel &t = cfg->points[q].table;
        if (mc_soft_table_build(t.levels, t.cum[0], t.cum[1], t.value, &tabs[(size_t)q])) return QLDPC_EINVAL;      /* not reached: the check has built it */
    }
    HIPCHK(hipStreamSynchronize(mc->dec->stream));      /* a queued channel kernel may still read the tables that dm_grow replaces */
    if ((rc = mc_lazy(mc, &mc->d_llr, (size_t)mc->batch * (size_t)mc->N)) || (rc = dm_grow(&mc->mem, &mc->d_tabs, &mc->tabs_cap, (size_t)P))) return rc;
    std::vector<uint32_t> erows;
    const bool any_erase = mc_point_erows(mc, cfg->points, P, cfg->punct_order, &erows);
    mc->wstats.assign((size_t)P, qldpc_mc_point_stat());
    for (int q = 0; q < P; q++) { mc->wstats[(size_t)q].qber = cfg->points[q].label; mc->wstats[(size_t)q].n_punct = cfg->points[q].n_punct; }
    const mc_rounds_job job = {P, cfg->chunk ? cfg->chunk : std::min(64, mc->batch), cfg->first_frame, cfg->max_frames, cfg->max_frame_errors, nullptr,
                               any_erase ? erows.data() : nullptr, 0, MC_ROWS_SWEEP, tabs.data()};
    std::vector<uint64_t> last((size_t)P, 0);
    if ((rc = mc_rounds(mc, job, last.data(), res))) return rc;
    for (int q = 0; q < P; q++) mc_row_out(mc, q, cfg->max_frames, last[(size_t)q], &mc->wstats[(size_t)q]);
    return QLDPC_OK;
}

extern "C" int qldpc_mc_sweep_stats(qldpc_mc *mc, qldpc_mc_point_stat *rows, int cap)
{
    if (!mc) return QLDPC_EINVAL;
    return mc_stats_out(mc->wstats, rows, cap);
}

extern "C" int qldpc_mc_sweep_hist(qldpc_mc *mc, int point, uint64_t *hist, int cap)
{
    if (!mc || cap < 0 || (cap && !hist)) return QLDPC_EINVAL;
    if (point < 0 || (size_t)point >= mc->wstats.size()) { qldpc_set_error("mc_sweep_hist: point=%d, the last sweep had %d", point, (int)mc->wstats.size()); return QLDPC_ESIZE; }
    if (mc->rows_owner != MC_ROWS_SWEEP) { qldpc_set_error("mc_sweep_hist: the device rows hold a later qldpc_mc_strata run"); return QLDPC_ESTATE; }
    return mc_row_hist(mc, point, hist, cap);
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
    return mc_generate(mc, mc_range(first_frame, (uint32_t)weight), n_frames, d_info, d_cw, d_rx, nullptr, mc->dec->stream, nullptr, nullptr, mc_key_bits(key_bits));
}

/* every argument check of qldpc_mc_strata: nothing is touched before all of them pass */
static int mc_strata_args(const qldpc_mc *mc, const qldpc_mc_strata_cfg *cfg)
{
    int rc = mc_rounds_args(mc, "mc_strata", cfg->reserved,
                            "mc_strata: a channel table is in force (qldpc_mc_set_channel); error weights are weights of the BSC", "n_strata", cfg->n_strata,
                            &cfg->design_qber, cfg->chunk, cfg->max_frames);
    if (rc) return rc;
    if (!cfg->weights) { qldpc_set_error("mc_strata: a missing array (weights)"); return QLDPC_EINVAL; }
    for (int q = 0; q < cfg->n_strata; q++)
        if ((rc = mc_weight_args(mc, "mc_strata", cfg->weights[q], cfg->key_bits))) return rc;
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
    /* per call: the stratum rows, and the fixed set as every stratum's erase row */
    std::vector<mc_row> prow((size_t)P);
    std::vector<uint32_t> erows;
    const float mag = qldpc_bsc_llr((float)cfg->design_qber);
    for (int q = 0; q < P; q++) prow[(size_t)q] = {(uint32_t)cfg->weights[q], mag};
    if (mc->n_fixed) for (int q = 0; q < P; q++) erows.insert(erows.end(), mc->h_fixed.begin(), mc->h_fixed.begin() + (ptrdiff_t)Wn);
    mc->tstats.assign((size_t)P, qldpc_mc_stratum_stat());
    for (int q = 0; q < P; q++) mc->tstats[(size_t)q].weight = cfg->weights[q];
    const mc_rounds_job job = {P, cfg->chunk ? cfg->chunk : std::min(64, mc->batch), cfg->first_frame, cfg->max_frames, cfg->max_frame_errors, prow.data(),
                               mc->n_fixed ? erows.data() : nullptr, mc_key_bits(cfg->key_bits), MC_ROWS_STRATA, nullptr};
    std::vector<uint64_t> last((size_t)P, 0);
    if ((rc = mc_rounds(mc, job, last.data(), res))) return rc;
    for (int q = 0; q < P; q++) mc_row_out(mc, q, cfg->max_frames, last[(size_t)q], &mc->tstats[(size_t)q]);
    return QLDPC_OK;
}

extern "C" int qldpc_mc_strata_stats(qldpc_mc *mc, qldpc_mc_stratum_stat *rows, int cap)
{
    if (!mc) return QLDPC_EINVAL;
    return mc_stats_out(mc->tstats, rows, cap);
}

extern "C" int qldpc_mc_strata_hist(qldpc_mc *mc, int stratum, uint64_t *hist, int cap)
{
    if (!mc || cap < 0 || (cap && !hist)) return QLDPC_EINVAL;
    if (stratum < 0 || (size_t)stratum >= mc->tstats.size()) { qldpc_set_error("mc_strata_hist: stratum=%d, the last run had %d", stratum, (int)mc->tstats.size()); return QLDPC_ESIZE; }
    if (mc->rows_owner != MC_ROWS_STRATA) { qldpc_set_error("mc_strata_hist: the device rows hold a later qldpc_mc_sweep"); return QLDPC_ESTATE; }
    return mc_row_hist(mc, stratum, hist, cap);
}

/* ------------------------------------------------------------------ blind reconciliation rounds ---- */

/* everything the rounds need on the device: the launch buffers and the open list once, the pools for `levels` levels unless they hold as many already */
static int mc_blind_reserve(qldpc_mc *mc, int levels)
{
    HIPCHK(hipSetDevice(mc->device));
    const size_t Wn = (size_t)mc->Wn, B = (size_t)mc->batch, cap = MC_BLIND_POOL_CAP(mc->batch);
    int rc = QLDPC_OK;
    if (!mc->blind_ready) {
        if ((rc = mc_lazy(mc, &mc->d_bcand, B * Wn)) || (rc = mc_lazy(mc, &mc->d_bweak, B * Wn)) || (rc = mc_lazy(mc, &mc->d_btake, B)) ||
            (rc = mc_lazy(mc, &mc->d_bopen, B)) || (rc = mc_lazy(mc, &mc->d_oframe, (size_t)mc->fail_cap)) ||
            (rc = mc_lazy(mc, &mc->d_oknown, (size_t)mc->fail_cap * Wn)) || (rc = mc_lazy(mc, &mc->d_bctr, MC_BLIND_WORDS)) ||
            (rc = mc_lazy_pinned(mc, &mc->h_bctr, MC_BLIND_WORDS)))
            return rc;
        mc->blind_ready = true;
    }
    if (levels <= mc->blind_levels) return QLDPC_OK;
    HIPCHK(hipStreamSynchronize(mc->dec->stream));      /* nothing queued reads the pools that go */
    dm_release(&mc->mem, &mc->d_pframe);
    dm_release(&mc->mem, &mc->d_pknown);
    mc->blind_levels = 0;
    if ((rc = mc_lazy(mc, &mc->d_pframe, (size_t)levels * cap)) || (rc = mc_lazy(mc, &mc->d_pknown, (size_t)levels * cap * Wn))) return rc;
    mc->blind_levels = levels;
    return QLDPC_OK;
}

/* every argument check of qldpc_mc_blind: nothing is touched before all of them pass */
static int mc_blind_args(const qldpc_mc *mc, const qldpc_mc_blind_cfg *cfg)
{
    if (cfg->reserved[0] || cfg->reserved[1]) { qldpc_set_error("mc_blind: reserved fields %d, %d must be zero", cfg->reserved[0], cfg->reserved[1]); return QLDPC_EINVAL; }
    if (!(cfg->qber > 0.0 && cfg->qber < 0.5)) { qldpc_set_error("mc_blind: qber=%g outside (0, 0.5)", cfg->qber); return QLDPC_ESIZE; }
    if (cfg->ask_bits < 1) { qldpc_set_error("mc_blind: ask_bits=%d (at least 1)", cfg->ask_bits); return QLDPC_ESIZE; }
    if (cfg->max_rounds < 0 || cfg->max_rounds > QLDPC_MC_BLIND_MAX_ROUNDS) { qldpc_set_error("mc_blind: max_rounds=%d outside 0 .. %d", cfg->max_rounds, QLDPC_MC_BLIND_MAX_ROUNDS); return QLDPC_ESIZE; }
    if (mc->soft) { qldpc_set_error("mc_blind: a channel table is in force; the rounds run on the BSC: clear it with qldpc_mc_set_channel(mc, NULL)"); return QLDPC_EUNSUPPORTED; }
    if (mc->dec->engine == QLDPC_ENGINE_EDGES) { qldpc_set_error("mc_blind: the select of the weakest VNs is not built for the edge-parallel engine: create the decoder with engine = FRAMES"); return QLDPC_EUNSUPPORTED; }
    if (mc->dec->compact_mode != 2) {      /* the engine's own rule, resolved when the decoder was created */
        qldpc_set_error("mc_blind: the decoder may compact its active frames (compact = %d), after which the posteriors of the frames that converged earlier are gone: "
                        "create it with compact = 2", mc->dec->cfg.compact);
        return QLDPC_EUNSUPPORTED;
    }
    if (mc->dec->gu.patience > 0 && !mc->dec->freeze) {      /* a frame given up asks with the posteriors it stopped at: exact only with frozen messages */
        qldpc_set_error("mc_blind: the decoder gives frames up (giveup_patience = %d) and lets their messages run on, so the posteriors a failed frame asks with "
                        "are not the ones it stopped at: create it with freeze_messages = 1", mc->dec->gu.patience);
        return QLDPC_EUNSUPPORTED;
    }
    return QLDPC_OK;
}

extern "C" int qldpc_mc_blind(qldpc_mc *mc, const qldpc_mc_blind_cfg *cfg, qldpc_mc_blind_result *res)
{
    if (!mc || !cfg || !res) return QLDPC_EINVAL;
    memset(res, 0, sizeof(*res));
    res->next_frame = cfg->first_frame;
    int rc = mc_blind_args(mc, cfg);
    if (rc || (rc = mc_blind_reserve(mc, cfg->max_rounds))) return rc;
    const hipStream_t s = mc->dec->stream;
    const int R = cfg->max_rounds;
    const size_t Wn = (size_t)mc->Wn, cap = MC_BLIND_POOL_CAP(mc->batch), words = (size_t)(R + 2) * (MC_BLIND_COUNTERS + 1);
    mc_u64 *const d_count = mc->d_bctr + (size_t)(R + 2) * MC_BLIND_COUNTERS;
    const mc_u64 *const h_count = mc->h_bctr + (size_t)(R + 2) * MC_BLIND_COUNTERS;
    const mc_row row = {mc_threshold(cfg->qber), qldpc_bsc_llr((float)cfg->qber)};
    HIPCHK(hipMemsetAsync(mc->d_bctr, 0, sizeof(mc_u64) * words, s));
    memset(mc->h_bctr, 0, sizeof(mc_u64) * words);
    mc->bstats.assign((size_t)R + 2, qldpc_mc_blind_round_stat());

    uint64_t pool[QLDPC_MC_BLIND_MAX_ROUNDS + 1] = {0}, done = 0, input_left = cfg->max_frames;
    int level = 0, n = 0;
    double *const stage[7] = {&res->source_ms, &res->encode_ms, &res->channel_ms, &res->load_ms, &res->decode_ms, &res->select_ms, &res->advance_ms};
    const auto t_start = std::chrono::steady_clock::now();
    while (mc_blind_next(R, mc->batch, pool, input_left, &level, &n)) {
        /* level r >= 1: the last n entries of pool r, a contiguous frame table and a contiguous [n][Wn] array of known rows */
        const size_t top = level ? (size_t)(level - 1) * cap + (size_t)pool[level] - (size_t)n : 0;
        const uint32_t *known = level ? mc->d_pknown + top * Wn : nullptr;
        const mc_slots sl = {level ? mc->d_pframe + top : nullptr, cfg->first_frame + done, nullptr, nullptr, row};
        HIPCHK(hipEventRecord(mc->ev[0], s));
        if ((rc = mc_generate_load(mc, sl, n, s, mc->ev, mc->ev[3]))) return rc;
        if (mc->n_fixed && (rc = mc_erase(mc, mc->d_fixed, mc_range(0), n, n, s))) return rc;      /* the fixed puncture set: one row for all n frames */
        if (known && (rc = qldpc_load_known_dev(mc->dec, known, mc->d_cw, n))) return rc;          /* Alice's answer: her codeword is on the device */
        HIPCHK(hipEventRecord(mc->ev[4], s));
        if ((rc = qldpc_run(mc->dec))) return rc;
        HIPCHK(hipEventRecord(mc->ev[5], s));
        if ((rc = mc_fetch(mc))) return rc;
        const unsigned total = (unsigned)n * (unsigned)mc->Wn;
        if (level < R) {
            hipLaunchKernelGGL(mc_blind_cand, dim3(mc_blocks(total)), dim3(MC_LANES), 0, s, (const uint32_t *)mc->d_chan_mask, known, (const int *)mc->d_ok, mc->d_bcand,
                               mc->d_btake, total, (unsigned)mc->Wn);
            LAUNCHCHK();
            if ((rc = qldpc_fetch_weakest_dev(mc->dec, mc->d_bcand, mc->d_btake, cfg->ask_bits, mc->d_bweak))) return rc;
        }
        HIPCHK(hipEventRecord(mc->ev[6], s));
        const unsigned waves = (unsigned)std::min(n, MC_MAX_WAVES);
        hipLaunchKernelGGL(mc_blind_advance, dim3((waves + 3u) / 4u), dim3(MC_LANES), 0, s, mc_decoded_of(mc), (unsigned)n, known, mc->channel_vns,
                           mc->d_bctr + (size_t)level * MC_BLIND_COUNTERS, level == R ? mc->d_bctr + (size_t)(R + 1) * MC_BLIND_COUNTERS : nullptr, mc->d_bopen,
                           level ? d_count + level : nullptr, (mc_u64)(pool[level] - (uint64_t)n));
        LAUNCHCHK();
        /* the open frames go on to pool level + 1 with what they asked for, or after the last round onto the list of the frames that ended open */
        const unsigned groups = ((unsigned)n + MC_APPEND_SLOTS - 1u) / MC_APPEND_SLOTS;
        if (level < R)
            hipLaunchKernelGGL(mc_blind_advance_append, dim3(groups), dim3(MC_LANES), 0, s, (const int *)mc->d_bopen, (unsigned)n, sl, known, (const uint32_t *)mc->d_bweak,
                               (unsigned)mc->Wn, mc->d_pframe + (size_t)level * cap, mc->d_pknown + (size_t)level * cap * Wn, (mc_u64)pool[level + 1], (mc_u64)cap,
                               d_count + level + 1);
        else
            hipLaunchKernelGGL(mc_blind_advance_append, dim3(groups), dim3(MC_LANES), 0, s, (const int *)mc->d_bopen, (unsigned)n, sl, known, (const uint32_t *)nullptr,
                               (unsigned)mc->Wn, mc->d_oframe, mc->d_oknown, h_count[R + 1], (mc_u64)mc->fail_cap, d_count + R + 1);
        LAUNCHCHK();
        if ((rc = mc_round_end(mc, mc->h_bctr, mc->d_bctr, words, stage, 7, s))) return rc;
        res->launches++; res->decodes += (uint64_t)n;
        if (level == 0) { done += (uint64_t)n; input_left -= (uint64_t)n; }
        uint64_t fe = 0;
        for (int r = 0; r <= R + 1; r++) fe += mc->h_bctr[(size_t)r * MC_BLIND_COUNTERS + MC_FRAME_ERRORS];
        for (int r = 1; r <= R; r++) {
            pool[r] = h_count[r];
            if (pool[r] > cap) { qldpc_set_error("mc_blind: pool %d holds %llu entries of %zu", r, (unsigned long long)pool[r], cap); return QLDPC_ESTATE; }
        }
        if (cfg->max_frame_errors && fe >= cfg->max_frame_errors) input_left = 0;      /* the input ends here; the pools are flushed, never dropped */
    }
    res->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    for (int r = 0; r <= R + 1; r++) {
        const mc_u64 *c = mc->h_bctr + (size_t)r * MC_BLIND_COUNTERS;
        qldpc_mc_blind_round_stat *st = &mc->bstats[(size_t)r];
        mc_counters_out(st, c);
        st->disclosed = c[MC_DISCLOSED];
        res->frames += st->frames; res->frame_errors += st->frame_errors; res->undetected += st->undetected; res->disclosed += st->disclosed;
    }
    res->open = mc->bstats[(size_t)R + 1].frames;
    res->next_frame = cfg->first_frame + done;
    return QLDPC_OK;
}

extern "C" int qldpc_mc_blind_stats(qldpc_mc *mc, qldpc_mc_blind_round_stat *rows, int cap)
{
    if (!mc) return QLDPC_EINVAL;
    return mc_stats_out(mc->bstats, rows, cap);
}

/* the list of the frames that ended open, `ended` of them, in the order of the launches: the first fail_cap of them by ascending index with their
 * rows (rows may be NULL); writes min(cap, their number) and returns their number */
static int mc_open_out(qldpc_mc *mc, uint64_t ended, const uint64_t *d_frame, const uint32_t *d_rows, uint64_t *frames, uint32_t *rows, int cap)
{
    const size_t Wn = (size_t)mc->Wn;
    const int listed = (int)std::min<uint64_t>(ended, (uint64_t)mc->fail_cap), n = std::min(listed, cap);
    if (n == 0) return listed;
    HIPCHK(hipSetDevice(mc->device));
    HIPCHK(hipStreamSynchronize(mc->dec->stream));
    std::vector<uint64_t> all((size_t)listed);
    HIPCHK(hipMemcpy(all.data(), d_frame, sizeof(uint64_t) * all.size(), hipMemcpyDeviceToHost));
    std::vector<int> order((size_t)listed);      /* the list is in the order of the launches */
    for (int i = 0; i < listed; i++) order[(size_t)i] = i;
    std::sort(order.begin(), order.end(), [&](int a, int b) { return all[(size_t)a] < all[(size_t)b]; });
    for (int i = 0; i < n; i++) {
        frames[i] = all[(size_t)order[(size_t)i]];
        if (rows) HIPCHK(hipMemcpy(rows + (size_t)i * Wn, d_rows + (size_t)order[(size_t)i] * Wn, sizeof(uint32_t) * Wn, hipMemcpyDeviceToHost));
    }
    return listed;
}

extern "C" int qldpc_mc_blind_open(qldpc_mc *mc, uint64_t *frames, uint32_t *known_words, int cap)
{
    if (!mc || cap < 0 || (cap && !frames)) return QLDPC_EINVAL;
    if (mc->bstats.empty()) return 0;
    return mc_open_out(mc, mc->bstats.back().frames, mc->d_oframe, mc->d_oknown, frames, known_words, cap);
}

/* ------------------------------------------------------------------ guessing rounds ---- */

/* everything the guessing rounds need on the device, once and for every g */
static int mc_guess_reserve(qldpc_mc *mc)
{
    HIPCHK(hipSetDevice(mc->device));
    if (mc->guess_ready) return QLDPC_OK;
    const size_t Wn = (size_t)mc->Wn, B = (size_t)mc->batch, cap = MC_GUESS_POOL_CAP(mc->batch), S = B / 2 + 1;
    int rc = QLDPC_OK;
    if ((rc = mc_lazy(mc, &mc->d_bcand, B * Wn)) || (rc = mc_lazy(mc, &mc->d_bweak, B * Wn)) || (rc = mc_lazy(mc, &mc->d_btake, B)) ||
        (rc = mc_lazy(mc, &mc->d_bopen, B)) || (rc = mc_lazy(mc, &mc->d_gframe, cap)) || (rc = mc_lazy(mc, &mc->d_gweak, cap * Wn)) ||
        (rc = mc_lazy(mc, &mc->d_ghard, cap * Wn)) || (rc = mc_lazy(mc, &mc->d_gverd, cap * MC_GUESS_VERDICT)) ||
        (rc = mc_lazy(mc, &mc->d_gkeep, B * MC_GUESS_VERDICT)) || (rc = mc_lazy(mc, &mc->d_gslot, B)) || (rc = mc_lazy(mc, &mc->d_gknown, B * Wn)) ||
        (rc = mc_lazy(mc, &mc->d_gvalue, B * Wn)) || (rc = mc_lazy(mc, &mc->d_gwin, S)) || (rc = mc_lazy(mc, &mc->d_gnok, S)) ||
        (rc = mc_lazy(mc, &mc->d_gamb, S)) || (rc = mc_lazy(mc, &mc->d_gout, S * Wn)) || (rc = mc_lazy(mc, &mc->d_goframe, (size_t)mc->fail_cap)) ||
        (rc = mc_lazy(mc, &mc->d_goweak, (size_t)mc->fail_cap * Wn)) || (rc = mc_lazy(mc, &mc->d_gctr, (size_t)MC_GUESS_WORDS)) ||
        (rc = mc_lazy_pinned(mc, &mc->h_gctr, (size_t)MC_GUESS_WORDS)))
        return rc;
    mc->guess_ready = true;
    return QLDPC_OK;
}

/* every argument check of qldpc_mc_guess: nothing is touched before all of them pass */
static int mc_guess_args(const qldpc_mc *mc, const qldpc_mc_guess_cfg *cfg)
{
    if (cfg->reserved[0] || cfg->reserved[1]) { qldpc_set_error("mc_guess: reserved fields %d, %d must be zero", cfg->reserved[0], cfg->reserved[1]); return QLDPC_EINVAL; }
    if (!(cfg->qber > 0.0 && cfg->qber < 0.5)) { qldpc_set_error("mc_guess: qber=%g outside (0, 0.5)", cfg->qber); return QLDPC_ESIZE; }
    if (cfg->guess_bits < 0 || cfg->guess_bits > QLDPC_GUESS_MAX_BITS) { qldpc_set_error("mc_guess: guess_bits=%d outside 0 .. %d", cfg->guess_bits, QLDPC_GUESS_MAX_BITS); return QLDPC_ESIZE; }
    if ((1 << cfg->guess_bits) > mc->batch) { qldpc_set_error("mc_guess: the %d trials of guess_bits=%d do not fit the batch of %d frames: create the loop with a larger batch", 1 << cfg->guess_bits, cfg->guess_bits, mc->batch); return QLDPC_ESIZE; }
    if ((unsigned)cfg->guess_bits > mc->channel_vns) { qldpc_set_error("mc_guess: guess_bits=%d above the %u channel VNs", cfg->guess_bits, mc->channel_vns); return QLDPC_ESIZE; }
    if (mc->soft) { qldpc_set_error("mc_guess: a channel table is in force; the trials run on the BSC: clear it with qldpc_mc_set_channel(mc, NULL)"); return QLDPC_EUNSUPPORTED; }
    if (mc->dec->engine == QLDPC_ENGINE_EDGES) { qldpc_set_error("mc_guess: the select of the weakest VNs is not built for the edge-parallel engine: create the decoder with engine = FRAMES"); return QLDPC_EUNSUPPORTED; }
    if (mc->dec->compact_mode != 2) {      /* the engine's own rule, resolved when the decoder was created */
        qldpc_set_error("mc_guess: the decoder may compact its active frames (compact = %d), after which the posteriors of the frames that converged earlier are gone: "
                        "create it with compact = 2", mc->dec->cfg.compact);
        return QLDPC_EUNSUPPORTED;
    }
    if (mc->dec->gu.patience > 0 && !mc->dec->freeze) {      /* a frame given up guesses with the posteriors it stopped at: exact only with frozen messages */
        qldpc_set_error("mc_guess: the decoder gives frames up (giveup_patience = %d) and lets their messages run on, so the posteriors a failed frame guesses with "
                        "are not the ones it stopped at: create it with freeze_messages = 1", mc->dec->gu.patience);
        return QLDPC_EUNSUPPORTED;
    }
    return QLDPC_OK;
}

extern "C" int qldpc_mc_guess(qldpc_mc *mc, const qldpc_mc_guess_cfg *cfg, qldpc_mc_guess_result *res)
{
    if (!mc || !cfg || !res) return QLDPC_EINVAL;
    memset(res, 0, sizeof(*res));
    res->next_frame = cfg->first_frame;
    int rc = mc_guess_args(mc, cfg);
    if (rc || (rc = mc_guess_reserve(mc))) return rc;
    const hipStream_t s = mc->dec->stream;
    const int g = cfg->guess_bits, T = 1 << g;
    const size_t Wn = (size_t)mc->Wn, cap = MC_GUESS_POOL_CAP(mc->batch);
    const mc_row row = {mc_threshold(cfg->qber), qldpc_bsc_llr((float)cfg->qber)};
    mc_u64 *const d_rows = mc->d_gctr, *const d_sums = mc->d_gctr + MC_G_POOL;
    const mc_u64 *const h = mc->h_gctr;
    HIPCHK(hipMemsetAsync(mc->d_gctr, 0, sizeof(mc_u64) * MC_GUESS_WORDS, s));
    memset(mc->h_gctr, 0, sizeof(mc_u64) * MC_GUESS_WORDS);
    mc->gstats.assign((size_t)MC_GUESS_ROWS, qldpc_mc_blind_round_stat());

    uint64_t pool = 0, done = 0, input_left = cfg->max_frames;
    int kind = 0, n = 0;
    double *const fresh_stage[7] = {&res->source_ms, &res->encode_ms, &res->channel_ms, &res->load_ms, &res->decode_ms, &res->select_ms, &res->advance_ms};
    double *const trial_stage[8] = {&res->expand_ms, &res->source_ms, &res->encode_ms, &res->channel_ms, &res->load_ms, &res->decode_ms, &res->pick_ms, &res->advance_ms};
    const auto t_start = std::chrono::steady_clock::now();
    while (mc_guess_next(g, mc->batch, pool, input_left, &kind, &n)) {
        HIPCHK(hipEventRecord(mc->ev[0], s));
        if (kind == MC_GUESS_FRESH) {
            const mc_slots sl = {nullptr, cfg->first_frame + done, nullptr, nullptr, row};
            if ((rc = mc_generate_load(mc, sl, n, s, mc->ev, mc->ev[3]))) return rc;
            if (mc->n_fixed && (rc = mc_erase(mc, mc->d_fixed, mc_range(0), n, n, s))) return rc;      /* the fixed puncture set: one row for all n frames */
            HIPCHK(hipEventRecord(mc->ev[4], s));
            if ((rc = qldpc_run(mc->dec))) return rc;
            HIPCHK(hipEventRecord(mc->ev[5], s));
            if ((rc = mc_fetch(mc))) return rc;
            const unsigned total = (unsigned)n * (unsigned)mc->Wn, waves = (unsigned)std::min(n, MC_MAX_WAVES);
            if (g) {
                hipLaunchKernelGGL(mc_blind_cand, dim3(mc_blocks(total)), dim3(MC_LANES), 0, s, (const uint32_t *)mc->d_chan_mask, (const uint32_t *)nullptr,
                                   (const int *)mc->d_ok, mc->d_bcand, mc->d_btake, total, (unsigned)mc->Wn);
                LAUNCHCHK();
                if ((rc = qldpc_fetch_weakest_dev(mc->dec, mc->d_bcand, mc->d_btake, g, mc->d_bweak))) return rc;
            }
            HIPCHK(hipEventRecord(mc->ev[6], s));
            /* the frames that closed onto row 0; with g = 0 the others end open here, else they are pooled and tallied when their trials are through */
            hipLaunchKernelGGL(mc_blind_advance, dim3((waves + 3u) / 4u), dim3(MC_LANES), 0, s, mc_decoded_of(mc), (unsigned)n, (const uint32_t *)nullptr, mc->channel_vns,
                               d_rows, g ? (mc_u64 *)nullptr : d_rows + 2 * MC_BLIND_COUNTERS, mc->d_bopen, (mc_u64 *)nullptr, (mc_u64)0);
            LAUNCHCHK();
            const unsigned groups = ((unsigned)n + MC_APPEND_SLOTS - 1u) / MC_APPEND_SLOTS;
            if (g) {
                hipLaunchKernelGGL(mc_guess_keep, dim3((waves + 3u) / 4u), dim3(MC_LANES), 0, s, mc_decoded_of(mc), (unsigned)n, mc->d_gkeep);
                LAUNCHCHK();
                /* one entry is {frame index, guess row, hard row, verdict}: the ordered append of the blind rounds, once per row array */
                const struct { const uint32_t *src; unsigned words; uint32_t *dst; } part[3] = {
                    {mc->d_bweak, (unsigned)mc->Wn, mc->d_gweak}, {mc->d_out, (unsigned)mc->Wn, mc->d_ghard}, {mc->d_gkeep, MC_GUESS_VERDICT, mc->d_gverd}};
                for (const auto &p : part) {
                    hipLaunchKernelGGL(mc_blind_advance_append, dim3(groups), dim3(MC_LANES), 0, s, (const int *)mc->d_bopen, (unsigned)n, sl, (const uint32_t *)nullptr, p.src,
                                       p.words, mc->d_gframe, p.dst, (mc_u64)pool, (mc_u64)cap, d_sums + (MC_G_POOL - MC_G_POOL));
                    LAUNCHCHK();
                }
            } else {
                hipLaunchKernelGGL(mc_blind_advance_append, dim3(groups), dim3(MC_LANES), 0, s, (const int *)mc->d_bopen, (unsigned)n, sl, (const uint32_t *)nullptr,
                                   (const uint32_t *)nullptr, (unsigned)mc->Wn, mc->d_goframe, mc->d_goweak, h[MC_G_OPEN], (mc_u64)mc->fail_cap, d_sums + (MC_G_OPEN - MC_G_POOL));
                LAUNCHCHK();
            }
            if ((rc = mc_round_end(mc, mc->h_gctr, mc->d_gctr, MC_GUESS_WORDS, fresh_stage, 7, s))) return rc;
            res->decodes += (uint64_t)n;
            done += (uint64_t)n; input_left -= (uint64_t)n;
        } else {
            /* the last n entries of the pool: a contiguous frame table and contiguous row arrays */
            const size_t top = (size_t)pool - (size_t)n;
            const int slots = n * T;
            const mc_slots sl = {mc->d_gslot, 0, nullptr, nullptr, row};
            hipLaunchKernelGGL(mc_guess_slots, dim3(mc_blocks((size_t)slots)), dim3(MC_LANES), 0, s, (const uint64_t *)(mc->d_gframe + top), mc->d_gslot, (unsigned)slots, g);
            LAUNCHCHK();
            if ((rc = qldpc_guess_expand_dev(mc->N, g, n, mc->d_gweak + top * Wn, mc->d_ghard + top * Wn, mc->d_gknown, mc->d_gvalue, (void *)s))) return rc;
            HIPCHK(hipEventRecord(mc->ev[1], s));
            if ((rc = mc_generate_load(mc, sl, slots, s, mc->ev + 1, mc->ev[4]))) return rc;
            if (mc->n_fixed && (rc = mc_erase(mc, mc->d_fixed, mc_range(0), slots, slots, s))) return rc;
            if ((rc = qldpc_load_known_dev(mc->dec, mc->d_gknown, mc->d_gvalue, slots))) return rc;      /* Bob's own guesses: nothing of Alice's is read */
            HIPCHK(hipEventRecord(mc->ev[5], s));
            if ((rc = qldpc_run(mc->dec))) return rc;
            HIPCHK(hipEventRecord(mc->ev[6], s));
            if ((rc = mc_fetch(mc))) return rc;
            if ((rc = qldpc_guess_pick_dev(mc->N, g, n, mc->d_ok, mc->d_out, mc->d_gwin, mc->d_gnok, mc->d_gamb, mc->d_gout, (void *)s))) return rc;
            HIPCHK(hipEventRecord(mc->ev[7], s));
            const unsigned waves = (unsigned)std::min(n, MC_MAX_WAVES);
            hipLaunchKernelGGL(mc_guess_resolve, dim3((waves + 3u) / 4u), dim3(MC_LANES), 0, s, mc_decoded_of(mc), (unsigned)n, g, (const int *)mc->d_gwin, (const int *)mc->d_gnok,
                               (const int *)mc->d_gamb, (const uint32_t *)(mc->d_gverd + top * MC_GUESS_VERDICT), mc->channel_vns, d_rows + MC_BLIND_COUNTERS,
                               d_rows + 2 * MC_BLIND_COUNTERS, d_sums, mc->d_bopen, (mc_u64)top);
            LAUNCHCHK();
            const mc_slots src = {mc->d_gframe + top, 0, nullptr, nullptr, row};
            hipLaunchKernelGGL(mc_blind_advance_append, dim3(((unsigned)n + MC_APPEND_SLOTS - 1u) / MC_APPEND_SLOTS), dim3(MC_LANES), 0, s, (const int *)mc->d_bopen, (unsigned)n, src,
                               (const uint32_t *)nullptr, (const uint32_t *)(mc->d_gweak + top * Wn), (unsigned)mc->Wn, mc->d_goframe, mc->d_goweak, h[MC_G_OPEN],
                               (mc_u64)mc->fail_cap, d_sums + (MC_G_OPEN - MC_G_POOL));
            LAUNCHCHK();
            if ((rc = mc_round_end(mc, mc->h_gctr, mc->d_gctr, MC_GUESS_WORDS, trial_stage, 8, s))) return rc;
            res->decodes += (uint64_t)slots; res->trials += (uint64_t)slots;
        }
        res->launches++;
        pool = h[MC_G_POOL];
        if (pool > cap) { qldpc_set_error("mc_guess: the pool holds %llu entries of %zu", (unsigned long long)pool, cap); return QLDPC_ESTATE; }
        /* an error = a frame closed or rescued wrong, or one that ended open; the input ends here, the pool is flushed, never dropped */
        const uint64_t fe = h[MC_FRAME_ERRORS] + h[MC_BLIND_COUNTERS + MC_FRAME_ERRORS] + h[2 * MC_BLIND_COUNTERS + MC_FRAMES];
        if (cfg->max_frame_errors && fe >= cfg->max_frame_errors) input_left = 0;
    }
    res->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count();
    for (int r = 0; r < MC_GUESS_ROWS; r++) {
        qldpc_mc_blind_round_stat *st = &mc->gstats[(size_t)r];
        mc_counters_out(st, h + (size_t)r * MC_BLIND_COUNTERS);
        st->disclosed = 0;
        res->frames += st->frames; res->frame_errors += st->frame_errors; res->undetected += st->undetected;
    }
    res->rescued = mc->gstats[1].frames; res->open = mc->gstats[2].frames;
    res->trial_iter_sum = h[MC_G_TRIAL_ITER]; res->n_ok_sum = h[MC_G_N_OK]; res->ambiguous = h[MC_G_AMBIGUOUS];
    res->next_frame = cfg->first_frame + done;
    return QLDPC_OK;
}

extern "C" int qldpc_mc_guess_stats(qldpc_mc *mc, qldpc_mc_blind_round_stat *rows, int cap)
{
    if (!mc) return QLDPC_EINVAL;
    return mc_stats_out(mc->gstats, rows, cap);
}

extern "C" int qldpc_mc_guess_open(qldpc_mc *mc, uint64_t *frames, uint32_t *weak_words, int cap)
{
    if (!mc || cap < 0 || (cap && !frames)) return QLDPC_EINVAL;
    if (mc->gstats.empty()) return 0;
    return mc_open_out(mc, mc->gstats.back().frames, mc->d_goframe, mc->d_goweak, frames, weak_words, cap);
}
