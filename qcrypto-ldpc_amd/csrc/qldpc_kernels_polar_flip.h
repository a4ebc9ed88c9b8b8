/*
 * qldpc_kernels_polar_flip.h -- the kernels of SC-Flip trials in the polar reconciliation sessions (qldpc_polar_recon_decode_flip,
 * qldpc_polar_flip_select_dev), gfx950, wave64.  Every rule is qldpc_polar_flip_core.h's.  qldpc_polar_recon.hip launches them around the rows form
 * of the SC decoder, on the blocks that failed only.
 *
 *   pfl_first_verdict  the first pass of a call that does not resume: a lane per block, pld_entry and prc_verdict_block on the block's own rows
 *                      (slot b = block b), the decode count, and the open list of the blocks that failed (pld_append).
 *   pfl_select         a wave per slot: the slot's T flips from its leaf row.  T passes; in a pass every lane strides the row with vector loads
 *                      (16 bytes of int8 leaves, a float4 of float ones), keeps the smallest key at or above the pass's floor
 *                      (pfl_pass_key), and a butterfly of 64-bit minima leaves the wave's in every lane.  T N / 64 leaves a lane, and only
 *                      failed blocks pay it.  Rows shorter than a vector are read a leaf a lane.
 *   pfl_trial_prior    pld_slot_prior_lane (qldpc_kernels_polar_ladder.h, the body of pld_slot_prior) for trial j of a chunk: the inputs of
 *                      block open[j / T] plus the flip pos[j] and its value from the probe's leaf row j / T.  A void trial gets the base inputs.
 *   pfl_settle         a lane per trial: prc_accept_block on the trial's rows, a ballot, the block's T-lane field of it (void trials never
 *                      accept), its lowest set bit.  The winning lane, or the block's first lane where nobody wins, writes status, corrected,
 *                      flip_pos, the key and the decode count.
 *
 * Control flow is wave-uniform wherever a ballot or a shuffle follows: a lane past the end takes part with nothing to add.  T is a power of two
 * up to 32 and a workgroup holds a multiple of 64 lanes, so the T trials of a block are one aligned run of lanes inside a wave.  Indices are 64
 * bits wide; no spinning, no LDS, nothing between workgroups but pld_append's counter.
 */
#ifndef QLDPC_KERNELS_POLAR_FLIP_H
#define QLDPC_KERNELS_POLAR_FLIP_H

#include "qldpc_kernels_polar_ladder.h"
#include "qldpc_polar_flip_core.h"

/* slot b = block b: info [n][Wi], x [n][W] -> status, corrected (or NULL), decodes (or NULL), keys, and the open list with *count (zero before).
   extra: [n] or NULL (every count 0), only read */
__global__ __launch_bounds__(PRC_LANES) void pfl_first_verdict(const uint32_t *__restrict__ info, const uint32_t *__restrict__ x, uint32_t *__restrict__ keys,
                                                               const int *__restrict__ key_bits, const uint32_t *__restrict__ crc, const int *__restrict__ extra,
                                                               int *__restrict__ status, int *__restrict__ corrected, int *__restrict__ decodes, int *__restrict__ open,
                                                               int *__restrict__ count, unsigned n, int log2_n, int K, int crc_len, uint32_t crc_poly, int n_extra)
{
    const size_t b = (size_t)blockIdx.x * PRC_LANES + threadIdx.x, W = (size_t)pl_words(log2_n), Wi = pmc_words(K);
    bool failed = false;
    if (b < n) {
        const int kb = key_bits ? key_bits[b] : 1 << log2_n;
        int st = PRC_ESIZE, co = -1;
        const bool valid = pld_entry(0, 0, kb, log2_n, extra ? extra[b] : 0, n_extra) == PLD_OPEN;
        if (valid) prc_verdict_block(log2_n, K, crc_len, crc_poly, info + b * Wi, x + b * W, 0, 0, keys + b * W, kb, crc[b], &st, &co);
        status[b] = st;
        if (corrected) corrected[b] = co;
        if (decodes) decodes[b] = valid ? 1 : 0;
        failed = st == PRC_EDECODE;
    }
    pld_append(failed, (int)b, open, count);
}

__device__ static inline uint64_t pfl_wave_min(uint64_t v)
{
#pragma unroll
    for (int k = 32; k >= 1; k >>= 1) {
        const uint64_t o = (uint64_t)__shfl_xor((unsigned long long)v, k, 64);
        v = o < v ? o : v;
    }
    return v;
}

/* leaf [n_slots][N] (16-byte aligned), fmask [W], rank [N] or NULL, extra or NULL, open or NULL (the count of slot s is extra[open[s]], or
   extra[s]) -> pos [n_slots][T]; grid = ceil(n_slots / 4), 256 lanes: a wave per slot */
template <class E>
__global__ __launch_bounds__(PRC_LANES) void pfl_select(const E *__restrict__ leaf, const uint32_t *__restrict__ fmask, const int *__restrict__ rank,
                                                        const int *__restrict__ extra, const int *__restrict__ open, int *__restrict__ pos, unsigned n_slots, int log2_n, int T)
{
    constexpr bool i8 = std::is_same<E, int8_t>::value;
    constexpr unsigned VEC = i8 ? 16u : 4u;                      /* leaves of a 16-byte load */
    const unsigned lane = threadIdx.x & 63u;
    const size_t s = (size_t)blockIdx.x * (PRC_LANES / 64u) + (threadIdx.x >> 6), N = (size_t)1 << log2_n;
    if (s >= n_slots) return;                                    /* the whole wave */
    const int ex = extra && rank ? extra[open ? open[s] : (int)s] : 0;
    const bool ranked = rank && ex > 0;                          /* the wave's: without it no rank is below the count */
    const E *row = leaf + s * N;
    uint64_t lo = 0u;
    for (int t = 0; t < T; t++) {                                /* lo and best are the wave's after the reduction: every lane goes round T times */
        uint64_t best = PFL_NO_KEY;
        if (lo != PFL_NO_KEY) {
            if (N >= VEC) {
                for (size_t v = lane; v * VEC < N; v += 64u) {
                    const size_t i0 = v * VEC;
                    const uint32_t fw = fmask[i0 >> 5];
                    uint32_t mag[VEC];
                    if constexpr (i8) {
                        const uint4 q = *(const uint4 *)(row + i0);
                        const uint32_t w4[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                        for (unsigned k = 0; k < VEC; k++) mag[k] = pfl_mag_i8((int)(int8_t)(w4[k >> 2] >> (8u * (k & 3u))));
                    } else {
                        const float4 q = *(const float4 *)(row + i0);
                        mag[0] = pfl_mag_f32(q.x); mag[1] = pfl_mag_f32(q.y); mag[2] = pfl_mag_f32(q.z); mag[3] = pfl_mag_f32(q.w);
                    }
#pragma unroll
                    for (unsigned k = 0; k < VEC; k++) {
                        const size_t i = i0 + k;
                        const uint64_t key = pfl_pass_key(mag[k], i, pl_bit(fw, (int)(i & 31u)), ranked ? rank[i] : PLD_NO_RANK, ex, lo);
                        best = key < best ? key : best;
                    }
                }
            } else if (lane < N) {                               /* a row shorter than a vector: a leaf a lane */
                const uint32_t mag = i8 ? pfl_mag_i8((int)row[lane]) : pfl_mag_f32((float)row[lane]);
                best = pfl_pass_key(mag, lane, pl_bit(fmask[0], (int)lane), ranked ? rank[lane] : PLD_NO_RANK, ex, lo);
            }
        }
        best = pfl_wave_min(best);
        if (lane == 0u) pos[s * (size_t)T + (size_t)t] = pfl_pass_pos(best);
        lo = pfl_pass_next(best);
    }
}

/* trial j = block open[j / T] with the flip pos[j]: as pld_slot_prior, slots 0 .. n_trials - 1; leaf [n_trials / T][N]: the probe's rows.
   total = n_trials quads lanes; Tlog = log2 T */
template <class T, class E>
__global__ __launch_bounds__(PRC_LANES) void pfl_trial_prior(const int *__restrict__ open, const int *__restrict__ pos, const E *__restrict__ leaf,
                                                             const uint32_t *__restrict__ keys, const int *__restrict__ key_bits, const uint32_t *__restrict__ syn,
                                                             const uint32_t *__restrict__ xbits, const int *__restrict__ extra, const uint32_t *__restrict__ fmask,
                                                             const int *__restrict__ fprefix, const int *__restrict__ rank, void *__restrict__ llr,
                                                             uint32_t *__restrict__ frozen, uint32_t *__restrict__ flags, size_t total, int log2_n, unsigned W, unsigned Wf,
                                                             unsigned We, int Tlog, T prior, T pin)
{
    const size_t i = (size_t)blockIdx.x * PRC_LANES + threadIdx.x;
    const unsigned lq = log2_n >= 2 ? (unsigned)log2_n - 2u : 0u;
    const bool active = i < total;
    const size_t j = active ? i >> lq : 0u, c = j >> Tlog;
    size_t b = 0u;
    int flip = -1;
    unsigned bit = 0u;
    if (active) {
        b = (size_t)open[c];
        flip = pos[j];
        if (flip >= 0) {
            const E l = leaf[(c << log2_n) + (size_t)flip];
            if constexpr (std::is_same<E, int8_t>::value) bit = pfl_flip_bit_i8((int)l);
            else bit = pfl_flip_bit_f32(l);
        }
    }
    pld_slot_prior_lane<T>(active, j, (unsigned)(i & ((1u << lq) - 1u)), b, flip, bit, keys, key_bits, syn, xbits, extra, fmask, fprefix, rank, llr, frozen, flags, nullptr,
                           log2_n, W, Wf, We, prior, pin);
}

/* trial j: info [n_trials][Wi], x [n_trials][W], pos [n_trials] -> status, corrected (or NULL), flip_pos, decodes (or NULL) and keys of block
   open[j / T]; n_trials is a multiple of T = 1 << Tlog */
__global__ __launch_bounds__(PRC_LANES) void pfl_settle(const int *__restrict__ open, const int *__restrict__ pos, const uint32_t *__restrict__ info,
                                                        const uint32_t *__restrict__ x, uint32_t *__restrict__ keys, const int *__restrict__ key_bits,
                                                        const uint32_t *__restrict__ crc, int *__restrict__ status, int *__restrict__ corrected, int32_t *__restrict__ flip_pos,
                                                        int *__restrict__ decodes, size_t n_trials, int log2_n, int K, int crc_len, uint32_t crc_poly, int Tlog)
{
    const size_t j = (size_t)blockIdx.x * PRC_LANES + threadIdx.x, W = (size_t)pl_words(log2_n), Wi = pmc_words(K);
    const unsigned lane = threadIdx.x & 63u, T = 1u << Tlog, t = lane & (T - 1u);
    const bool active = j < n_trials;
    bool accept = false;
    size_t b = 0u;
    int p = -1, kb = 0;
    if (active) {
        b = (size_t)open[j >> Tlog];
        p = pos[j];
        kb = key_bits ? key_bits[b] : 1 << log2_n;
        accept = p >= 0 && prc_accept_block(log2_n, K, crc_len, crc_poly, info + j * Wi, x + j * W, 0, 0, kb, crc[b]);
    }
    const unsigned long long all = __ballot((int)accept);        /* every lane of the wave */
    const int win = pfl_winner((uint32_t)(all >> (lane - t)) & (T == 32u ? 0xffffffffu : (1u << T) - 1u));
    if (active && t == (unsigned)(win >= 0 ? win : 0)) {         /* one lane a block */
        int co = -1;
        if (win >= 0) co = prc_take_block(log2_n, x + j * W, keys + b * W, kb);
        status[b] = win >= 0 ? PRC_OK : PRC_EDECODE;
        if (corrected) corrected[b] = co;
        flip_pos[b] = win >= 0 ? p : -1;
        if (decodes) decodes[b] += 1 + (int)T;
    }
}

#endif /* QLDPC_KERNELS_POLAR_FLIP_H */
