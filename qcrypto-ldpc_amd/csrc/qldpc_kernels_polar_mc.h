/*
 * qldpc_kernels_polar_mc.h -- the kernels of the Monte-Carlo loop around the polar decoders (qldpc_polar_mc_*), gfx950.  Every rule is
 * qldpc_polar_mc_core.h's; qldpc_polar_mc.hip launches them between the encoder and the decoder of the context the loop runs around.
 *
 *   pmc_source   a wave per frame: the message words by Philox, their CRC (every lane runs the register over the words its neighbours hold, so the
 *                remainder is wave-uniform and nothing goes through memory), the info row, and behind a barrier the u row as a gather through
 *                rank[].  Every output word is stored once; no atomics.
 *   pmc_channel  a lane per quad of positions, the table in LDS once per workgroup: one Philox call, four levels, ONE store of four int8 (a dword)
 *                or of four floats (16 bytes), so a wave writes 256 or 1 024 contiguous bytes of a row.  The flip counts of a frame's lanes are
 *                summed by shuffles; one atomic add per wave (or per frame, where a wave holds several) goes to the frame's slot.
 *   pmc_monitor  a lane per frame: the verdict, the tallies summed over the wave and added to the ONE counter row by one atomic a wave and counter,
 *                a fail flag per frame and the failed frames of the workgroup as one count.
 *   pmc_append   the failed frames of a batch, in frame order, become entries base, base + 1, .. of the list: a wave per 64 frames counts the
 *                failures before its frames (the workgroup counts of pmc_monitor, then the flags of the started workgroup) and ballots its own,
 *                as mc_blind_advance_append of the LDPC loop does.  No returning atomic: the order does not depend on the launch.
 */
#ifndef QLDPC_KERNELS_POLAR_MC_H
#define QLDPC_KERNELS_POLAR_MC_H

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "qldpc_polar_mc_core.h"

#define PMC_LANES 256              /* pmc_channel, pmc_monitor */
#define PMC_WAVE 64                /* pmc_source: a frame; pmc_append: 64 frames */

typedef unsigned long long pmc_u64;

/* the counter row on the device: the first seven of QLDPC_POLAR_MC_* in include/qldpc.h's order (batches and next_frame are the host's) */
enum { PMC_C_FRAMES = 0, PMC_C_BIT_ERRORS, PMC_C_FRAME_ERRORS, PMC_C_UNDETECTED, PMC_C_CRC_FAILS, PMC_C_FLIPS, PMC_C_CHANNEL_BITS, PMC_C_DEVICE, PMC_C_ROW = 16 };

__device__ static inline unsigned pmc_wave_sum(unsigned v)
{
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}

/* info [n][Wi] (Wi = pmc_words(K)) and, unless u is NULL, u [n][W]; rank[32 W], fmask[W] (1 = frozen).  grid = n frames, PMC_WAVE lanes */
__global__ __launch_bounds__(PMC_WAVE) void pmc_source(uint32_t *__restrict__ info, uint32_t *__restrict__ u, const int *__restrict__ rank,
                                                       const uint32_t *__restrict__ fmask, unsigned W, int A, int K, int crc_len, uint32_t crc_poly,
                                                       int frozen_mode, int source, uint64_t seed, uint64_t first)
{
    const unsigned f = blockIdx.x, lane = threadIdx.x, Wa = pmc_words(A), Wi = pmc_words(K);
    const uint64_t frame = first + f;
    uint32_t *row = info + (size_t)f * Wi;
    uint32_t r = 0u;
    if (crc_len)
        for (unsigned j0 = 0; j0 < Wa; j0 += PMC_WAVE) {      /* 64 message words at a time, one a lane; the trip counts are the wave's */
            const uint32_t word = j0 + lane < Wa ? pmc_msg_word(seed, frame, j0 + lane, A, source) : 0u;
            const unsigned cnt = min((unsigned)PMC_WAVE, Wa - j0);
            for (unsigned k = 0; k < cnt; k++) r = pmc_crc_word(r, (uint32_t)__shfl((int)word, (int)k, 64), pmc_msg_bits(j0 + k, A), crc_len, crc_poly);
        }
    for (unsigned j = lane; j < Wi; j += PMC_WAVE) row[j] = pmc_info_word(j < Wa ? pmc_msg_word(seed, frame, j, A, source) : 0u, j, A, crc_len, r);
    if (!u) return;
    __syncthreads();                                          /* the row is read by other lanes than wrote it */
    for (unsigned w = lane; w < W; w += PMC_WAVE)
        u[(size_t)f * W + w] = pmc_u_word(row, rank + 32u * (size_t)w, frozen_mode == PMC_FROZEN_RANDOM ? pmc_frozen_word(seed, frame, w) & fmask[w] : 0u);
}

/* x [n][W] -> llr [n][N] int8 (I8) or float, and flips[n] (zeroed before the launch); either may be NULL.  total = n << lq lanes, lq = log2 of the
 * quads of a frame.  No lane leaves before the shuffles: the last workgroup's spare lanes carry no flips. */
template <bool I8>
__global__ __launch_bounds__(PMC_LANES) void pmc_channel(const uint32_t *__restrict__ x, void *__restrict__ llr, uint32_t *__restrict__ flips,
                                                         const mc_soft_table *__restrict__ tab, unsigned total, int log2_n, unsigned W, uint64_t seed,
                                                         uint64_t first)
{
    static_assert(PMC_LANES == MC_SOFT_MAX_LEVELS, "pmc_channel loads one table entry per lane");
    __shared__ uint32_t thr[2][MC_SOFT_MAX_LEVELS];
    __shared__ float value[MC_SOFT_MAX_LEVELS];
    __shared__ uint32_t live[2];
    const unsigned t = threadIdx.x;
    thr[0][t] = t < MC_SOFT_MAX_LEVELS - 1 ? tab->thr[0][t] : 0xFFFFFFFFu;
    thr[1][t] = t < MC_SOFT_MAX_LEVELS - 1 ? tab->thr[1][t] : 0xFFFFFFFFu;
    value[t] = tab->value[t];
    if (t < 2) live[t] = tab->live[t];
    __syncthreads();
    const unsigned i = blockIdx.x * PMC_LANES + t, lq = log2_n >= 2 ? (unsigned)log2_n - 2u : 0u, Qn = 1u << lq;
    const bool active = i < total;
    const unsigned f = active ? i >> lq : 0u, q = i & (Qn - 1u);
    unsigned fl = 0u;
    if (active) {
        float l[4];
        fl = pmc_quad(seed, first + f, q, pmc_quad_bits(x + (size_t)f * W, q), pmc_quad_valid(log2_n), thr[0], live[0], thr[1], live[1], value, l);
        if (llr && I8) {
            int8_t *p = (int8_t *)llr + ((size_t)f << log2_n) + 4u * (size_t)q;
            if (log2_n >= 2)
                *(uint32_t *)p = ((uint32_t)pmc_i8(l[0]) & 0xffu) | ((uint32_t)pmc_i8(l[1]) & 0xffu) << 8 | ((uint32_t)pmc_i8(l[2]) & 0xffu) << 16 | ((uint32_t)pmc_i8(l[3]) & 0xffu) << 24;
            else { p[0] = (int8_t)pmc_i8(l[0]); p[1] = (int8_t)pmc_i8(l[1]); }      /* N = 2: positions 2 and 3 do not exist */
        } else if (llr) {
            float *p = (float *)llr + ((size_t)f << log2_n) + 4u * (size_t)q;
            if (log2_n >= 2) *(float4 *)p = make_float4(l[0], l[1], l[2], l[3]);
            else { p[0] = l[0]; p[1] = l[1]; }
        }
    }
    if (!flips) return;
    if (Qn >= 64u) {                                          /* a wave lies inside one frame, and is all active or all spare */
        fl = pmc_wave_sum(fl);
        if ((t & 63u) == 0u && fl) atomicAdd(flips + f, fl);
    } else {                                                  /* a frame is Qn neighbouring lanes of one wave */
        for (unsigned s = 1; s < Qn; s <<= 1) fl += __shfl_xor(fl, (int)s, 64);
        if (active && q == 0u && fl) atomicAdd(flips + f, fl);
    }
}

/* dec, sent [n][Wi] info rows, pick[n] or NULL, flips[n] -> the counter row, fail[n] (1 = a frame error) and wg_fail[gridDim.x] */
__global__ __launch_bounds__(PMC_LANES) void pmc_monitor(const uint32_t *__restrict__ dec, const uint32_t *__restrict__ sent, const int32_t *__restrict__ pick,
                                                         const uint32_t *__restrict__ flips, unsigned n, unsigned Wi, int A, unsigned N,
                                                         pmc_u64 *__restrict__ ctr, uint32_t *__restrict__ fail, uint32_t *__restrict__ wg_fail)
{
    __shared__ unsigned part[PMC_LANES / 64];
    const unsigned t = threadIdx.x, f = blockIdx.x * PMC_LANES + t, Wa = pmc_words(A);
    const bool active = f < n;
    unsigned be = 0u, fl = 0u, crcf = 0u;
    if (active) {
        const size_t row = (size_t)f * Wi;
        for (unsigned j = 0; j < Wa; j++) be += (unsigned)__popc((dec[row + j] ^ sent[row + j]) & (j == Wa - 1u ? mc_tail_mask(A) : 0xFFFFFFFFu));
        fl = flips[f];
        crcf = pick && pick[f] < 0;
        fail[f] = be > 0u;
    }
    const unsigned fe = be > 0u, ud = fe & (crcf ^ 1u);
    const unsigned frames = pmc_wave_sum(active), s_be = pmc_wave_sum(be), s_fe = pmc_wave_sum(fe), s_ud = pmc_wave_sum(ud), s_cf = pmc_wave_sum(crcf),
                   s_fl = pmc_wave_sum(fl);
    if ((t & 63u) == 0u) {
        part[t >> 6] = s_fe;
        if (frames) {
            atomicAdd(ctr + PMC_C_FRAMES, (pmc_u64)frames);
            atomicAdd(ctr + PMC_C_CHANNEL_BITS, (pmc_u64)frames * N);
        }
        if (s_be) atomicAdd(ctr + PMC_C_BIT_ERRORS, (pmc_u64)s_be);
        if (s_fe) atomicAdd(ctr + PMC_C_FRAME_ERRORS, (pmc_u64)s_fe);
        if (s_ud) atomicAdd(ctr + PMC_C_UNDETECTED, (pmc_u64)s_ud);
        if (s_cf) atomicAdd(ctr + PMC_C_CRC_FAILS, (pmc_u64)s_cf);
        if (s_fl) atomicAdd(ctr + PMC_C_FLIPS, (pmc_u64)s_fl);
    }
    __syncthreads();
    if (t == 0u) {
        unsigned c = 0u;
        for (unsigned w = 0; w < PMC_LANES / 64; w++) c += part[w];
        wg_fail[blockIdx.x] = c;
    }
}

/* workgroup b (one wave) takes frames 64 b .. 64 b + 63 of the n of a batch whose first frame is `first`; entries at `cap` and beyond are not
 * written */
__global__ __launch_bounds__(PMC_WAVE) void pmc_append(const uint32_t *__restrict__ fail, const uint32_t *__restrict__ wg_fail, unsigned n, uint64_t first,
                                                       pmc_u64 base, pmc_u64 cap, pmc_u64 *__restrict__ list)
{
    const unsigned lane = threadIdx.x, f0 = blockIdx.x * PMC_WAVE, whole = f0 / PMC_LANES;      /* monitor workgroups that end before f0 */
    unsigned c = 0u;
    for (unsigned i = lane; i < whole; i += PMC_WAVE) c += wg_fail[i];
    for (unsigned i = whole * PMC_LANES + lane; i < f0; i += PMC_WAVE) c += fail[i];
    c = pmc_wave_sum(c);
    const unsigned f = f0 + lane;
    const bool flag = f < n && fail[min(f, n - 1u)] != 0u;
    const unsigned long long flags = __ballot(flag);
    const pmc_u64 e = base + c + (unsigned)__popcll(flags & ((1ull << lane) - 1ull));
    if (flag && e < cap) list[e] = first + f;
}

#endif /* QLDPC_KERNELS_POLAR_MC_H */
