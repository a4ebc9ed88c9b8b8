/*
 * qldpc_kernels_polar_recon.h -- the kernels of the polar reconciliation sessions (qldpc_polar_recon_*), gfx950, wave64.  Every rule is
 * qldpc_polar_recon_core.h's; qldpc_polar_recon.hip launches them around the encoder and the decoder of the context a session wraps.
 *
 *   prc_mask      a lane per key word: the word under the block's key mask, into the session's row, which the context's own encode launch then
 *                 turns into u in place.  One line; it exists because that launch takes its rows as they are.
 *   prc_syndrome  a workgroup of 16 waves per 64 blocks.  A wave takes a block at a time: lane l picks bit 64 it + l of the gathered row through
 *                 the position table (fpos[] for the syndrome, the context's info_pos[] for the info row; neighbouring lanes read neighbouring
 *                 table entries and all of them one row of u), a ballot packs 64 of them, and each lane keeps the word that is its own until 64
 *                 words are stored together: every output word is stored once, by a plain vector store.  Behind ONE barrier the first wave runs
 *                 the CRC register over the 64 info rows, a lane per block: serial per block, as the rule is, without every lane of a wave
 *                 repeating it.  The trip counts of the loops around the ballot are the wave's.
 *   prc_prior     a lane per quad of positions, as pmc_channel: ONE store of four int8 (a dword) or four floats (16 bytes), so a wave writes 256 or
 *                 1 024 contiguous bytes of an LLR row; the pad and a refused block are +pin.  The lane also forms its four bits of the frozen row
 *                 (rank = the word's prefix popcount + the frozen positions of the word before them), the eight lanes of a word OR them together by
 *                 shuffles that every lane of the wave takes part in, and the first of them stores the word.
 *   prc_verdict   a lane per block, prc_verdict_block as the mirror runs it: the CRC register over the info row, the pad words of x^ from the top,
 *                 then x^ and the key word by word with the key rewritten in the same pass.  No shuffle, no barrier: a lane may leave early.
 *
 * Indices are 64 bits wide.  No atomics, no spinning, nothing between workgroups, no LDS.
 */
#ifndef QLDPC_KERNELS_POLAR_RECON_H
#define QLDPC_KERNELS_POLAR_RECON_H

#include <hip/hip_runtime.h>

#include <stdint.h>

#include <type_traits>

#include "qldpc_polar_recon_core.h"

#define PRC_LANES 256              /* prc_mask, prc_prior, prc_verdict */
#define PRC_SYN_BLOCKS 64          /* blocks of a workgroup of prc_syndrome: a lane each of its first wave in the CRC phase */
#define PRC_SYN_LANES 1024

/* keys [n][W] -> out [n][W]; total = n W words, W = 1 << lw; key_bits [n] or NULL (every block is N bits) */
__global__ __launch_bounds__(PRC_LANES) void prc_mask(const uint32_t *__restrict__ keys, const int *__restrict__ key_bits, uint32_t *__restrict__ out, size_t total,
                                                      int log2_n, unsigned lw)
{
    const size_t i = (size_t)blockIdx.x * PRC_LANES + threadIdx.x;
    if (i >= total) return;
    const int kb = prc_key_bits(key_bits ? key_bits[i >> lw] : 1 << log2_n, log2_n);
    out[i] = keys[i] & prc_key_mask(kb, (uint32_t)(i & (((size_t)1 << lw) - 1u)));
}

/* the row gathered through pos[count] -> out[ceil(count / 32)], by the 64 lanes of a wave; every lane of the wave calls it with the same arguments */
__device__ static inline void prc_gather_row(const uint32_t *__restrict__ row, const int *__restrict__ pos, unsigned count, uint32_t *__restrict__ out, unsigned lane)
{
    const unsigned its = (count + 63u) / 64u, words = (count + 31u) / 32u;
    uint32_t mine = 0u;
    for (unsigned it = 0; it < its; it++) {
        const unsigned m = it * 64u + lane;
        const unsigned bit = m < count ? prc_pick_bit(row, pos, m) : 0u;
        const unsigned long long b = __ballot((int)bit);                        /* lane l of the ballot is bit l of the 64: MSB-first after the reversal */
        const uint32_t lo = __brev((uint32_t)b), hi = __brev((uint32_t)(b >> 32));
        if ((lane >> 1) == (it & 31u)) mine = lane & 1u ? hi : lo;
        if ((it & 31u) == 31u || it + 1u == its) {                              /* 64 words are complete, or the row is */
            const unsigned j = (it & ~31u) * 2u + lane;
            if (j < words) out[j] = mine;
            mine = 0u;
        }
    }
}

/* u [n][W] (the encoded masked keys) -> syn [n][Wf], info [n][Wi] (the session's scratch) and crc [n].  grid = ceil(n / PRC_SYN_BLOCKS) */
__global__ __launch_bounds__(PRC_SYN_LANES) void prc_syndrome(const uint32_t *__restrict__ u, const int *__restrict__ fpos, const int *__restrict__ ipos,
                                                              uint32_t *info, uint32_t *__restrict__ syn, uint32_t *__restrict__ crc, unsigned n, unsigned W,
                                                              unsigned Nf, unsigned K, int crc_len, uint32_t crc_poly)
{
    const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const size_t b0 = (size_t)blockIdx.x * PRC_SYN_BLOCKS, Wf = pmc_words((int)Nf), Wi = pmc_words((int)K);
    for (unsigned k = wave; k < PRC_SYN_BLOCKS && b0 + k < n; k += PRC_SYN_LANES / 64u) {      /* the wave's own blocks: no lane leaves alone */
        const size_t f = b0 + k;
        prc_gather_row(u + f * W, fpos, Nf, syn + f * Wf, lane);
        prc_gather_row(u + f * W, ipos, K, info + f * Wi, lane);
    }
    __syncthreads();                                          /* the info rows are read by other lanes than wrote them */
    const size_t f = b0 + threadIdx.x;
    if (threadIdx.x < PRC_SYN_BLOCKS && f < n) crc[f] = prc_row_crc(info + f * Wi, (int)K, crc_len, crc_poly);
}

/* keys [n][W], key_bits [n] or NULL, syn [n][Wf] -> llr [n][N] (T = int: int8 levels, T = float) and frozen [n][W].  total = n quads lanes */
template <class T>
__global__ __launch_bounds__(PRC_LANES) void prc_prior(const uint32_t *__restrict__ keys, const int *__restrict__ key_bits, const uint32_t *__restrict__ syn,
                                                       const uint32_t *__restrict__ fmask, const int *__restrict__ fprefix, void *__restrict__ llr,
                                                       uint32_t *__restrict__ frozen, size_t total, int log2_n, unsigned W, unsigned Wf, T prior, T pin)
{
    const size_t i = (size_t)blockIdx.x * PRC_LANES + threadIdx.x;
    const unsigned lq = log2_n >= 2 ? (unsigned)log2_n - 2u : 0u, Qn = 1u << lq, group = Qn < 8u ? Qn : 8u;      /* lanes of a frozen word */
    const bool active = i < total;
    const size_t f = active ? i >> lq : 0u;
    const unsigned q = (unsigned)(i & (Qn - 1u));
    uint32_t fz = 0u;
    if (active) {
        const int kb = prc_key_bits(key_bits ? key_bits[f] : 1 << log2_n, log2_n);
        const uint32_t bits = pmc_quad_bits(keys + f * W, q);
        T l[4];
#pragma unroll
        for (unsigned b = 0; b < 4; b++) l[b] = PRC_LEVEL(4u * q + b, (bits >> (3u - b)) & 1u, kb, prior, pin);
        if constexpr (std::is_same<T, int>::value) {
            int8_t *p = (int8_t *)llr + (f << log2_n) + 4u * (size_t)q;
            if (log2_n >= 2)
                *(uint32_t *)p = ((uint32_t)l[0] & 0xffu) | ((uint32_t)l[1] & 0xffu) << 8 | ((uint32_t)l[2] & 0xffu) << 16 | ((uint32_t)l[3] & 0xffu) << 24;
            else { p[0] = (int8_t)l[0]; p[1] = (int8_t)l[1]; }      /* N = 2: positions 2 and 3 do not exist */
        } else {
            float *p = (float *)llr + (f << log2_n) + 4u * (size_t)q;
            if (log2_n >= 2) *(float4 *)p = make_float4((float)l[0], (float)l[1], (float)l[2], (float)l[3]);
            else { p[0] = (float)l[0]; p[1] = (float)l[1]; }
        }
        const unsigned w = q >> 3;
        fz = prc_frozen_bits(syn + f * Wf, fmask[w], (uint32_t)fprefix[w], (int)(4u * (q & 7u)), 4);
    }
    for (unsigned s = 1; s < group; s <<= 1) fz |= (uint32_t)__shfl_xor((int)fz, (int)s, 64);      /* group is the launch's: every lane shuffles */
    if (active && (q & (group - 1u)) == 0u) frozen[f * W + (q >> 3)] = fz;
}

/* info [n][Wi], x [n][W], pick [n] or NULL, keys [n][W], key_bits [n] or NULL, crc [n] (NULL with pick) -> status [n], corrected [n] or NULL, keys */
__global__ __launch_bounds__(PRC_LANES) void prc_verdict(const uint32_t *__restrict__ info, const uint32_t *__restrict__ x, const int32_t *__restrict__ pick,
                                                         uint32_t *__restrict__ keys, const int *__restrict__ key_bits, const uint32_t *__restrict__ crc,
                                                         int *__restrict__ status, int *__restrict__ corrected, unsigned n, int log2_n, int K, int crc_len,
                                                         uint32_t crc_poly)
{
    const size_t f = (size_t)blockIdx.x * PRC_LANES + threadIdx.x, W = (size_t)pl_words(log2_n), Wi = pmc_words(K);
    if (f >= n) return;
    int st, co;
    prc_verdict_block(log2_n, K, crc_len, crc_poly, info ? info + f * Wi : nullptr, x + f * W, pick != nullptr, pick ? pick[f] : 0, keys + f * W, key_bits ? key_bits[f] : 1 << log2_n,
                      crc ? crc[f] : 0u, &st, &co);
    status[f] = st;
    if (corrected) corrected[f] = co;
}

#endif /* QLDPC_KERNELS_POLAR_RECON_H */
