/*
 * qldpc_mc_core.h -- the frame definition of the Monte-Carlo loop (qldpc_mc_*), plain C, shared by the kernels (qldpc_mc.hip) and by
 * their host mirror (qldpc_mc_host.c), so that the CPU suite runs what the lanes run.
 *
 * Frame i (a 64-bit global index) is a pure function of (seed, i): nothing depends on the batch size, the launch shape or the device.
 *
 *   generator  Philox4x32-10 (Salmon et al., SC'11): multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85,
 *              10 rounds, key = (seed low word, seed high word)
 *   source     info word j of frame i = output word j % 4 at counter (j / 4, 0, i_lo, i_hi); MSB-first (helpers.h:65-70), the bits
 *              past K in the last word cleared
 *   channel    VN v of frame i flips iff u < T[class(v)], u = output word v % 4 at counter (v / 4, 1, i_lo, i_hi),
 *              T = floor(p 2^32) computed in double on the host: p = qber for QLDPC_VN_CHANNEL, parity_ber for QLDPC_VN_PINNED,
 *              0 for QLDPC_VN_PUNCTURED.  A flip probability is exactly T / 2^32; no floating point runs on the device.
 *
 * The class map is handed over PADDED to a multiple of 32 VNs with QLDPC_VN_PUNCTURED (threshold 0: no flip past N), four classes per
 * little-endian word, so that a lane takes the 32 classes of its word with two aligned 16-byte loads.
 */
#ifndef QLDPC_MC_CORE_H
#define QLDPC_MC_CORE_H

#include <stdint.h>

#if defined(__HIPCC__)
#define MC_FN __host__ __device__ static inline
#else
#define MC_FN static inline
#endif

#define MC_PHILOX_M0 0xD2511F53u
#define MC_PHILOX_M1 0xCD9E8D57u
#define MC_PHILOX_W0 0x9E3779B9u
#define MC_PHILOX_W1 0xBB67AE85u

#define MC_STREAM_SOURCE 0u        /* second counter word */
#define MC_STREAM_CHANNEL 1u

MC_FN void mc_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4])
{
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)MC_PHILOX_M0 * c0, p1 = (uint64_t)MC_PHILOX_M1 * c2;      /* v_mul_hi_u32 + v_mul_lo_u32 each */
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += MC_PHILOX_W0; k1 += MC_PHILOX_W1;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

/* the bits of the last word of a row of `bits` bits, MSB-first */
MC_FN uint32_t mc_tail_mask(int bits) { return (bits & 31) ? 0xFFFFFFFFu << (32 - (bits & 31)) : 0xFFFFFFFFu; }

/* T = floor(p 2^32) for p in [0, 1): the product is exact in double (a power-of-two scaling) */
static inline uint32_t mc_threshold(double p) { return (uint32_t)(p * 4294967296.0); }

/* info word j (of ceil(K / 32)) of frame `frame` */
MC_FN uint32_t mc_info_word(uint64_t seed, uint64_t frame, uint32_t j, int K)
{
    uint32_t o[4];
    mc_philox(j >> 2, MC_STREAM_SOURCE, (uint32_t)frame, (uint32_t)(frame >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), o);
    const uint32_t w = o[j & 3u];
    return j == ((uint32_t)K - 1u) / 32u ? w & mc_tail_mask(K) : w;
}

/* flip word w (VNs 32 w .. 32 w + 31) of frame `frame`: cls4[g] = the classes of VNs 32 w + 4 g .. + 3, one per byte, lowest byte first;
 * t_channel / t_pinned = the thresholds of the two classes that can flip.  8 Philox calls; a call whose four VNs cannot flip is skipped. */
MC_FN uint32_t mc_flip_word(uint64_t seed, uint64_t frame, uint32_t w, const uint32_t cls4[8], uint32_t t_channel, uint32_t t_pinned)
{
    uint32_t flips = 0;
    for (uint32_t g = 0; g < 8; g++) {
        uint32_t t[4], o[4];
        for (uint32_t b = 0; b < 4; b++) {
            const uint32_t c = (cls4[g] >> (8u * b)) & 0xffu;
            t[b] = c == 0u ? t_channel : (c == 1u ? t_pinned : 0u);
        }
        if ((t[0] | t[1] | t[2] | t[3]) == 0u) continue;
        mc_philox(8u * w + g, MC_STREAM_CHANNEL, (uint32_t)frame, (uint32_t)(frame >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), o);
        for (uint32_t b = 0; b < 4; b++)
            if (o[b] < t[b]) flips |= 0x80000000u >> (4u * g + b);
    }
    return flips;
}

/*
 * Host side.  The padded class map cls[32 ceil(N / 32)] of a (K, N, info_bits_pos, vn_class): vn_class != NULL is copied (every entry 0 .. 2), else the
 * harness's classes (BS/src/main.cpp:348-354): QLDPC_VN_CHANNEL at info_bits_pos (NULL = 0 .. K-1), QLDPC_VN_PINNED elsewhere.  mask
 * (optional, ceil(N / 32) words) = the packed mask of info_bits_pos.  Returns 0, or -1 for a position outside [0, N), a repeated position or
 * a class above 2.
 */
static inline int mc_classes(int K, int N, const int *info_bits_pos, const uint8_t *vn_class, uint8_t *cls, uint32_t *mask)
{
    const int Wn = (N + 31) / 32;
    for (int v = 0; v < 32 * Wn; v++) cls[v] = v < N ? 1 : 2;
    if (mask) for (int w = 0; w < Wn; w++) mask[w] = 0;
    for (int i = 0; i < K; i++) {
        const int v = info_bits_pos ? info_bits_pos[i] : i;
        if (v < 0 || v >= N || cls[v] == 0) return -1;
        cls[v] = 0;
        if (mask) mask[v >> 5] |= 0x80000000u >> (v & 31);
    }
    if (vn_class)
        for (int v = 0; v < N; v++) {
            if (vn_class[v] > 2) return -1;
            cls[v] = vn_class[v];
        }
    return 0;
}

/* cls (padded, one class per byte) -> the four-per-word form of mc_flip_word; no assumption on the host's byte order */
static inline void mc_pack_classes(const uint8_t *cls, int Wn, uint32_t *cls4)
{
    for (int g = 0; g < 8 * Wn; g++)
        cls4[g] = (uint32_t)cls[4 * g] | (uint32_t)cls[4 * g + 1] << 8 | (uint32_t)cls[4 * g + 2] << 16 | (uint32_t)cls[4 * g + 3] << 24;
}

#endif /* QLDPC_MC_CORE_H */
