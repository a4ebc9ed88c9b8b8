/*
 * qldpc_polar_mc_core.h -- the frame definition of the Monte-Carlo loop around the polar decoders (qldpc_polar_mc_*).  Plain C on top of
 * qldpc_mc_core.h (mc_philox, mc_info_word, mc_soft_level, mc_soft_table) and qldpc_polar_list_core.h (the CRC's register step, the packing),
 * shared by the kernels (qldpc_kernels_polar_mc.h) and by their host mirror (qldpc_polar_mc_host.c), so that the CPU suite runs what the lanes run.
 *
 * Frame i (a 64-bit global index) is a pure function of (seed, i, code, CRC, frozen mode, table): nothing depends on the batch, the launch shape
 * or how a run is split into calls.  Rows are packed MSB-first as everywhere in the polar subsystem.
 *
 *   message    A = n_info - crc_len bits; word j = mc_info_word(seed, i, j, A): stream 0, the LDPC loop's source.  PMC_SOURCE_ZERO: zeros.
 *   info row   K = n_info bits: the message, then its CRC remainder (pll_crc_step: register form, zero start) appended MSB first, so that the
 *              remainder of the whole row is 0 and the list decoder is handed no crc row.  crc_len = 0 (every SC context): A = K.
 *   u          u[info_pos[m]] = info bit m, written as a gather through rank[position] = m, or -1 at a frozen position.
 *              PMC_FROZEN_ZERO    frozen positions are 0; the decoder gets no frozen row.
 *              PMC_FROZEN_RANDOM  frozen word w = output word w % 4 at counter (w / 4, 4, i_lo, i_hi), masked to the frozen positions; the u
 *                                 row itself is the decoder's frozen row.  x = encode(u) is then a uniformly random word: the reconciliation
 *                                 form, with Alice's frozen values.  Stream 4 is this loop's own: no other frame moves.
 *   x          encode(u)
 *   channel    one threshold table of 2 .. 256 levels, qldpc_mc_set_channel's: position v draws u = output word v % 4 at counter
 *              (v / 4, 3, i_lo, i_hi), level = #{k : u >= cum[x_v][k]}, LLR = value[level]; int8 messages store (int8)value[level], and every
 *              value must then be an integer in [-128, 127].  flips = the positions whose LLR's sign contradicts x_v; an LLR of 0 contradicts
 *              nothing.  No floating point is computed on the device.
 *   verdict    be = popcount over the A message bits of (decoded info ^ sent info); frame error iff be > 0; crc_fail iff the list decoder's pick
 *              is -1; undetected iff a frame error that is no crc_fail.
 */
#ifndef QLDPC_POLAR_MC_CORE_H
#define QLDPC_POLAR_MC_CORE_H

#include "qldpc_mc_core.h"
#include "qldpc_polar_list_core.h"

#define PMC_STREAM_FROZEN 4u       /* second counter word */
enum { PMC_FROZEN_ZERO = 0, PMC_FROZEN_RANDOM = 1 };      /* QLDPC_POLAR_MC_FROZEN_* of include/qldpc.h */
enum { PMC_SOURCE_RANDOM = 0, PMC_SOURCE_ZERO = 1 };      /* QLDPC_MC_SOURCE_* */

/* words of a row of `bits` bits */
MC_FN uint32_t pmc_words(int bits) { return ((uint32_t)bits + 31u) / 32u; }

/* message word j (of pmc_words(A), A >= 1) of frame `frame` */
MC_FN uint32_t pmc_msg_word(uint64_t seed, uint64_t frame, uint32_t j, int A, int source)
{
    return source == PMC_SOURCE_ZERO ? 0u : mc_info_word(seed, frame, j, A);
}

/* the bits of message word j that belong to the message: 32, fewer in the last word */
MC_FN int pmc_msg_bits(uint32_t j, int A) { return (int)(j + 1u) * 32 <= A ? 32 : A - (int)j * 32; }

/* the CRC register after the top `bits` bits of a word */
MC_FN uint32_t pmc_crc_word(uint32_t r, uint32_t word, int bits, int crc_len, uint32_t crc_poly)
{
    for (int b = 0; b < bits; b++) r = pll_crc_step(r, (word >> (31 - b)) & 1u, crc_len, crc_poly);
    return r;
}

/* word j of the info row: the message word (0 past the message) and the bits of the remainder that fall into it, bit A of the row = the
 * remainder's top bit.  crc_len <= 32, so the remainder touches words A / 32 and A / 32 + 1 at the most */
MC_FN uint32_t pmc_info_word(uint32_t msg_word, uint32_t j, int A, int crc_len, uint32_t crc)
{
    if (crc_len == 0) return msg_word;
    const uint64_t c = ((uint64_t)crc << (64 - crc_len)) >> (A & 31);
    const uint32_t ja = (uint32_t)A >> 5;
    return msg_word | (j == ja ? (uint32_t)(c >> 32) : 0u) | (j == ja + 1u ? (uint32_t)c : 0u);
}

/* frozen-stream word w of frame `frame`, before the frozen mask */
MC_FN uint32_t pmc_frozen_word(uint64_t seed, uint64_t frame, uint32_t w)
{
    uint32_t o[4];
    mc_philox(w >> 2, PMC_STREAM_FROZEN, (uint32_t)frame, (uint32_t)(frame >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), o);
    return o[w & 3u];
}

/* a word of the u row: rank32 = the rank entries of its 32 positions (-1: frozen, or past N), info = the frame's info row, frozen_bits = its frozen
 * values, already masked (0 with PMC_FROZEN_ZERO) */
MC_FN uint32_t pmc_u_word(const uint32_t *info, const int *rank32, uint32_t frozen_bits)
{
    uint32_t word = frozen_bits;
    for (int b = 0; b < 32; b++) {
        const int m = rank32[b];
        if (m >= 0) word |= pl_bit(info[m >> 5], m) << (31 - b);
    }
    return word;
}

/* quads of a frame, and the positions of a quad that exist: N / 4 and 4, but 1 and 2 at N = 2 */
MC_FN uint32_t pmc_quads(int log2_n) { return log2_n >= 2 ? 1u << (log2_n - 2) : 1u; }
MC_FN uint32_t pmc_quad_valid(int log2_n) { return log2_n >= 2 ? 4u : 2u; }
/* the x bits of quad q, position 4 q + b at bit 3 - b, from the frame's x row */
MC_FN uint32_t pmc_quad_bits(const uint32_t *x, uint32_t q) { return (x[q >> 3] >> (28u - 4u * (q & 7u))) & 0xfu; }

/* positions 4 q .. 4 q + 3 of frame `frame`: bits = their x bits (pmc_quad_bits), valid = how many of them exist; thr0 / thr1 / value = the table
 * (LDS in the kernel).  Writes the four LLRs (0 where no position is) and returns the number of contradicted positions.  One Philox call. */
MC_FN uint32_t pmc_quad(uint64_t seed, uint64_t frame, uint32_t q, uint32_t bits, uint32_t valid, const uint32_t *thr0, uint32_t live0,
                        const uint32_t *thr1, uint32_t live1, const float *value, float llr[4])
{
    uint32_t o[4], flips = 0;
    mc_philox(q, MC_STREAM_SOFT, (uint32_t)frame, (uint32_t)(frame >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), o);
    for (uint32_t b = 0; b < 4; b++) {
        const uint32_t sent = (bits >> (3u - b)) & 1u;
        const float l = b < valid ? value[sent ? mc_soft_level(thr1, live1, o[b]) : mc_soft_level(thr0, live0, o[b])] : 0.0f;
        llr[b] = l;
        flips += (uint32_t)(sent ? l > 0.0f : l < 0.0f);
    }
    return flips;
}

/* the int8 a table value is stored as with int8 messages (pmc_table_build has checked that it is one) */
MC_FN int pmc_i8(float v) { return (int)v; }

/* ---- host side ---- */

/* mc_soft_table_build, and with int8 messages the rule on the values.  Returns 0, -1 for levels outside 2 .. 256, -2 for a missing array, a
 * decreasing row or an entry above 2^32, -3 for a value that is no integer in [-128, 127]; the table is written only on 0 */
static inline int pmc_table_build(int i8, int levels, const uint64_t *cum0, const uint64_t *cum1, const float *value, mc_soft_table *t)
{
    if (levels < 2 || levels > MC_SOFT_MAX_LEVELS) return -1;
    if (!cum0 || !cum1 || !value) return -2;
    for (int l = 0; l < levels && i8; l++)
        if (!(value[l] >= -128.0f && value[l] <= 127.0f) || (float)(int)value[l] != value[l]) return -3;
    return mc_soft_table_build(levels, cum0, cum1, value, t);
}

/* rank[32 W]: position -> m where info_pos[m] is the position, -1 elsewhere and past N (info_pos checked: distinct and below N) */
static inline void pmc_rank(int log2_n, int n_info, const int *info_pos, int *rank)
{
    const long entries = 32l * pl_words(log2_n);
    for (long p = 0; p < entries; p++) rank[p] = -1;
    for (int m = 0; m < n_info; m++) rank[info_pos[m]] = m;
}

#endif /* QLDPC_POLAR_MC_CORE_H */
