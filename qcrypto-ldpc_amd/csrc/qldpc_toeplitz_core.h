/*
 * qldpc_toeplitz_core.h -- the arithmetic of the Toeplitz hash (qldpc_toeplitz_*), plain C, shared by the kernel (qldpc_toeplitz.hip)
 * and by its host mirror qldpc_toeplitz_host, so that the CPU suite runs what the lanes run.
 *
 *     y_i = XOR_{j < n} x_j t_{i+j}
 *
 * Key and seed arrive MSB-first (bit k <-> word[k/32] & (1u << (31 - k%32)), helpers.h:65-70).  Inside, both are BIT-REVERSED words
 * (bit b of word k <-> stream bit 32k + b): the 32 seed bits from bit p = 32q + s on are then the low word of {L[q+1], L[q]} >> s with
 * s in 0..31, which is one funnel shift (v_alignbit_b32) for every s, s == 0 included; in the MSB-first order the same window is a shift
 * by 32 - s in 1..32 and s == 0 needs a select.  Reversing costs one scalar instruction per key word (it is wave-uniform) and one vector
 * instruction per seed word staged, not per use.  The parity of key & window does not depend on the bit order.
 */
#ifndef QLDPC_TOEPLITZ_CORE_H
#define QLDPC_TOEPLITZ_CORE_H

#include <stdint.h>

#include "qldpc_hashbatch_core.h"      /* hb_tail_mask: the bits of the last word of a row */

#if defined(__HIPCC__)
#define TZ_FN __host__ __device__ static inline
#else
#define TZ_FN static inline
#endif

#define TZ_MAX_BITS HB_MAX_BITS    /* key_bits and out_bits of a block */
#define tz_tail_mask hb_tail_mask  /* the one tail mask under the name this header gave it: tests/c/toeplitz_sanitize.c checks it by that name */

TZ_FN uint32_t tz_brev(uint32_t x)
{
#if defined(__clang__)
    return __builtin_bitreverse32(x);
#else
    x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
    x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);
    x = ((x >> 4) & 0x0f0f0f0fu) | ((x & 0x0f0f0f0fu) << 4);
    x = ((x >> 8) & 0x00ff00ffu) | ((x & 0x00ff00ffu) << 8);
    return (x >> 16) | (x << 16);
#endif
}

/* the 32 stream bits from bit s (0..31) of lo on; lo, hi: consecutive bit-reversed words */
TZ_FN uint32_t tz_window(uint32_t lo, uint32_t hi, uint32_t s)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(hi, lo, s);                 /* v_alignbit_b32; left to the generic form the compiler shifts 64 bits */
#else
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (s & 31u));
#endif
}

/* one key word (bit-reversed) against its window: acc ^ (key_rev & window) */
TZ_FN uint32_t tz_fold(uint32_t acc, uint32_t key_rev, uint32_t window)
{
#if defined(__HIP_DEVICE_COMPILE__) && __has_builtin(__builtin_amdgcn_bitop3_b32)
    return __builtin_amdgcn_bitop3_b32(acc, key_rev, window, 0x78);      /* one v_bitop3_b32: truth table of a ^ (b & c) with a = 0xf0, b = 0xcc, c = 0xaa */
#else
    return acc ^ (key_rev & window);
#endif
}

TZ_FN uint32_t tz_parity(uint32_t x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__popc(x) & 1u;
#else
    return (uint32_t)__builtin_parity(x);
#endif
}

/* words of a seed of key_bits + out_bits - 1 bits */
TZ_FN uint32_t tz_seed_words(int key_bits, int out_bits)
{
    return key_bits > 0 && out_bits > 0 ? (uint32_t)(((int64_t)key_bits + out_bits - 1 + 31) / 32) : 0u;
}

/*
 * One lane (output bit 32 w + s) over the key words [first, first + count): win[k] is the bit-reversed seed word w + first + k, so the
 * lane reads win[0 .. count].  Key word `last` is the key's last word and is cut to its key bits by tail_mask.  The kernel runs its
 * groups of 8 key words unrolled on the same two functions and the rest of a tile through this loop; the host mirror runs every word here.
 */
TZ_FN uint32_t tz_lane_words(uint32_t acc, const uint32_t *key, uint32_t first, uint32_t count, uint32_t last, uint32_t tail_mask,
                             const uint32_t *win, uint32_t s)
{
    uint32_t lo = win[0];
    for (uint32_t k = 0; k < count; k++) {
        const uint32_t kw = first + k == last ? key[first + k] & tail_mask : key[first + k];
        const uint32_t hi = win[k + 1];
        acc = tz_fold(acc, tz_brev(kw), tz_window(lo, hi, s));
        lo = hi;
    }
    return acc;
}

#endif /* QLDPC_TOEPLITZ_CORE_H */
