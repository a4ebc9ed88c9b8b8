/*
 * qldpc_wave_transpose.h -- the 64 x 64 bit transpose across the lanes of a wave: six butterfly stages (exchange with lane ^ d, keep one half,
 * shift the other in).  A lane gives one 64-bit word, bit = column; afterwards lane c holds column c, and ONE popcount is that column's sum over
 * the wave: a vertical popcount.  Used by the syndrome count of the give-up rule (qldpc_kernels_giveup.h) and by the tally of the polar
 * construction (qldpc_kernels_polar_tally.h).
 */
#ifndef QLDPC_WAVE_TRANSPOSE_H
#define QLDPC_WAVE_TRANSPOSE_H

#include <hip/hip_runtime.h>

/* stage d of the 64 x 64 bit transpose: x = this lane's word, y = the word of lane ^ d */
__device__ __forceinline__ unsigned long long qk_transpose_stage(unsigned long long x, unsigned long long y, int lane, int d)
{
    const unsigned long long m = ~0ull / ((1ull << d) + 1ull);      /* the bit positions with bit d clear */
    return (lane & d) ? ((x & ~m) | ((y >> d) & m)) : ((x & m) | ((y & m) << d));
}
/* bit b of the result in lane l = bit l of x in lane b; every lane of the wave must take part */
__device__ __forceinline__ unsigned long long qk_transpose64(unsigned long long x, int lane)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) x = qk_transpose_stage(x, __shfl_xor(x, d), lane, d);
    return x;
}

#endif /* QLDPC_WAVE_TRANSPOSE_H */
