/*
 * qldpc_toeplitz_ntt_core.h -- the arithmetic of the sub-quadratic Toeplitz hash (QLDPC_TOEPLITZ_NTT), plain C, shared by the pass kernels
 * (qldpc_toeplitz_ntt.hip) and by their host mirror qldpc_toeplitz_ntt_host, so that the CPU suite runs what the lanes run.
 *
 * y_i = XOR_j x_j t_(i+j) is the low bit of the integer correlation c_i = SUM_j x_j t_(i+j) <= n <= 2^24, and a cyclic convolution of
 * length L >= n + m - 1 over Z_p, p = 15 * 2^27 + 1 > 2^24, gives c_i exactly:
 *
 *     a_((k + d) mod L) = x_(n-1-k)  (k < n, else 0),   b_k = t_k  (k < the seed bits, else 0),   (a * b)_((n-1+d+i) mod L) = c_i
 *
 * d = (-(n-1)) mod 32 turns the key so that the outputs start at a multiple of 32: an output word is then 32 consecutive residues of one
 * tile and is stored whole.  A cyclic shift of a shifts the product and nothing else, so the words do not depend on d, and seed bits at
 * index >= n + m - 1 only reach product indices outside the m that are read.  L is a power of two, at least 32 (one output word).
 *
 * Residues are canonical, in [0, p), everywhere; twiddles are kept in Montgomery form (w * 2^32 mod p), so tzn_mont(x, w) is the plain
 * product x * w.  Conditional corrections are selects: nothing here branches on, or addresses with, a value derived from the key.
 *
 * A transform of length 2^k runs as P = ceil(k / B) passes.  Pass 0 takes the top b0 = k - (P-1) B index bits (the ragged one), every
 * later pass the next B bits down: a pass over the index bits [sh, sh + b) is a 2^b-point transform of the rows t for every column
 * (hi, lo) = (bits above, bits below), followed in the forward direction by the factor w_(2^(sh+b))^(f lo), f the frequency the row
 * now holds.  Forward passes are decimation in frequency and leave bit-reversed rows; the inverse undoes them step by step in the opposite
 * order (factor, then decimation in time), so no permutation pass exists.  A tile is 2^(B+5) residues (all of a short transform): all
 * rows of as many adjacent columns as fit, in address order, so a tile is runs of at least 32 adjacent residues.
 */
#ifndef QLDPC_TOEPLITZ_NTT_CORE_H
#define QLDPC_TOEPLITZ_NTT_CORE_H

#include <stdint.h>

#if defined(__HIPCC__)
#define TZN_FN __host__ __device__ static inline
#else
#define TZN_FN static inline
#endif

#define TZN_P 2013265921u          /* 15 * 2^27 + 1 */
#define TZN_PINV 2281701377u       /* p^-1 mod 2^32 */
#define TZN_R1 268435454u          /* 2^32 mod p: 1 in Montgomery form */
#define TZN_R2 1172168163u         /* 2^64 mod p */
#define TZN_GEN 31u                /* a primitive root of p */
#define TZN_MIN_LOG2 5             /* L >= 32 */
#define TZN_MAX_LOG2 25            /* L <= 2^25: n, m <= 2^24 */
#define TZN_COLS_LOG2 5            /* a tile of the B instance is 2^(B + 5) residues */

TZN_FN uint32_t tzn_add(uint32_t a, uint32_t b)
{
    const uint32_t s = a + b;                                    /* < 2p < 2^32 */
    return s - (s >= TZN_P ? TZN_P : 0u);
}

TZN_FN uint32_t tzn_sub(uint32_t a, uint32_t b)
{
    return a - b + (a < b ? TZN_P : 0u);
}

/* a b 2^-32 mod p for a b < 2^32 p, in [0, p) */
TZN_FN uint32_t tzn_mont(uint32_t a, uint32_t b)
{
    const uint64_t t = (uint64_t)a * b;
    const uint32_t m = (uint32_t)t * TZN_PINV;                   /* m p == t mod 2^32, so the low words cancel */
    const uint32_t hi = (uint32_t)(t >> 32), u = (uint32_t)(((uint64_t)m * TZN_P) >> 32);
    return hi - u + (hi < u ? TZN_P : 0u);
}

/* the plain product a b mod p */
TZN_FN uint32_t tzn_mul(uint32_t a, uint32_t b) { return tzn_mont(tzn_mont(a, b), TZN_R2); }

TZN_FN uint32_t tzn_pow(uint32_t a, uint32_t e)
{
    uint32_t r = 1u;
    for (; e; e >>= 1, a = tzn_mul(a, a))
        if (e & 1u) r = tzn_mul(r, a);
    return r;
}

/* a primitive 2^log2_len-th root of unity, log2_len <= 27 (plain form) */
TZN_FN uint32_t tzn_root(uint32_t log2_len) { return tzn_pow(TZN_GEN, (TZN_P - 1u) >> log2_len); }

/* what the last inverse pass multiplies by: L^-1, and 2^32 again for the 2^-32 the pointwise tzn_mont of the two spectra left */
TZN_FN uint32_t tzn_scale(uint32_t k)
{
    const uint32_t linv = tzn_pow(1u << k, TZN_P - 2u);
    return tzn_mul(tzn_mul(linv, TZN_R1), TZN_R1);
}

/* decimation in frequency / in time on a pair; w in Montgomery form */
TZN_FN void tzn_dif(uint32_t *u, uint32_t *v, uint32_t w)
{
    const uint32_t a = *u, b = *v;
    *u = tzn_add(a, b);
    *v = tzn_mont(tzn_sub(a, b), w);
}

TZN_FN void tzn_dit(uint32_t *u, uint32_t *v, uint32_t w)
{
    const uint32_t a = *u, b = tzn_mont(*v, w);
    *u = tzn_add(a, b);
    *v = tzn_sub(a, b);
}

/* log2 of the transform length of a block: the smallest power of two >= n + m - 1, at least 32; -1 where the block has no seed */
TZN_FN int tzn_log2_len(int key_bits, int out_bits)
{
    if (key_bits <= 0 || out_bits <= 0) return -1;
    const uint32_t need = (uint32_t)key_bits + (uint32_t)out_bits - 1u;
    int k = TZN_MIN_LOG2;
    while ((1u << k) < need) k++;
    return k;
}

/* the turn of the key and where output bit 0 then lies */
TZN_FN uint32_t tzn_turn(uint32_t n) { return (32u - ((n - 1u) & 31u)) & 31u; }
TZN_FN uint32_t tzn_out_base(uint32_t n, uint32_t k) { return (n - 1u + tzn_turn(n)) & ((1u << k) - 1u); }

/* ---- the pass decomposition ---- */

typedef struct {
    uint32_t k, sh, b;             /* the transform is 2^k long; this pass works on the index bits [sh, sh + b) */
    uint32_t le;                   /* a tile is 2^le residues */
    uint32_t sp;                   /* tile position bits: [low sp column bits][b row bits][the other column bits] */
} tzn_pass;

TZN_FN uint32_t tzn_passes(uint32_t k, uint32_t B) { return (k + B - 1u) / B; }

TZN_FN tzn_pass tzn_pass_of(uint32_t k, uint32_t B, uint32_t pass)
{
    const uint32_t P = tzn_passes(k, B), tile = B + TZN_COLS_LOG2;
    tzn_pass ps;
    ps.k = k;
    ps.b = pass ? B : k - (P - 1u) * B;
    ps.sh = (P - 1u - pass) * B;
    ps.le = tile < k ? tile : k;
    ps.sp = ps.sh < ps.le - ps.b ? ps.sh : ps.le - ps.b;
    return ps;
}

/* position e of tile `tile` -> index in the transform; *lo: the index bits below the pass (the exponent of the factor) */
TZN_FN uint32_t tzn_index(tzn_pass ps, uint32_t tile, uint32_t e, uint32_t *lo)
{
    const uint32_t c = ((e >> (ps.sp + ps.b)) << ps.sp) | (e & ((1u << ps.sp) - 1u));
    const uint32_t t = (e >> ps.sp) & ((1u << ps.b) - 1u);
    const uint32_t col = (tile << (ps.le - ps.b)) + c;
    *lo = col & ((1u << ps.sh) - 1u);
    return ((col >> ps.sh) << (ps.sh + ps.b)) | (t << ps.sh) | *lo;
}

/* butterfly u of the stage whose pairs lie 2^lh rows apart -> the position of its upper element; the lower one is 1 << (sp + lh) on */
TZN_FN uint32_t tzn_pair(tzn_pass ps, uint32_t u, uint32_t lh)
{
    const uint32_t z = ps.sp + lh;
    return ((u >> z) << (z + 1u)) | (u & ((1u << z) - 1u));
}

/* its twiddle w_(2^(lh+1))^(row mod 2^lh) as an index into the table of w_(2^B)^x, x < 2^(B-1) */
TZN_FN uint32_t tzn_pair_twiddle(tzn_pass ps, uint32_t pos, uint32_t lh, uint32_t B)
{
    return ((pos >> ps.sp) & ((1u << lh) - 1u)) << (B - 1u - lh);
}

/* the exponent x of the factor w_(2^kmax)^x between passes for position e: (frequency of the row) * lo, scaled to the table's root */
TZN_FN uint32_t tzn_factor(tzn_pass ps, uint32_t e, uint32_t lo, uint32_t kmax)
{
    const uint32_t t = (e >> ps.sp) & ((1u << ps.b) - 1u);
#if defined(__clang__)
    const uint32_t f = __builtin_bitreverse32(t) >> (32u - ps.b);        /* rows are left bit-reversed; b >= 1 */
#else
    uint32_t f = 0;
    for (uint32_t i = 0; i < ps.b; i++) f |= ((t >> i) & 1u) << (ps.b - 1u - i);
#endif
    return (f * lo) << (kmax - ps.sh - ps.b);
}

/* w^x (forward) or w^-x (inverse) from the two-level table: lo[x mod 2^kl] * hi[x >> kl], both in Montgomery form, as is the result */
TZN_FN uint32_t tzn_twiddle(const uint32_t *lo, const uint32_t *hi, uint32_t kl, uint32_t kmax, uint32_t x, int inverse)
{
    if (inverse) x = ((1u << kmax) - x) & ((1u << kmax) - 1u);
    return tzn_mont(lo[x & ((1u << kl) - 1u)], hi[x >> kl]);
}

TZN_FN uint32_t tzn_table_split(uint32_t kmax) { return (kmax + 1u) / 2u; }

/* ---- bits <-> residues; rows are MSB-first ---- */

TZN_FN uint32_t tzn_bit(const uint32_t *words, uint32_t i) { return (words[i >> 5] >> (31u - (i & 31u))) & 1u; }

/* a_g: the key reversed and turned by d = tzn_turn(n); no word past bit n - 1 is read */
TZN_FN uint32_t tzn_key_residue(const uint32_t *key, uint32_t n, uint32_t k, uint32_t g)
{
    const uint32_t q = (g - tzn_turn(n)) & ((1u << k) - 1u);
    const uint32_t in = q < n ? 1u : 0u;
    return tzn_bit(key, in ? n - 1u - q : 0u) & in;
}

/* b_g: seed bit g of the first seed_bits, which is at least 1 */
TZN_FN uint32_t tzn_seed_residue(const uint32_t *seed, uint32_t seed_bits, uint32_t g)
{
    const uint32_t in = g < seed_bits ? 1u : 0u;
    return tzn_bit(seed, in ? g : 0u) & in;
}

/* transform index -> output bit index; an output where it is < m */
TZN_FN uint32_t tzn_out_index(uint32_t n, uint32_t k, uint32_t g) { return (g - tzn_out_base(n, k)) & ((1u << k) - 1u); }

/* the output bit of a residue of the unscaled inverse: the low bit of the canonical value.  tzn_mont returns it in [0, p); a value left in
   [p, 2p) would have the other parity, p being odd */
TZN_FN uint32_t tzn_out_bit(uint32_t residue, uint32_t scale) { return tzn_mont(residue, scale) & 1u; }

#endif /* QLDPC_TOEPLITZ_NTT_CORE_H */
