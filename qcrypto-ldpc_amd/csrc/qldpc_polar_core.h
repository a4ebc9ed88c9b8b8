/*
 * qldpc_polar_core.h -- the definition of the polar encoder and of the successive-cancellation (SC) decoder of qldpc_polar_*.  Plain C, shared by
 * the kernels (qldpc_kernels_polar.h) and by their host mirrors (qldpc_polar_host.c), so that the CPU suite runs what the lanes run.
 *
 *   size       N = 2^n, 1 <= n <= PL_MAX_LOG2N.  Index i is natural order, no bit reversal.  Rows are packed MSB-first: bit i of a row is
 *              word[i / 32] & (1u << (31 - i % 32)); a row has ceil(N / 32) words and the bits past N are zero.
 *   encode     for m = 1, 2, .., N/2: in every block of 2m bits the first half becomes first ^ second (x = u F^{(x)n}, an involution).  The stages
 *              m < 32 work inside a word (pl_enc_word: partner i + m is m places to the RIGHT of i), the stages m >= 32 XOR whole words.
 *   decode     at a node of size s with beliefs L[0 .. s): a = L[0 .. s/2), b = L[s/2 .. s).
 *                left child   f(a, b) = sgn(a) sgn(b) min(|a|, |b|), sgn(v) = -1 iff v < 0: 0 and -0.0 count as positive
 *                right child  g(a, b, c) = sat(b + (1 - 2c) a), c = the RE-ENCODED decisions of the left child
 *                result       [c_left ^ c_right, c_right]
 *              leaf: frozen -> the given frozen value (0 without one); else bit = (L < 0), so L = 0 decides 0.
 *   I8         sat clamps to [-(maxq + 1), maxq]; f is NOT saturated (f(-32, -32) = +32 at maxq = 31), so beliefs live in [-(maxq + 1), maxq + 1]
 *              and maxq <= PL_MAX_MAXQ = 126 keeps them in an int8.  Inputs are int8 levels, clamped into [-(maxq + 1), maxq] on load.
 *   F32        sat is the identity, g is ONE float add or subtract (compile with -ffp-contract=off), inputs finite.
 *   outputs    u (all N decisions), info (bit m = u[info_pos[m]], the caller's order: pl_info_word), x (the root's re-encoded word), leaf (the N
 *              leaf beliefs).
 *
 * The traversal is the same for every frame; only the values differ.  Both sides run it by leaf blocks of PL_SUB = min(N, 32) leaves: the decisions of
 * a block are one packed word, its re-encoded word is pl_enc_word of that, and everything above a block is word XORs (pl_combine_words).
 */
#ifndef QLDPC_POLAR_CORE_H
#define QLDPC_POLAR_CORE_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PL_FN __host__ __device__ static inline
#else
#define PL_FN static inline
#endif

#define PL_MAX_LOG2N 20
#define PL_MAX_MAXQ 126            /* f gives maxq + 1, which has to fit an int8 */
#define PL_SUB_LOG 5               /* a leaf block: 32 leaves, one packed word */

PL_FN int pl_words(int log2_n) { return log2_n <= 5 ? 1 : 1 << (log2_n - 5); }
/* leaves of a leaf block, and its log */
PL_FN int pl_sub_log(int log2_n) { return log2_n < PL_SUB_LOG ? log2_n : PL_SUB_LOG; }

/* ---- messages ---- */
PL_FN int pl_i8_load(int v, int maxq) { return v > maxq ? maxq : (v < -(maxq + 1) ? -(maxq + 1) : v); }
PL_FN int pl_i8_f(int a, int b)
{
    const int ma = a < 0 ? -a : a, mb = b < 0 ? -b : b, m = ma < mb ? ma : mb;
    return ((a < 0) != (b < 0)) ? -m : m;
}
PL_FN int pl_i8_g(int a, int b, unsigned c, int maxq) { return pl_i8_load(c ? b - a : b + a, maxq); }
PL_FN float pl_f32_f(float a, float b)
{
    const float ma = __builtin_fabsf(a), mb = __builtin_fabsf(b), m = ma < mb ? ma : mb;
    return ((a < 0.0f) != (b < 0.0f)) ? -m : m;
}
PL_FN float pl_f32_g(float a, float b, unsigned c) { return c ? b - a : b + a; }
/* a leaf's decision from its belief's sign (neg = L < 0), its frozen flag and its frozen value */
PL_FN unsigned pl_leaf_bit(unsigned neg, unsigned frozen, unsigned value) { return frozen ? value : neg; }
/* the frozen flags of a leaf block of one frame in the rows form: the code's word, and what the frame's own row adds to it (a row never thaws) */
PL_FN uint32_t pl_rows_frozen(uint32_t code_word, uint32_t row_word) { return code_word | row_word; }

/* ---- the encoder ---- */
/* the stages m = 1 .. 2^(sub_log - 1) of a word whose top 2^sub_log bits are in use (sub_log <= 5) */
PL_FN uint32_t pl_enc_word(uint32_t w, int sub_log)
{
    static const uint32_t first[5] = {0xaaaaaaaau, 0xccccccccu, 0xf0f0f0f0u, 0xff00ff00u, 0xffff0000u};      /* the first halves of the blocks of 2m bits */
    for (int s = 0; s < sub_log; s++) w ^= (w << (1u << s)) & first[s];
    return w;
}
/* the bit i % 32 of a word, MSB-first */
PL_FN unsigned pl_bit(uint32_t w, int i) { return (w >> (31 - (i & 31))) & 1u; }
/* the valid bits of the only word of a row of N < 32 bits, all ones otherwise */
PL_FN uint32_t pl_row_mask(int log2_n) { return log2_n >= 5 ? 0xffffffffu : 0xffffffffu << (32 - (1 << log2_n)); }

/* After leaf block j (a word at x[j * stride]) has been written re-encoded: every node that ends with block j is combined, smallest first -- a node
 * of 2h words ending at word j gets first half ^= second half.  `stride`: words between neighbouring words of the row (1 on the host, 64 where a
 * wave interleaves its frames). */
PL_FN void pl_combine_words(uint32_t *x, long j, long stride)
{
    for (long h = 1; j & h; h <<= 1)
        for (long k = 0; k < h; k++) x[(j + 1 - 2 * h + k) * stride] ^= x[(j + 1 - h + k) * stride];
}
/* the level whose beliefs g produces before leaf block j > 0, in blocks: 2^t blocks, t = the trailing zeros of j */
PL_FN int pl_ctz(long j) { return __builtin_ctzl((unsigned long)j); }

/* ---- the outputs ---- */
/* packed word w of a frame's info row: bit b = u[info_pos[32 w + b]], u the words U[k * stride] (stride 64 where a wave interleaves its frames) */
PL_FN uint32_t pl_info_word(const uint32_t *U, size_t stride, const int *info_pos, int n_info, size_t w)
{
    uint32_t word = 0u;
    for (size_t b = 0; b < 32u && w * 32u + b < (size_t)n_info; b++) {
        const int p = info_pos[w * 32u + b];
        word |= pl_bit(U[(size_t)(p >> 5) * stride], p) << (31 - b);
    }
    return word;
}

/* ---- argument checks: 0 or a qldpc_status value (QLDPC_EINVAL -1, QLDPC_ESIZE -6); qldpc_polar_int.h's helpers word the refusals ---- */
#define PL_EINVAL (-1)
#define PL_ESIZE (-6)
PL_FN int pl_check_size(int log2_n, int max_log2_n) { return log2_n >= 1 && log2_n <= max_log2_n ? 0 : PL_ESIZE; }
PL_FN int pl_check_maxq(int messages, int maxq) { return messages != 0 || (maxq >= 1 && maxq <= PL_MAX_MAXQ) ? 0 : PL_ESIZE; }
/* info_pos[n_info] distinct and below N, marked in `info_mask` (ceil(N / 32) zeroed words, MSB-first) */
PL_FN int pl_mark_info(int log2_n, int n_info, const int *info_pos, uint32_t *info_mask)
{
    const long N = 1l << log2_n;
    if (n_info < 0 || n_info > N || (n_info > 0 && !info_pos)) return PL_ESIZE;
    for (int m = 0; m < n_info; m++) {
        const int p = info_pos[m];
        if (p < 0 || p >= N) return PL_ESIZE;
        const uint32_t bit = 1u << (31 - (p & 31));
        if (info_mask[p >> 5] & bit) return PL_EINVAL;
        info_mask[p >> 5] |= bit;
    }
    return 0;
}

/* ---- what the host mirrors are made of: each is a macro X(SUF, TIN, T, LOAD, F, G) that defines the functions of one message type, with
 * TIN the type of the caller's rows, T the type a belief is computed in, and LOAD / G used where an `int maxq` is in scope ---- */
#define PL_I8_LOAD(v) pl_i8_load((int)(v), maxq)
#define PL_I8_G(a, b, c) pl_i8_g((a), (b), (c), maxq)
#define PL_F32_LOAD(v) (v)
#define PL_HOST_MESSAGES(X)                                \
    X(i8, int8_t, int, PL_I8_LOAD, pl_i8_f, PL_I8_G)       \
    X(f32, float, float, PL_F32_LOAD, pl_f32_f, pl_f32_g)

/* The recursion inside a leaf block, as a lane holds it in registers: a node of s <= 32 leaves whose first leaf is bit pos (MSB-first) of the
 * block's words, beliefs L[s] -> decisions into *u, the re-encoded bits of every finished node into *x, leaf beliefs into leaf[] (or NULL) */
#define PL_HOST_LEAF_BLOCK(SUF, TIN, T, LOAD, F, G)                                                                                        \
    static void pl_node_##SUF(int maxq, const T *L, int s, int pos, uint32_t frozen, uint32_t value, uint32_t *u, uint32_t *x, TIN *leaf)  \
    {                                                                                                                                      \
        (void)maxq;                                                                                                                        \
        if (s == 1) {                                                                                                                      \
            const uint32_t bit = pl_leaf_bit(L[0] < 0, pl_bit(frozen, pos), pl_bit(value, pos));                                           \
            *u |= bit << (31 - pos);                                                                                                       \
            *x |= bit << (31 - pos);                                                                                                       \
            if (leaf) leaf[pos] = (TIN)L[0];                                                                                               \
            return;                                                                                                                        \
        }                                                                                                                                  \
        const int h = s / 2;                                                                                                               \
        T l[16] = {0};                                                                                                                     \
        for (int k = 0; k < h; k++) l[k] = F(L[k], L[k + h]);                                                                              \
        pl_node_##SUF(maxq, l, h, pos, frozen, value, u, x, leaf);                                                                         \
        for (int k = 0; k < h; k++) l[k] = G(L[k], L[k + h], pl_bit(*x, pos + k));                                                         \
        pl_node_##SUF(maxq, l, h, pos + h, frozen, value, u, x, leaf);                                                                     \
        *x ^= (*x << h) & ((0xffffffffu << (32 - h)) >> pos);                                                                              \
    }

#endif /* QLDPC_POLAR_CORE_H */
