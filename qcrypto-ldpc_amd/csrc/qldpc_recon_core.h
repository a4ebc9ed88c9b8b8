/*
 * qldpc_recon_core.h -- the arithmetic the two sides of a reconciliation session must agree on, plain C, shared by the kernels and the host code of
 * qldpc_recon.hip and compiled on its own by the CPU suite (tests/c/recon_sanitize.c), so that each piece is stated once:
 *
 *   CRC-32   (IEEE 802.3, reflected) over key words fed MSB-first, bits past n_bits masked to 0: serial, and as the chunked fold the kernels run
 *   puncture the evenly spaced puncturing pattern of (M, p) and its two directions, position -> rank (Bob, rk_assemble) and rank -> position
 *            (Alice, rk_disclose)
 *   staging  the layout of a staging block, the same in the pinned host block and in the device block
 */
#ifndef QLDPC_RECON_CORE_H
#define QLDPC_RECON_CORE_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RC_FN __host__ __device__ static inline
#else
#define RC_FN static inline
#endif

#define CRC_POLY 0xEDB88320u      /* CRC-32 (IEEE 802.3), reflected */

/* entry `byte` of the 256-entry table of the byte-wise recurrence */
RC_FN uint32_t crc_table_entry(uint32_t byte)
{
    uint32_t c = byte;
    for (int k = 0; k < 8; k++) c = (c & 1u) ? CRC_POLY ^ (c >> 1) : c >> 1;
    return c;
}
/* the register after the four bytes of word x, most significant first */
RC_FN uint32_t crc_word_step(uint32_t c, uint32_t x, const uint32_t *t)
{
    for (int b = 3; b >= 0; b--) c = t[(c ^ (x >> (8 * b))) & 0xFF] ^ (c >> 8);
    return c;
}
/* the bits of word i of nw that lie below n_bits */
RC_FN uint32_t tail_mask(int i, int nw, int n_bits)
{
    return (i == nw - 1 && (n_bits & 31)) ? 0xFFFFFFFFu << (32 - (n_bits & 31)) : 0xFFFFFFFFu;
}
RC_FN uint32_t crc_serial(const uint32_t *w, int n_bits, const uint32_t *t)
{
    uint32_t c = 0xFFFFFFFFu;
    const int nw = (n_bits + 31) / 32;
    for (int i = 0; i < nw; i++) c = crc_word_step(c, w[i] & tail_mask(i, nw, n_bits), t);
    return c ^ 0xFFFFFFFFu;
}

/*
 * The same CRC computed in parallel: the register is linear over GF(2) in (start value, message), so with start value 0 the
 * register after A || B is reg(A) x^|B| + reg(B) (polynomials mod the CRC polynomial) and the start value 0xFFFFFFFF adds
 * 0xFFFFFFFF x^|message|.  Every lane runs the byte-wise recurrence over its own chunk (chunks of equal length; zero words in
 * front of the message leave a zero register alone), the partial registers are folded in a tree -- the same jump-ahead idea the
 * privacy-amplification kernel uses for the LFSR -- and the two constants are applied at the end.  In the reflected form bit 31
 * is the coefficient of x^0 and multiplying by x is a right shift.
 */
RC_FN uint32_t gf_mulmod(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int i = 0; i < 32; i++) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ CRC_POLY : (b >> 1);
    }
    return p;
}
/* x^n mod the CRC polynomial */
RC_FN uint32_t gf_xpow(unsigned long long n)
{
    uint32_t r = 0x80000000u, sq = 0x40000000u;      /* 1, x */
    while (n) {
        if (n & 1ull) r = gf_mulmod(r, sq);
        sq = gf_mulmod(sq, sq);
        n >>= 1;
    }
    return r;
}
/* words per chunk when nw words are dealt to `lanes` chunks; *pad = the zero words in front of the message */
RC_FN int crc_chunk_words(int nw, int lanes, int *pad)
{
    const int c = (nw + lanes - 1) / lanes;
    *pad = c * lanes - nw;
    return c;
}
/* the CRC from the folded register of a message of nw words: start value and final xor */
RC_FN uint32_t crc_close(uint32_t reg, int nw)
{
    return reg ^ gf_mulmod(0xFFFFFFFFu, gf_xpow(32ull * (unsigned long long)nw)) ^ 0xFFFFFFFFu;
}
/* `lanes` (a power of two) chunks folded in a tree, as a workgroup of the kernels does it; t = the table, reg = scratch of `lanes` words */
RC_FN uint32_t crc_chunked(const uint32_t *w, int n_bits, int lanes, const uint32_t *t, uint32_t *reg)
{
    const int nw = (n_bits + 31) / 32;
    int pad;
    const int c = crc_chunk_words(nw, lanes, &pad);
    for (int l = 0; l < lanes; l++) {
        reg[l] = 0;
        for (int v = l * c; v < (l + 1) * c; v++) {
            const int i = v - pad;
            if (i >= 0) reg[l] = crc_word_step(reg[l], w[i] & tail_mask(i, nw, n_bits), t);
        }
    }
    uint32_t X = gf_xpow(32ull * (unsigned long long)c);
    for (int s = 1; s < lanes; s <<= 1) {
        for (int l = 0; l + s < lanes; l += 2 * s) reg[l] = gf_mulmod(reg[l], X) ^ reg[l + s];
        X = gf_mulmod(X, X);
    }
    return crc_close(reg[0], nw);
}

/*
 * Punctured parity positions of a block: p of the M accumulator bits, evenly spaced (position j is punctured iff
 * floor((j + 1) p / M) > floor(j p / M)), so no check loses both of its parity neighbours while p <= M / 2 and the pattern needs
 * no table or seed: both sides compute it from (M, p).  The reference shuffles the parity positions at random and searches for
 * good patterns (BS/src/main.cpp:305-333); on this accumulator structure random patterns fail where the even one decodes
 * (tools/punct_probe.py: 37 % punctured at QBER 4 %: FER 0.07 random, 0 even; 49 % at 3 %: 1.0 vs 0).
 */
RC_FN int punct_before(int j, int p, int M) { return (int)(((long long)j * p) / M); }      /* punctured positions in [0, j) */
RC_FN int punct_at(int j, int p, int M) { return punct_before(j + 1, p, M) > punct_before(j, p, M); }
/* a disclosed position's place among the disclosed bits */
RC_FN int punct_rank(int j, int p, int M) { return j - punct_before(j, p, M); }
/* the r-th disclosed position (r < M - p): smallest j with (j + 1) - punct_before(j + 1) == r + 1 */
RC_FN int punct_position(int r, int p, int M)
{
    int lo = r, hi = r + p;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (mid + 1 - punct_before(mid + 1, p, M) >= r + 1) hi = mid; else lo = mid + 1;
    }
    return lo;
}

/*
 * The staging blocks of a job of n blocks on a code of Wk key words and Wm parity words, as 32-bit words from `base`:
 *   in      keys [n][Wk] | disclosed parity [n][Wm] | |LLR| [n] | block length [n] | punctured [n] | Alice's CRC [n]
 *   Bob     verified key words [n][Wk] | status [n] | bits flipped [n] | iterations [n] | CRC found [n]
 *   Alice   disclosed parity [n][Wm] | CRC [n]
 * A NULL base gives the word count alone (the columns stay NULL).
 */
#define RC_COL(type, base, off) ((base) ? (type *)(void *)((base) + (off)) : (type *)0)

typedef struct recon_in_view {
    uint32_t *keys, *disc;
    float *mag;
    int *key_bits, *n_punct;
    uint32_t *crc;
    size_t words;
} recon_in_view;
RC_FN recon_in_view recon_in_layout(uint32_t *base, int n, int Wk, int Wm)
{
    const size_t N = (size_t)n, disc = N * (size_t)Wk, mag = disc + N * (size_t)Wm;
    recon_in_view v;
    v.keys = base; v.disc = RC_COL(uint32_t, base, disc);
    v.mag = RC_COL(float, base, mag); v.key_bits = RC_COL(int, base, mag + N); v.n_punct = RC_COL(int, base, mag + 2 * N);
    v.crc = RC_COL(uint32_t, base, mag + 3 * N);
    v.words = mag + 4 * N;
    return v;
}

typedef struct recon_bob_view {
    uint32_t *keys;
    int *status, *flips, *iters, *crc;      /* rk_verify's `res` is `status`: the four columns follow each other */
    size_t words;
} recon_bob_view;
RC_FN recon_bob_view recon_bob_layout(uint32_t *base, int n, int Wk)
{
    const size_t N = (size_t)n, res = N * (size_t)Wk;
    recon_bob_view v;
    v.keys = base;
    v.status = RC_COL(int, base, res); v.flips = RC_COL(int, base, res + N); v.iters = RC_COL(int, base, res + 2 * N); v.crc = RC_COL(int, base, res + 3 * N);
    v.words = res + 4 * N;
    return v;
}

typedef struct recon_alice_view {
    uint32_t *disc, *crc;
    size_t words;
} recon_alice_view;
RC_FN recon_alice_view recon_alice_layout(uint32_t *base, int n, int Wm)
{
    const size_t N = (size_t)n, crc = N * (size_t)Wm;
    recon_alice_view v;
    v.disc = base; v.crc = RC_COL(uint32_t, base, crc);
    v.words = crc + N;
    return v;
}

#endif /* QLDPC_RECON_CORE_H */
