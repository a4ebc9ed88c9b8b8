/*
 * qldpc_polyhash_core.h -- the universal hash of error verification (qldpc_polyhash_*), plain C, shared by the kernels (qldpc_polyhash.hip)
 * and by their host mirror (qldpc_polyhash_host.c), so that the CPU suite runs what the lanes run.
 *
 * Polynomial evaluation over the Mersenne prime p = 2^61 - 1.  A block of n >= 1 bits in W = ceil(n / 32) words (MSB-first, the bits past n
 * ignored) has the W + 1 coefficients c_0 .. c_(W-1) = its words, the tail masked, and c_W = n, and under the key k
 *
 *     tag = SUM_{j <= W} c_j k^(W+1-j) mod p          (Horner: h = 0; for every c: h = (h + c) k)
 *
 * The length is a coefficient, so zero padding cannot collide; two different (n, message) pairs differ in a non-zero polynomial of degree
 * <= W + 1 without constant term, so they collide for at most W + 1 non-zero keys and for k = 0.  A key is 64 caller's bits taken & p with p -> 0:
 * field value 0 has probability 2^-60, every other 2^-61, which gives (W + 2) 2^-61 per key.
 *
 * Residues are canonical, in [0, p), at every function boundary.  Corrections are selects.
 *
 * THE DECOMPOSITION.  With m coefficients d_0 .. d_(m-1) and x the evaluation point, E = SUM_j d_j x^(m-1-j) (so tag = k E over all
 * W + 1 coefficients) is computed by T virtual lanes: the sequence is shifted by a places (a zeros in front change nothing), lane u takes
 * the positions u, u + T, u + 2T, ... that exist, as Horner in X = x^T (h = h X + d), and E = SUM_u h_u x^((r - 1 - u) mod T) with
 * r = (m + a) mod T.  The kernel uses this twice.  A workgroup of L lanes hashes one tile of at most tile_words coefficients with
 * T = 4 L (a lane owns the four words of one 16-byte load, one accumulator each), a the words between the last 16-byte boundary and the
 * tile's first word.  A block of several tiles leaves one partial P_tau per tile, and
 *
 *     E = (SUM_{tau < tiles-1} P_tau Y^(tiles-2-tau)) k^(len of the last tile) + P_(tiles-1),      Y = k^tile_words
 *
 * where the sum is the same evaluation with T = L, a = 0 and x = Y.  Rows of a tile that hold nothing but whole key words ("fast" rows) take
 * their words as they are (the a words in front of row 0 as 0); the rows that reach the masked last word, the length or the tile's end are
 * checked word by word, and a lane loads there only where its 16 bytes hold a word of the tile.
 */
#ifndef QLDPC_POLYHASH_CORE_H
#define QLDPC_POLYHASH_CORE_H

#include <stdint.h>

#include "qldpc_hashbatch_core.h"

#define PH_P 0x1FFFFFFFFFFFFFFFull /* 2^61 - 1 */
#define PH_MAX_KEYS 4
#define PH_LANE_WORDS 4u           /* key words per lane and load */
#define PH_TILE_WORDS QLDPC_POLYHASH_TILE_WORDS
#define PH_TILE_WORDS_SMALL QLDPC_POLYHASH_TILE_WORDS_SMALL

/* any 64-bit sum of residues -> canonical: 2^61 = 1, so the top three bits fold onto the low 61 (<= p + 7 < 2p) */
HB_FN uint64_t ph_fold(uint64_t s)
{
    const uint64_t f = (s & PH_P) + (s >> 61);
    return f - (f >= PH_P ? PH_P : 0ull);
}

HB_FN uint64_t ph_add(uint64_t a, uint64_t b)
{
    const uint64_t s = a + b;                                    /* < 2p */
    return s - (s >= PH_P ? PH_P : 0ull);
}

/* the caller's 64 bits as a field element: & p, and p itself is 0 */
HB_FN uint64_t ph_key(uint32_t hi, uint32_t lo)
{
    const uint64_t k = (((uint64_t)hi << 32) | lo) & PH_P;
    return k == PH_P ? 0ull : k;
}

/*
 * a b + c mod p for canonical a, b, c.  With a = a1 2^32 + a0, b = b1 2^32 + b0 (a1, b1 < 2^29) the 122-bit value a b + c is built from
 * four 32 x 32 -> 64-bit multiply-adds, each with room for its carry-in, c = c1 2^32 + c0 going in by halves (a key word has c1 = 0):
 *     t0 = a0 b0 + c0                     <= (2^32 - 1)^2 + 2^32 - 1 < 2^64
 *     t1 = a0 b1 + (t0 >> 32) + c1        < 2^61 + 2^32 + 2^29
 *     t2 = a1 b0 + (t1 mod 2^32)          < 2^61 + 2^32
 *     hi = a1 b1 + (t1 >> 32) + (t2 >> 32)      < 2^58 + 2^31,         lo = (t2 mod 2^32) 2^32 + (t0 mod 2^32)
 * so a b + c = hi 2^64 + lo, and 2^61 = 1 folds it without a wide division: 8 hi + (lo >> 61) + (lo & p) < 2^62, which ph_fold finishes.
 */
HB_FN uint64_t ph_mul_add(uint64_t a, uint64_t b, uint64_t c)
{
    const uint32_t a0 = (uint32_t)a, a1 = (uint32_t)(a >> 32), b0 = (uint32_t)b, b1 = (uint32_t)(b >> 32);
    const uint64_t t0 = (uint64_t)a0 * b0 + (uint32_t)c;
    const uint64_t t1 = (uint64_t)a0 * b1 + (t0 >> 32) + (c >> 32);
    const uint64_t t2 = (uint64_t)a1 * b0 + (uint32_t)t1;
    const uint64_t hi = (uint64_t)a1 * b1 + (t1 >> 32) + (t2 >> 32), lo = (t2 << 32) | (uint32_t)t0;
    return ph_fold(((hi << 3) | (lo >> 61)) + (lo & PH_P));
}

HB_FN uint64_t ph_mul(uint64_t a, uint64_t b) { return ph_mul_add(a, b, 0ull); }

HB_FN uint64_t ph_pow(uint64_t a, uint32_t e)
{
    uint64_t r = 1ull;
    for (; e; e >>= 1, a = ph_mul(a, a))
        if (e & 1u) r = ph_mul(r, a);
    return r;
}

/* the tag as its two words: hi (29 bits), then lo */
HB_FN void ph_store_tag(uint32_t *out, uint64_t tag) { out[0] = (uint32_t)(tag >> 32); out[1] = (uint32_t)tag; }

/* ---- the decomposition, as pure functions of (lane count, tile) ---- */

HB_FN uint32_t ph_coefs(int key_bits) { return hb_words(key_bits) + 1u; }
HB_FN uint32_t ph_tiles(uint32_t coefs, uint32_t tile) { return (coefs + tile - 1u) / tile; }
/* coefficients of tile tau < ph_tiles: only the last one is ragged */
HB_FN uint32_t ph_tile_len(uint32_t coefs, uint32_t tile, uint32_t tau) { return coefs - tau * tile < tile ? coefs - tau * tile : tile; }
/* those at the front of a tile that starts at coefficient `base` which are whole key words: the ones before word W - 1 */
HB_FN uint32_t ph_tile_plain(uint32_t key_words, uint32_t base, uint32_t len)
{
    const uint32_t left = key_words - 1u > base ? key_words - 1u - base : 0u;
    return left < len ? left : len;
}
/* 0 = the production tile; anything but the two instances is refused */
HB_FN uint32_t ph_tile_words(int tile_words)
{
    return tile_words == 0 || tile_words == PH_TILE_WORDS ? (uint32_t)PH_TILE_WORDS : tile_words == PH_TILE_WORDS_SMALL ? (uint32_t)PH_TILE_WORDS_SMALL : 0u;
}
/* words between the last 16-byte boundary and p */
HB_FN uint32_t ph_shift(const uint32_t *p) { return (uint32_t)(((uintptr_t)p >> 2) & (PH_LANE_WORDS - 1u)); }

/* m coefficients of which the first `plain` are whole words, shifted by a < 4 <= T, over T virtual lanes: the rows [0, fast) hold nothing
   but whole key words (and, in front of row 0, the a words before the tile, which are read as 0); the rows from `fast` on are checked
   word by word; r gives the weights */
typedef struct ph_split { uint32_t rows, fast, r; } ph_split;

HB_FN ph_split ph_rows(uint32_t m, uint32_t plain, uint32_t a, uint32_t T)
{
    ph_split s;
    s.rows = (m + a + T - 1u) / T;
    s.r = (m + a) % T;
    s.fast = (plain + a) / T;
    return s;
}

/* the exponent of x that virtual lane u's value is weighted with */
HB_FN uint32_t ph_weight_exp(uint32_t r, uint32_t u, uint32_t T) { return (r + T - 1u - u) % T; }

/* the coefficients of a tile of m from coefficient `base` on that lie in memory: the key words, the masked one included, not the length */
HB_FN uint32_t ph_tile_avail(uint32_t key_words, uint32_t base, uint32_t m)
{
    const uint32_t left = key_words > base ? key_words - base : 0u;
    return left < m ? left : m;
}

/* whether the aligned group of PH_LANE_WORDS positions from p0 on holds a key word of the tile: only then may it be loaded (the load then
   stays inside a 16-byte line that holds a word of the row, whatever lies in the rest of it) */
HB_FN int ph_group_has_word(uint32_t p0, uint32_t a, uint32_t avail) { return avail > 0u && p0 < a + avail && p0 + PH_LANE_WORDS > a; }

/* one step of a checked row: `word` is what lies at position pos of the tile's aligned rows (anything where no key word of the tile lies);
   a position in front of the tile or past its m coefficients leaves h alone */
HB_FN uint64_t ph_checked(uint64_t h, uint64_t X, uint32_t word, uint32_t base, uint32_t pos, uint32_t a, uint32_t m,
                          uint32_t key_words, uint32_t tail_mask, uint32_t key_bits)
{
    const uint32_t j = pos - a, g = base + j;
    const uint32_t c = g + 1u < key_words ? word : g + 1u == key_words ? word & tail_mask : key_bits;
    const uint64_t next = ph_mul_add(h, X, c);
    return pos >= a && j < m ? next : h;
}

/* one doubling step of the table tab[i] = x^i, i <= n: tab[0 .. half] stand, lane t of `lanes` writes its share of tab[half + 1 .. 2 half]
   (up to n).  Start from tab[0] = 1, tab[1] = x and step half = 1, 2, 4, ... while half < n, all lanes meeting after every step */
HB_FN void ph_pow_step(uint64_t *tab, uint32_t half, uint32_t n, uint32_t t, uint32_t lanes)
{
    const uint64_t xs = tab[half];
    for (uint32_t i = t + 1u; i <= half && half + i <= n; i += lanes) tab[half + i] = ph_mul(tab[i], xs);
}

#endif /* QLDPC_POLYHASH_CORE_H */
