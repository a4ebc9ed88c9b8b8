/*
 * qldpc_recon_tag_core.h -- the keyed tag of a reconciliation session's verify step (qldpc_recon_*_tagged, qldpc_recon_tag_blocks), plain C, shared by
 * the kernels (qldpc_kernels_recon_tag.h) and by their host mirror (qldpc_recon_tag_host.c), so that the rule is stated once.
 *
 * The tag IS the one of qldpc_polyhash_core.h, whose field arithmetic this header uses and does not restate: a block of n bits in W = ceil(n / 32)
 * words (tail masked), H = SUM_{j < W} c_j k^(W-1-j) (Horner h = h k + c over the masked words), tag = k (k H + n) mod p, stored hi word then lo word;
 * r = 1 .. 4 such values per block, key after key.
 *
 * THE DECOMPOSITION is the one of the sessions' CRC (crc_chunked / rk_block_crc of qldpc_recon_core.h), not the 16-byte tiles of qldpc_polyhash.hip:
 * crc_chunk_words(W, lanes, &pad) deals c contiguous words to every lane, `pad` zero words in front of the message (they leave a zero accumulator
 * alone); a lane runs Horner in k over its chunk, and the partials fold in the CRC's binary tree, s[t] = s[t] X + s[t + s] with X = k^c squared after
 * every level.  So one pass over a decoded row feeds the CRC and the tag.  The arithmetic is exact: every power-of-two lane count gives the tag of
 * qldpc_polyhash_host.
 */
#ifndef QLDPC_RECON_TAG_CORE_H
#define QLDPC_RECON_TAG_CORE_H

#include "qldpc_polyhash_core.h"
#include "qldpc_recon_core.h"

#define RT_MAX_KEYS PH_MAX_KEYS
#define RT_MAX_BITS (1 << 18)      /* the longest block a session tags: 8192 words */
#define RT_TAG_BITS 61             /* what one key's tag discloses at the most */

/* a lane's step over one masked word of its chunk */
HB_FN uint64_t rt_step(uint64_t h, uint64_t k, uint32_t word) { return ph_mul_add(h, k, (uint64_t)word); }
/* the weight of the first fold level: k^c for chunks of c words */
HB_FN uint64_t rt_chunk_pow(uint64_t k, int c) { return ph_pow(k, (uint32_t)c); }
/* one node of the fold tree */
HB_FN uint64_t rt_fold(uint64_t left, uint64_t X, uint64_t right) { return ph_mul_add(left, X, right); }
/* the tag from the folded H of a block of n_bits */
HB_FN uint64_t rt_close(uint64_t H, uint64_t k, int n_bits) { return ph_mul(ph_mul_add(H, k, (uint64_t)(uint32_t)n_bits), k); }

/* `lanes` (a power of two) chunks folded in a tree, as a workgroup of the kernels does it; part = scratch of `lanes` values */
HB_FN uint64_t rt_tag_chunked(const uint32_t *w, int n_bits, uint64_t k, int lanes, uint64_t *part)
{
    const int nw = (n_bits + 31) / 32;
    int pad;
    const int c = crc_chunk_words(nw, lanes, &pad);
    for (int l = 0; l < lanes; l++) {
        uint64_t h = 0;
        for (int v = l * c; v < (l + 1) * c; v++) {
            const int i = v - pad;
            if (i >= 0) h = rt_step(h, k, w[i] & tail_mask(i, nw, n_bits));
        }
        part[l] = h;
    }
    uint64_t X = rt_chunk_pow(k, c);
    for (int s = 1; s < lanes; s <<= 1) {
        for (int l = 0; l + s < lanes; l += 2 * s) part[l] = rt_fold(part[l], X, part[l + s]);
        X = ph_mul(X, X);
    }
    return rt_close(part[0], k, n_bits);
}

/* key_bits as the kernels use it: nothing is read past a key row whatever the column holds */
HB_FN int rt_key_bits(int kb, int Wk) { return kb < 0 ? 0 : (kb > 32 * Wk ? 32 * Wk : kb); }

/*
 * The staging block of a launch of qldpc_recon_tag_blocks, n rows of W key words under r keys, as 32-bit words from `base`, the same in the pinned
 * block and on the device:  keys [n][W] | block length [n] | hash keys [n][2 r] (row 0 alone when shared) | tags [n][2 r].  A NULL base gives the
 * word count alone.
 */
typedef struct recon_tag_view {
    uint32_t *keys;
    int *key_bits;
    uint32_t *hash_keys, *tags;
    size_t words;
} recon_tag_view;
HB_FN recon_tag_view recon_tag_layout(uint32_t *base, int n, int W, int r)
{
    const size_t N = (size_t)n, kb = N * (size_t)W, hk = kb + N, tg = hk + N * 2 * (size_t)r;
    recon_tag_view v;
    v.keys = base; v.key_bits = RC_COL(int, base, kb); v.hash_keys = RC_COL(uint32_t, base, hk); v.tags = RC_COL(uint32_t, base, tg);
    v.words = tg + N * 2 * (size_t)r;
    return v;
}

#endif /* QLDPC_RECON_TAG_CORE_H */
