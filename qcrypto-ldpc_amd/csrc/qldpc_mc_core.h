/*
 * qldpc_mc_core.h -- the frame definition, the quantised-channel definition, the puncture-pattern definition and the fixed-weight frame
 * definition of the Monte-Carlo loop (qldpc_mc_*), plain C, shared by the kernels (qldpc_mc.hip) and by their host mirror (qldpc_mc_host.c), so
 * that the CPU suite runs what the lanes run.
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
 * Quantised soft-output channels (qldpc_mc_set_channel, mc_soft_channel).  A binary-input channel with Q <= 256 output levels is given by
 * thresholds: VN v of frame i draws u = output word v % 4 at counter (v / 4, 3, i_lo, i_hi) and its level is the number of thresholds of the
 * sent bit's row that u has passed,
 *
 *   level = #{k : u >= cum[b][k]},   so that   P(level | b) = (cum[b][level] - cum[b][level - 1]) / 2^32   exactly
 *
 * (cum[b][-1] = 0, cum[b][Q-1] = 2^32); the decoder is handed value[level].  The rows are non-decreasing with entries in [0, 2^32]; the
 * entries equal to 2^32 -- levels that nothing reaches -- sit at the end of a row, so a row is kept as its 32-bit thresholds below 2^32
 * and their number (live).  Repeated thresholds give levels of probability zero.  Per class:
 *
 *   QLDPC_VN_CHANNEL    LLR = value[level]
 *   QLDPC_VN_PINNED     LLR = +-QLDPC_CONFIRMED_BIT_LLR by the sent bit, the sign inverted iff the same u < floor(parity_ber 2^32)
 *   QLDPC_VN_PUNCTURED  LLR = 0
 *
 * and the VN's flip bit (the rx row, hence channel_flips) is set iff the sign of the LLR contradicts the sent bit: b = 0 and LLR < 0, or
 * b = 1 and LLR > 0.  An LLR of 0 is no flip.  Stream 3 is this channel's own: the frames of the BSC (stream 1) do not move.
 */
#define MC_STREAM_SOFT 3u
#define MC_SOFT_MAX_LEVELS 256
#define MC_CONFIRMED_LLR 23.025850929840455f       /* QLDPC_CONFIRMED_BIT_LLR of include/qldpc.h */

typedef struct mc_soft_table {
    uint32_t levels, live[2];                      /* Q; the thresholds below 2^32 per row, at most Q - 1 */
    uint32_t thr[2][MC_SOFT_MAX_LEVELS - 1];
    float value[MC_SOFT_MAX_LEVELS];
} mc_soft_table;

/* #{k < live : u >= thr[k]} of an ascending row, live <= 255: eight halving steps, no data-dependent branch */
MC_FN uint32_t mc_soft_level(const uint32_t *thr, uint32_t live, uint32_t u)
{
    uint32_t lo = 0;      /* thr[0 .. lo-1] <= u */
    for (uint32_t step = MC_SOFT_MAX_LEVELS / 2; step; step >>= 1) {
        const uint32_t m = lo + step;
        if (m <= live && thr[m - 1] <= u) lo = m;
    }
    return lo;
}

/* VNs 4 g .. 4 g + 3 of frame `frame`: cls4 = their classes, one per byte, lowest byte first; bits = their sent bits, VN 4 g + b at bit 3 - b
 * (the MSB-first nibble of the codeword word); thr0 / thr1 / value = the table (LDS in the kernel).  Writes the four LLRs and returns the
 * four flip bits in the layout of `bits`.  One Philox call, none where all four are punctured (the padding past N is). */
MC_FN uint32_t mc_soft_quad(uint64_t seed, uint64_t frame, uint32_t g, uint32_t cls4, uint32_t bits, const uint32_t *thr0, uint32_t live0,
                            const uint32_t *thr1, uint32_t live1, const float *value, uint32_t t_pinned, float llr[4])
{
    uint32_t o[4] = {0u, 0u, 0u, 0u}, flips = 0;
    if (cls4 != 0x02020202u)
        mc_philox(g, MC_STREAM_SOFT, (uint32_t)frame, (uint32_t)(frame >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), o);
    for (uint32_t b = 0; b < 4; b++) {
        const uint32_t c = (cls4 >> (8u * b)) & 0xffu, sent = (bits >> (3u - b)) & 1u;
        float l = 0.0f;
        if (c == 0u) l = value[sent ? mc_soft_level(thr1, live1, o[b]) : mc_soft_level(thr0, live0, o[b])];
        else if (c == 1u) l = (sent != 0u) != (o[b] < t_pinned) ? -MC_CONFIRMED_LLR : MC_CONFIRMED_LLR;
        llr[b] = l;
        if (sent ? l > 0.0f : l < 0.0f) flips |= 8u >> b;
    }
    return flips;
}

/* (levels, cum0[levels - 1], cum1[levels - 1], value[levels]) -> the table.  Returns 0, -1 for levels outside 2 .. 256, -2 for a missing
 * array, a decreasing row or an entry above 2^32; the table is written only on 0 */
static inline int mc_soft_table_build(int levels, const uint64_t *cum0, const uint64_t *cum1, const float *value, mc_soft_table *t)
{
    if (levels < 2 || levels > MC_SOFT_MAX_LEVELS) return -1;
    if (!cum0 || !cum1 || !value) return -2;
    const uint64_t *cum[2] = {cum0, cum1};
    for (int b = 0; b < 2; b++)
        for (int k = 0; k < levels - 1; k++)
            if (cum[b][k] > 4294967296ull || (k > 0 && cum[b][k] < cum[b][k - 1])) return -2;
    t->levels = (uint32_t)levels;
    for (int b = 0; b < 2; b++) {
        t->live[b] = 0;
        for (int k = 0; k < MC_SOFT_MAX_LEVELS - 1; k++) {
            const int live = k < levels - 1 && cum[b][k] < 4294967296ull;
            t->thr[b][k] = live ? (uint32_t)cum[b][k] : 0xFFFFFFFFu;
            t->live[b] += (uint32_t)live;
        }
    }
    for (int l = 0; l < MC_SOFT_MAX_LEVELS; l++) t->value[l] = l < levels ? value[l] : 0.0f;
    return 0;
}

/*
 * Puncture patterns (qldpc_mc_patterns_dev, qldpc_mc_search).  Pattern p (a 64-bit global index) over an ascending candidate list
 * cand[0 .. n_cand-1] is a pure function of (seed, p, n_cand, n_punct, key_bits):
 *
 *   key        u_c = output word c % 4 at counter (c / 4, 2, p_lo, p_hi), key = (seed low word, seed high word); u'_c = u_c >> (32 - key_bits)
 *   selection  the n_punct candidates smallest in the lexicographic order (u'_c, c): equal keys go to the lower candidate index
 *
 * key_bits is 32 in production (0 stands for 32): a uniformly random subset up to 32-bit key collisions broken by index.  Smaller values
 * exist for TESTS only, which force equal keys with them and so reach the tie rule.
 *
 * The selection is a radix select, not a sort: the digits of u' from the top, MC_SEL_BITS at a time; per digit a histogram of the candidates
 * whose higher digits equal the prefix found so far, and mc_select_digit picks the bucket that holds rank k.  What remains is the threshold
 * key T and the number r of candidates with u' == T to take, the first r in index order.  Kernel and host mirror share every function here.
 */
#define MC_STREAM_PATTERN 2u
#define MC_SEL_BITS 8
#define MC_SEL_BINS (1 << MC_SEL_BITS)

MC_FN int mc_key_bits(int key_bits) { return key_bits == 0 ? 32 : key_bits; }

/* the coarsened keys of candidates 4 q .. 4 q + 3 of pattern p; key_bits in 1 .. 32 */
MC_FN void mc_pattern_keys(uint64_t seed, uint64_t p, uint32_t q, int key_bits, uint32_t u[4])
{
    mc_philox(q, MC_STREAM_PATTERN, (uint32_t)p, (uint32_t)(p >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), u);
    for (int b = 0; b < 4; b++) u[b] >>= 32 - key_bits;
}

/* the shift of the top digit that can be non-zero */
MC_FN int mc_select_top_shift(int key_bits) { return MC_SEL_BITS * ((key_bits + MC_SEL_BITS - 1) / MC_SEL_BITS - 1); }

/* hist = the digit histogram of the candidates still in play, *k (1-based, at most their number) the rank looked for among them: returns the
 * digit whose bucket holds it and leaves in *k the rank inside that bucket */
MC_FN uint32_t mc_select_digit(const uint32_t *hist, uint32_t *k)
{
    uint32_t d = 0;
    while (d < MC_SEL_BINS - 1 && hist[d] < *k) { *k -= hist[d]; d++; }
    return d;
}

/* does the final pass take candidate c with key u?  below counts the candidates before c with u' == T */
MC_FN int mc_pattern_takes(uint32_t u, uint32_t T, uint32_t r, uint32_t equal_before) { return u < T || (u == T && equal_before < r); }

/* a list of VNs (candidates, a puncture set): ascending, distinct, inside [0, N).  Returns -1, or the index of the first offending entry */
static inline int mc_vn_list_check(const int *vn, int n, int N)
{
    for (int i = 0; i < n; i++)
        if (vn[i] < 0 || vn[i] >= N || (i > 0 && vn[i] <= vn[i - 1])) return i;
    return -1;
}

/* the packed MSB-first row (ceil(N / 32) words) of a checked list */
static inline void mc_vn_list_row(const int *vn, int n, int N, uint32_t *row)
{
    for (int w = 0; w < (N + 31) / 32; w++) row[w] = 0;
    for (int i = 0; i < n; i++) row[vn[i] >> 5] |= 0x80000000u >> (vn[i] & 31);
}

/*
 * Fixed-weight error strata (qldpc_mc_weight_frames_*, qldpc_mc_strata).  Conditioned on the number of flipped channel bits a BSC's flip set
 * is uniform over the subsets of that size, so the fixed-weight frame (i, w) is defined on the words the BSC already draws:
 *
 *   key        u_v = output word v % 4 at counter (v / 4, 1, i_lo, i_hi) -- the word mc_flip_word compares with its threshold;
 *              u'_v = u_v >> (32 - key_bits), key_bits 1 .. 32 (0 stands for 32; below 32 for TESTS only, which force ties with it)
 *   flip set   the w VNs of class QLDPC_VN_CHANNEL smallest in the order (u'_v, v): equal keys go to the lower VN; 0 <= w <= channel VNs
 *   others     QLDPC_VN_PINNED flips iff u_v < floor(parity_ber 2^32), as in the BSC frame; QLDPC_VN_PUNCTURED never
 *
 * At key_bits = 32 the BSC set {v channel : u_v < T} is, for every T, the fixed-weight set of its own size, and the sets of two weights of one
 * frame are nested.  The select is the radix select of the puncture patterns (mc_select_top_shift, mc_select_digit, mc_pattern_takes) over
 * keys recomputed per pass; it ends with the threshold key T and the number r of channel VNs with u' == T to take, the first r in VN order
 * (weight 0: T = 0, r = 0, no pass).  The final pass works on whole codeword words: three masks per word, then the first bits of `eq`.
 */

/* VNs 4 g .. 4 g + 3 of frame `frame`: cls4 = their classes, one per byte, lowest byte first.  Returns bit b = VN 4 g + b is QLDPC_VN_CHANNEL,
 * bit 4 + b = it is QLDPC_VN_PINNED, and in u their stream-1 words; no Philox call (u = 0) where no VN is a channel VN and none a pinned VN
 * that can flip (t_pinned = 0: the digit passes need the channel VNs only) */
MC_FN uint32_t mc_weight_quad(uint64_t seed, uint64_t frame, uint32_t g, uint32_t cls4, uint32_t t_pinned, uint32_t u[4])
{
    uint32_t chan = 0, pinned = 0;
    for (uint32_t b = 0; b < 4; b++) {
        const uint32_t c = (cls4 >> (8u * b)) & 0xffu;
        chan |= (uint32_t)(c == 0u) << b;
        pinned |= (uint32_t)(c == 1u) << b;
    }
    if (chan | (t_pinned ? pinned : 0u))
        mc_philox(g, MC_STREAM_CHANNEL, (uint32_t)frame, (uint32_t)(frame >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), u);
    else u[0] = u[1] = u[2] = u[3] = 0u;
    return chan | pinned << 4;
}

/* codeword word w (VNs 32 w .. 32 w + 31, MSB-first) of frame `frame` against the threshold key T: less = the channel VNs with u' < T, eq = those
 * with u' == T, pin = the pinned VNs that flip.  cls4 as mc_flip_word takes it; key_bits in 1 .. 32.  8 Philox calls at the most. */
MC_FN void mc_weight_masks(uint64_t seed, uint64_t frame, uint32_t w, const uint32_t cls4[8], int key_bits, uint32_t T, uint32_t t_pinned,
                           uint32_t *less, uint32_t *eq, uint32_t *pin)
{
    uint32_t l = 0, e = 0, p = 0, u[4];
    for (uint32_t g = 0; g < 8; g++) {
        const uint32_t m = mc_weight_quad(seed, frame, 8u * w + g, cls4[g], t_pinned, u);
        for (uint32_t b = 0; b < 4; b++) {
            const uint32_t bit = 0x80000000u >> (4u * g + b), k = u[b] >> (32 - key_bits);
            if ((m >> b) & 1u) { if (k < T) l |= bit; else if (k == T) e |= bit; }
            else if (((m >> (4u + b)) & 1u) && u[b] < t_pinned) p |= bit;
        }
    }
    *less = l; *eq = e; *pin = p;
}

/* the selected VNs of a word: all of `less`, and of `eq` in VN order (from the MSB) those that mc_pattern_takes takes, given that equal_before
 * channel VNs with u' == T precede the word and r of them are taken in all */
MC_FN uint32_t mc_weight_take(uint32_t less, uint32_t eq, uint32_t T, uint32_t r, uint32_t equal_before)
{
    uint32_t sel = less;
    for (; eq && mc_pattern_takes(T, T, r, equal_before); equal_before++) {
        const uint32_t top = 0x80000000u >> __builtin_clz(eq);
        sel |= top; eq ^= top;
    }
    return sel;
}

/*
 * The QBER sweep (qldpc_mc_sweep): the deal of one round, a pure function of its arguments.  Point q is open iff done[q] < max_frames and
 * (max_fe == 0 or fe[q] < max_fe) and then needs ceil((max_frames - done[q]) / C) chunks.  The deal cycles over the open points in ascending
 * q and on each visit gives one chunk to a point that has fewer than it needs; it stops when the S slots are used or a whole cycle has given
 * nothing.  Returns the chunks dealt; give[P] is written in full.  C >= 1.
 */
#define MC_SWEEP_MAX_POINTS 4096                   /* QLDPC_MC_SWEEP_MAX_POINTS of include/qldpc.h */

static inline int mc_sweep_open(uint64_t done, uint64_t fe, uint64_t max_frames, uint64_t max_fe) { return done < max_frames && (max_fe == 0 || fe < max_fe); }

static inline int mc_sweep_deal(int P, int C, int S, uint64_t max_frames, uint64_t max_fe, const uint64_t *done, const uint64_t *fe, int *give)
{
    int used = 0, gave = 1;
    for (int q = 0; q < P; q++) give[q] = 0;
    while (used < S && gave) {
        gave = 0;
        for (int q = 0; q < P && used < S; q++) {
            if (!mc_sweep_open(done[q], fe[q], max_frames, max_fe)) continue;
            const uint64_t left = max_frames - done[q], need = left / (uint64_t)C + (left % (uint64_t)C != 0);      /* no left + C - 1: it may wrap */
            if ((uint64_t)give[q] < need) { give[q]++; used++; gave = 1; }
        }
    }
    return used;
}

/* the puncture order of a sweep: distinct VNs inside [0, N), in any order.  seen[N] comes in zeroed.  Returns -1, or the index of the first
 * offending entry */
static inline int mc_punct_order_check(const int *order, int n, int N, uint8_t *seen)
{
    for (int i = 0; i < n; i++) {
        if (order[i] < 0 || order[i] >= N || seen[order[i]]) return i;
        seen[order[i]] = 1;
    }
    return -1;
}

/*
 * Blind reconciliation rounds (qldpc_mc_blind): the schedule, a pure function of the pool counts.  A frame that is still open after round r - 1
 * waits in pool r (1 <= r <= R = max_rounds) as {frame index, known row}; a launch decodes n <= batch frames of ONE level: level 0 = fresh frames,
 * level r = the last n entries of pool r.  A launch at level r < R appends its open frames to pool r + 1.  In order:
 *
 *   1. the DEEPEST level with pool >= batch, `batch` of it
 *   2. else, while input is left, level 0 with min(batch, input_left)
 *   3. else the LOWEST non-empty level, all of it (the flush: ragged, and what it opens lands in a deeper pool that is flushed after it)
 *
 * Why no pool reaches 2 batch: pool r + 1 grows only by a launch at level r, of at most batch frames, and rules 1 - 3 pick level r only when no
 * deeper level holds batch or more (rule 1 would have taken the deepest such level; rules 2 and 3 apply when there is none at all).  So pool r + 1
 * holds at most batch - 1 before that launch and at most 2 batch - 1 after it, which is the capacity MC_BLIND_POOL_CAP.  Every launch either
 * consumes input or moves frames strictly deeper or out, so the loop ends, with every pool empty.  pool[0] is not read.
 */
#define MC_BLIND_MAX_ROUNDS 64                     /* QLDPC_MC_BLIND_MAX_ROUNDS of include/qldpc.h */
#define MC_BLIND_POOL_CAP(batch) (2 * (size_t)(batch) - 1)

/* returns 0 when nothing is left, else 1 with the level and the frames of the next launch */
static inline int mc_blind_next(int R, int batch, const uint64_t *pool, uint64_t input_left, int *level, int *n)
{
    for (int r = R; r >= 1; r--)
        if (pool[r] >= (uint64_t)batch) { *level = r; *n = batch; return 1; }
    if (input_left) { *level = 0; *n = input_left < (uint64_t)batch ? (int)input_left : batch; return 1; }
    for (int r = 1; r <= R; r++)
        if (pool[r]) { *level = r; *n = (int)pool[r]; return 1; }
    return 0;
}

/*
 * The schedule of qldpc_mc_guess, a pure function of the pool count.  Failed first decodes wait in ONE pool as {frame index, guess row, hard row, first verdict}; a
 * trial launch takes the last S = floor(batch / T) entries and decodes their S T trial frames.  In order:
 *
 *   1. a trial launch of S sources while pool >= S
 *   2. else a fresh launch of min(batch, input_left) frames
 *   3. else the flush: a trial launch of all remaining sources
 *
 * Why the pool stays below S + batch: only a fresh launch appends, at most batch entries, and rule 2 applies only while pool < S, i.e. pool <= S - 1
 * before it and <= S - 1 + batch after it.  Trial launches only take entries away.  Every launch either consumes input or removes at least one
 * entry (S >= 1 because T <= batch), so the loop ends with the pool empty.  With g = 0 nothing is ever pooled (the caller appends nothing).
 */
#define MC_GUESS_MAX_BITS 10                      /* QLDPC_GUESS_MAX_BITS of include/qldpc.h */
enum { MC_GUESS_FRESH = 1, MC_GUESS_TRIALS = 2 };   /* QLDPC_MC_GUESS_FRESH, QLDPC_MC_GUESS_TRIALS */
/* the capacity for every g >= 1 (S <= batch / 2); g = 0 pools nothing */
#define MC_GUESS_POOL_CAP(batch) ((size_t)(batch) / 2 + (size_t)(batch))

/* returns 0 when nothing is left, else 1 with the kind and n = the frames of a fresh launch or the SOURCES of a trial launch */
static inline int mc_guess_next(int g, int batch, uint64_t pool, uint64_t input_left, int *kind, int *n)
{
    const uint64_t S = (uint64_t)batch >> g;
    if (pool >= S && pool) { *kind = MC_GUESS_TRIALS; *n = (int)S; return 1; }
    if (input_left) { *kind = MC_GUESS_FRESH; *n = input_left < (uint64_t)batch ? (int)input_left : batch; return 1; }
    if (pool) { *kind = MC_GUESS_TRIALS; *n = (int)pool; return 1; }
    return 0;
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
