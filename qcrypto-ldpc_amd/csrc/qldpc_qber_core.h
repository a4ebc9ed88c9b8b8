/*
 * qldpc_qber_core.h -- the definition of "the QBER a frame's parity message shows" (qldpc_qber_estimate_dev, qldpc_recon_estimate_blocks), plain C,
 * shared by the kernels (qldpc_kernels_qber.h) and by their host mirrors (qldpc_qber_host.c), so that the CPU suite runs what the lanes run.
 *
 *   state    of VN v of frame f, what the loads mean (qldpc_load_bits_short_dev, _load_erasures_dev, _load_known_dev):
 *              known-exact  its known bit is set (value = its value bit; known wins over erased), or class QLDPC_VN_PINNED, or class
 *                           QLDPC_VN_CHANNEL with v >= n_channel[f] (shortened); value = its bit of the frame row unless known
 *              erased       class QLDPC_VN_PUNCTURED (any class but channel / pinned, as the loads read it) or its erase bit set, and not known
 *              noisy        the rest: class channel, v < n_channel[f], not known, not erased
 *   check c  is informative iff none of its VNs is erased; its effective degree d = the number of its noisy VNs, its outcome
 *            u = s_c ^ XOR of the values of all its VNs (s_c = 0 without a syndrome row)
 *   counts   [d][0] = informative checks of effective degree d, [d][1] = those of them with u = 1, d = 0 .. D = the code's largest check degree
 *   score    S_k = SUM_{d >= 1} u_d L1[d][k] + (n_d - u_d) L0[d][k] in int64, L1 / L0 = llround(log p_d(q_k) 2^24) / llround(log(1 - p_d(q_k)) 2^24),
 *            p_d(q) = (1 - (1 - 2 q)^d) / 2, q_k = q_lo (q_hi / q_lo)^(k / (n_grid - 1)); tables [D + 1][n_grid], row 0 zero
 *   estimate the smallest k with maximal S_k over a full scan; -1 when no informative check has d >= 1
 *
 * MERGING (opt-in, qldpc_qber_set_merge; off = everything above and nothing else), for a code whose parity part is an accumulator chain: K = N - M, VN K + c
 * lies on exactly checks c and c + 1 for c < M - 1, VN K + M - 1 on check M - 1 only, no other VN >= K in any row (qldpc_qber_repeat_table_host verifies it edge by
 * edge).  The checks on the two sides of an erased chain VN add up to one parity equation without it:
 *   link     VN K + c, c < M - 1, of frame f is a link iff its state in that frame is erased (by class or by erase bit; known wins, so a known one is exact)
 *   run      a maximal set of consecutive checks h .. t joined by links; check c is a head iff c = 0 or VN K + c - 1 is no link (qb_run_checks)
 *   one check   counted exactly as above
 *   two or more one observation: u = XOR over the run's checks of s_c and of the values of all their VNs but the links (each occurs twice and cancels),
 *            d = the number of noisy VNs with an odd number of edges into the run -- a VN shared by two checks of the run cancels in u and does not
 *            count in d (qb_earlier_in_run over the repeat table; the graph layer admits no VN twice in one row)
 *   left out a run with an erased VN other than its own links (an erased VN K + M - 1 included; an erased VN that occurs twice is not cancelled), with
 *            more than QB_MAX_RUN checks, or with d > QB_MAX_DEGREE
 *   counts   [QB_MAX_DEGREE + 1][2] whatever D; tables to degree QB_MAX_DEGREE; score, argmax and pool as above
 *
 * The state is resolved 32 VNs at a time on the packed rows (qb_collapse_word); the class map enters as two packed rows (pinned, punctured) that
 * are built once per call (qb_class_word).  Integer scores make host and device agree exactly whatever the order of summation.
 */
#ifndef QLDPC_QBER_CORE_H
#define QLDPC_QBER_CORE_H

#include <stdint.h>

#if defined(__HIPCC__)
#define QB_FN __host__ __device__ static inline
#else
#define QB_FN static inline
#endif

#define QB_MAX_DEGREE 63          /* D above this: QLDPC_EUNSUPPORTED */
#define QB_MAX_RUN 16             /* merging: a run of more checks is left out (bounds a thread's walk) */
#define QB_MAX_GRID 1024
#define QB_SCALE 16777216.0       /* 2^24 table units per nat */
#define QB_MIN_Q_LO 1e-6          /* |log p_1(q_lo)| 2^24 < 2^28, so that a score over fewer than 2^35 checks fits int64 */

/* bit v of a packed row, MSB-first (helpers.h:65-70) */
QB_FN uint32_t qb_bit(const uint32_t *row, int v) { return (row[v >> 5] >> (31 - (v & 31))) & 1u; }
/* the bits of word w that stand for VNs below n (n <= 0: none) */
QB_FN uint32_t qb_below_word(int w, int n)
{
    const long long left = (long long)n - (long long)w * 32;
    return left >= 32 ? 0xffffffffu : (left <= 0 ? 0u : 0xffffffffu << (32 - (int)left));
}
/* packed class rows of word w of a class map (NULL = all channel): *pinned / *punct have a bit set for the VNs of class QLDPC_VN_PINNED / of any class
 * that is neither channel nor pinned (the loads give those LLR 0) */
QB_FN void qb_class_word(const uint8_t *vn_class, int w, int N, uint32_t *pinned, uint32_t *punct)
{
    uint32_t pi = 0, pu = 0;
    for (int b = 0; vn_class && b < 32 && w * 32 + b < N; b++) {
        const int cls = vn_class[w * 32 + b];
        if (cls == 1) pi |= 0x80000000u >> b;
        else if (cls != 0) pu |= 0x80000000u >> b;
    }
    *pinned = pi; *punct = pu;
}
/* the three rows the checks gather from, for the 32 VNs of one word: their values, which are noisy, which are erased.  bits / erase / known / value =
 * the frame's words (0 where the row is absent), pinned / punct = the class words, below = qb_below_word(w, n_channel[f]) */
QB_FN void qb_collapse_word(uint32_t bits, uint32_t erase, uint32_t known, uint32_t value, uint32_t pinned, uint32_t punct, uint32_t below,
                            uint32_t *val, uint32_t *noisy, uint32_t *erased)
{
    *val = (bits & ~known) | (value & known);
    *erased = (punct | erase) & ~known;
    *noisy = ~pinned & ~punct & below & ~erase & ~known;
}
/* merging: the number of checks of the run that starts at head h, QB_MAX_RUN + 1 for any longer one.  e0 / e1 = the erased words that hold VN K + h and
 * the 32 VNs after that word (0 past the row): the at most QB_MAX_RUN link bits looked at lie in them */
QB_FN int qb_run_checks(uint32_t e0, uint32_t e1, int K, int h, int M)
{
    const uint64_t win = (((uint64_t)e0 << 32) | (uint64_t)e1) << ((K + h) & 31);
    int n = 0;
    while (n < QB_MAX_RUN && h + n < M - 1 && ((win >> (63 - n)) & 1u)) n++;
    return n + 1;
}
/* merging: is VN v one of the links K + h .. K + t - 1 of the run h .. t? */
QB_FN int qb_is_link(int v, int K, int h, int t) { return v >= K + h && v < K + t; }
/* merging: how many checks h .. c - 1 of the run hold VN v = tab[j][c], r = rep[j][c].  tab[D][M] = the transposed check table (-1 past a check's
 * degree), rep[D][M] = for every edge the distance back to the nearest earlier check within QB_MAX_RUN - 1 that holds the same VN, or 0 */
QB_FN int qb_earlier_in_run(const int *tab, const uint8_t *rep, int M, int D, int r, int c, int v, int h)
{
    int n = 0;
    while (r && c - r >= h) {
        n++; c -= r;
        int j = 0;
        while (j < D - 1 && tab[(size_t)j * M + c] != v) j++;      /* the rare third occurrence: v's slot in that row */
        r = rep[(size_t)j * M + c];
    }
    return n;
}
/* S_k of counts cnt[D + 1][2] (uint64: a frame's counts widened, or the pool) */
QB_FN int64_t qb_score(const uint64_t *cnt, int D, const int32_t *L1, const int32_t *L0, int n_grid, int k)
{
    int64_t S = 0;
    for (int d = 1; d <= D; d++) {
        const uint64_t n = cnt[2 * d], u = cnt[2 * d + 1];
        if (!n) continue;
        S += (int64_t)u * (int64_t)L1[(size_t)d * n_grid + k] + (int64_t)(n - u) * (int64_t)L0[(size_t)d * n_grid + k];
    }
    return S;
}
/* does (S, k) beat the best so far?  best_k < 0 = nothing yet; ties go to the lower k */
QB_FN int qb_better(int64_t S, int k, int64_t best_S, int best_k) { return best_k < 0 || S > best_S || (S == best_S && k < best_k); }
/* informative checks of degree >= 1 in cnt[D + 1][2] */
QB_FN uint64_t qb_observations(const uint64_t *cnt, int D)
{
    uint64_t n = 0;
    for (int d = 1; d <= D; d++) n += cnt[2 * d];
    return n;
}

#endif /* QLDPC_QBER_CORE_H */
