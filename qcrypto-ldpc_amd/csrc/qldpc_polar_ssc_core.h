/*
 * qldpc_polar_ssc_core.h -- the definition of the simplified successive-cancellation (SSC) decoder of Alamdar-Yazdi and Kschischang: the SC
 * decoder of qldpc_polar_core.h with the subtrees that hold only frozen leaves (rate 0) or only information leaves (rate 1) pruned.  Plain C,
 * shared by the kernel (qldpc_kernels_polar_ssc.h), by its host mirror (qldpc_polar_ssc_host.c) and by the context (qldpc_polar.hip), so that
 * the CPU suite runs what the lanes run.  Everything of qldpc_polar_core.h holds: sizes, packing, f, g, sat, the two message types, the leaf rule.
 *
 *   rule       at a node of s >= 1 leaves with beliefs L[0 .. s):
 *                every leaf frozen (rate 0)   the decisions are the frozen values, the node returns their encoding over those s bits; the beliefs
 *                                             are not looked at.  This is what SC computes anyway: exact.
 *                no leaf frozen (rate 1)      the node returns c[k] = (L[k] < 0), so 0 and -0.0 decide 0; its decisions are u = encode(c) (the
 *                                             encoder is an involution).  At s = 1 this is the leaf rule.
 *                otherwise                    the SC step: the left child with f, the right child with g over the left child's returned bits, and
 *                                             the result [c_l ^ c_r, c_r].
 *              The rule applies to nodes of every size, those inside a 32-leaf block included, so the function depends on the code alone.
 *   outputs    u, info and x, as for SC.  No leaf output: a pruned node never forms its leaf beliefs.
 *
 * THEOREM.  If no belief of any rate-1 node of a frame is 0 (or -0.0), SSC equals SC bit for bit in u and x.  By induction over the size of a
 * rate-1 node with beliefs [a, b], none of them 0: the claim is that SC returns the signs of [a, b].  At one leaf it is the leaf rule.  Above:
 * f of two non-zero beliefs is non-zero and has the product of their signs, so by induction the left child returns c_l = sgn(a) ^ sgn(b); g
 * then gives b + a where the signs agree and b - a where they differ, the sum of two magnitudes with b's sign, non-zero, so the right child
 * returns c_r = sgn(b), and the node [c_l ^ c_r, c_r] = the signs of [a, b].  Saturation keeps signs and never gives 0 from a non-zero value,
 * and float inputs below 1e30 stay finite.  Where a belief of a rate-1 node is 0, SC decides its bits from the f and g of that node's subtree,
 * SSC decides 0 for it: the two are different decoders there, and that is the only place.  Rate-0 pruning is exact on every input.
 *
 * THE PLAN (pl_ssc_plan).  The frozen mask of a code -> steps in leaf order.  A step is a maximal rate-0 or rate-1 node of 32 leaves or more
 * (aligned, dyadic), or a single leaf block that is neither (PL_SSC_MIXED), which the rule above decodes inside the block (pl_ssc_node).  For
 * N < 32 the whole frame is one mixed step.  A step is three ints: its first leaf block, the log2 of its leaves, its kind; at most N / 32 steps.
 * Both sides walk the plan: descend to the step's node (to the level above it for a rate-0 node, whose beliefs nobody reads), decide it, and
 * combine the nodes that end with the step's last block (pl_ssc_combine from twice the step's size).
 */
#ifndef QLDPC_POLAR_SSC_CORE_H
#define QLDPC_POLAR_SSC_CORE_H

#include "qldpc_polar_core.h"

#define PL_SSC_RATE0 0
#define PL_SSC_RATE1 1
#define PL_SSC_MIXED 2
#define PL_SSC_STEP 3              /* ints of a step: first leaf block, log2 of its leaves, kind */

/* the steps of a plan, at most */
PL_FN long pl_ssc_max_steps(int log2_n) { return pl_words(log2_n); }

/* frozen: the code's frozen mask (pl_words(log2_n) words, 1 = frozen, zero past N) -> steps[][PL_SSC_STEP] in leaf order; returns their number */
PL_FN long pl_ssc_plan(int log2_n, const uint32_t *frozen, int *steps)
{
    const long W = pl_words(log2_n);
    long n_steps = 0;
    if (log2_n < PL_SUB_LOG) {
        steps[0] = 0; steps[1] = log2_n; steps[2] = PL_SSC_MIXED;
        return 1;
    }
    for (long j = 0; j < W;) {
        const uint32_t w = frozen[j];
        int t = 0;                                               /* the step: 2^t blocks from j */
        if (w != 0u && w != 0xffffffffu) {
            steps[n_steps * PL_SSC_STEP + 2] = PL_SSC_MIXED;
        } else {
            /* the largest aligned node that starts at j and holds only words like w; a uniform node that held j without starting there
               would have been taken at its own start */
            for (;;) {
                const long c = 1l << t;
                if ((j & c) || j + 2 * c > W) break;
                long k = c;
                while (k < 2 * c && frozen[j + k] == w) k++;
                if (k < 2 * c) break;
                t++;
            }
            steps[n_steps * PL_SSC_STEP + 2] = w ? PL_SSC_RATE0 : PL_SSC_RATE1;
        }
        steps[n_steps * PL_SSC_STEP] = (int)j;
        steps[n_steps * PL_SSC_STEP + 1] = t + PL_SUB_LOG;
        n_steps++;
        j += 1l << t;
    }
    return n_steps;
}

/* pl_combine_words with its first half-width given and bounded: the nodes of 2 h words, h0 <= h < h1, that end with word j get
   first half ^= second half, smallest first.  (h0, h1) = (1, c) inside a node of c words, (c, W) after a step of c words */
PL_FN void pl_ssc_combine(uint32_t *x, long j, long stride, long h0, long h1)
{
    for (long h = h0; h < h1 && (j & h); h <<= 1)
        for (long k = 0; k < h; k++) x[(j + 1 - 2 * h + k) * stride] ^= x[(j + 1 - h + k) * stride];
}

/* the bits pos .. pos + 2^sl - 1 (MSB-first) of a word: a node of 2^sl leaves inside a leaf block */
PL_FN uint32_t pl_ssc_field(int sl, int pos) { return (0xffffffffu << (32 - (1 << sl))) >> pos; }
/* the kind of that node from the block's frozen word */
PL_FN int pl_ssc_kind(uint32_t frozen, uint32_t field) { return (frozen & field) == field ? PL_SSC_RATE0 : ((frozen & field) == 0u ? PL_SSC_RATE1 : PL_SSC_MIXED); }

/* The rule inside a leaf block, as a lane holds it in registers: a node of 2^sl <= 32 leaves whose first leaf is bit pos of the block's words,
 * beliefs L[2^sl] -> decisions into *u, the returned bits of every finished node into *x.  pl_enc_word of a word that is zero outside an
 * aligned field of 2^sl bits stays inside the field: what a stage m < 2^sl shifts out of it lands in the second half of a block of 2m bits. */
#define PL_SSC_HOST_LEAF_BLOCK(SUF, TIN, T, LOAD, F, G)                                                                                    \
    static void pl_ssc_node_##SUF(int maxq, const T *L, int sl, int pos, uint32_t frozen, uint32_t value, uint32_t *u, uint32_t *x)        \
    {                                                                                                                                      \
        (void)maxq;                                                                                                                        \
        const uint32_t field = pl_ssc_field(sl, pos);                                                                                      \
        const int kind = pl_ssc_kind(frozen, field), s = 1 << sl, h = s / 2;                                                               \
        if (kind == PL_SSC_RATE0) {                                                                                                        \
            *u |= value & field;                                                                                                           \
            *x |= pl_enc_word(value & field, sl);                                                                                          \
            return;                                                                                                                        \
        }                                                                                                                                  \
        if (kind == PL_SSC_RATE1) {                                                                                                        \
            uint32_t c = 0u;                                                                                                               \
            for (int k = 0; k < s; k++) c |= (uint32_t)(L[k] < 0) << (31 - pos - k);                                                        \
            *x |= c;                                                                                                                       \
            *u |= pl_enc_word(c, sl);                                                                                                      \
            return;                                                                                                                        \
        }                                                                                                                                  \
        T l[16] = {0};                                                                                                                     \
        for (int k = 0; k < h; k++) l[k] = F(L[k], L[k + h]);                                                                              \
        pl_ssc_node_##SUF(maxq, l, sl - 1, pos, frozen, value, u, x);                                                                      \
        for (int k = 0; k < h; k++) l[k] = G(L[k], L[k + h], pl_bit(*x, pos + k));                                                         \
        pl_ssc_node_##SUF(maxq, l, sl - 1, pos + h, frozen, value, u, x);                                                                  \
        *x ^= (*x << h) & ((0xffffffffu << (32 - h)) >> pos);                                                                              \
    }

#endif /* QLDPC_POLAR_SSC_CORE_H */
