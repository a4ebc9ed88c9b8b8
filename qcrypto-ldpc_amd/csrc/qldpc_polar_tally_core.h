/*
 * qldpc_polar_tally_core.h -- the rule of the genie-aided code construction of qldpc_polar_tally_* and qldpc_polar_construct_*.  Plain C, shared
 * by the kernel (qldpc_kernels_polar_tally.h), the host mirror and the ordering helpers (qldpc_polar_tally_host.c).
 *
 *   genie     for a frame with true row u, L_p is the leaf belief of the SC decoder of qldpc_polar_core.h with EVERY position frozen to u: what
 *             position p would see if all earlier decisions were right (Arikan's Monte-Carlo construction).
 *   tie       position p of the frame is a tie iff L_p == 0; a float -0.0 is a tie.
 *   wrong     position p of the frame is wrong iff L_p != 0 and (L_p < 0) != u_p.
 *   tally     over a set of frames, tally[0][p] = the wrong frames and tally[1][p] = the ties of position p: a row of [2][N] uint64 counts.
 *   score     score[p] = 2 wrong + ties, an integer.  score / (2 frames) estimates the error probability of position p under a uniformly random
 *             bit: a tie decides 0 and is wrong half the time, and counting it as 1/2 takes that coin's variance out.
 *   order     ascending reliability, the convention of a reliability sequence: the key is (score descending, rank in a prior order ascending),
 *             so a code of K bits takes the LAST K positions.
 *   K         the largest K whose last K positions of an order have a score sum <= a given bound; for a union bound eps over `frames` frames
 *             the bound is floor(2 frames eps).
 *
 * Everything is an integer and no float sum appears anywhere: device, mirror and restatement agree count for count in any order of addition.
 * A count above PLT_MAX_COUNT = 2^40 is refused by the helpers, so that a score sum over 2^20 positions stays below 2^63.
 */
#ifndef QLDPC_POLAR_TALLY_CORE_H
#define QLDPC_POLAR_TALLY_CORE_H

#include "qldpc_polar_core.h"

#define PLT_MAX_COUNT (1ull << 40)

PL_FN unsigned plt_tie_i8(int L) { return L == 0; }
PL_FN unsigned plt_tie_f32(float L) { return L == 0.0f; }        /* -0.0 too */
PL_FN unsigned plt_wrong_i8(int L, unsigned u) { return L != 0 && (unsigned)(L < 0) != u; }
PL_FN unsigned plt_wrong_f32(float L, unsigned u) { return L != 0.0f && (unsigned)(L < 0.0f) != u; }

PL_FN uint64_t plt_score(uint64_t wrong, uint64_t ties) { return 2u * wrong + ties; }
PL_FN int plt_check_count(uint64_t wrong, uint64_t ties) { return wrong <= PLT_MAX_COUNT && ties <= PLT_MAX_COUNT ? 0 : PL_ESIZE; }

/* The wrong word and the tie word of a leaf block of s <= 32 leaves: bit i (LSB-first, so that lane i of a wave bit transpose gets position i)
 * says it of leaf i, whose true bit is bit i (MSB-first) of `truth`.  X(SUF, TIN, T, ..) as qldpc_polar_core.h's PL_HOST_MESSAGES wants it;
 * a lane builds the same two words from its registers, unrolled, with the four functions above */
#define PLT_BLOCK_WORDS(SUF, TIN, T, LOAD, F, G)                                                                              \
    PL_FN void plt_block_words_##SUF(const T *leaf, int s, uint32_t truth, uint32_t *wrong, uint32_t *tie)                   \
    {                                                                                                                         \
        uint32_t w = 0u, t = 0u;                                                                                              \
        for (int i = 0; i < s; i++) {                                                                                         \
            t |= (uint32_t)plt_tie_##SUF(leaf[i]) << i;                                                                       \
            w |= (uint32_t)plt_wrong_##SUF(leaf[i], pl_bit(truth, i)) << i;                                                   \
        }                                                                                                                     \
        *wrong = w; *tie = t;                                                                                                 \
    }
PL_HOST_MESSAGES(PLT_BLOCK_WORDS)

#endif /* QLDPC_POLAR_TALLY_CORE_H */
