/*
 * qldpc_recon_guess_core.h -- the verdict of a guessing round inside a reconciliation session (qldpc_recon_decode_guess), plain C, shared by the kernels
 * (rk_guess_crc, rk_guess_settle in qldpc_kernels_recon_guess.h) and by their host mirror (qldpc_recon_guess_settle_host in qldpc_recon_guess_host.c),
 * so that the CPU suite runs what the lanes run.  Guess set, ranks, trials and the known / value rows are those of qldpc_guess_core.h, unchanged.
 *
 *   source     a block whose first decode ended QLDPC_EDECODE (syndrome or CRC); its T = 2^g trials are its own frame decoded from scratch with the
 *              guess set pinned (qldpc_guess_core.h)
 *   ok(t)      the syndrome of trial t's hard decision is zero (qldpc_fetch_status_dev)
 *   pass(t)    ok(t) && CRC-32 of the trial's key bits below key_bits == the CRC of Alice's key (msgs[i].crc32): the verdict rk_verify gives a
 *              first decode
 *   winner     the lowest passing t, or -1; n_ok, n_pass = the numbers of ok / passing trials
 *   ambiguous  some passing trial's key differs from the winner's in a bit below key_bits (the padding of the last key word and everything
 *              past the key do not count)
 *   result     with a winner: QLDPC_OK, the winner's key words (tail masked), corrected = the bits in which they differ from the key handed
 *              in, iterations = the first decode's + the winner's.  Without: QLDPC_EDECODE, the key handed in, corrected = 0, iterations =
 *              the first decode's.  The CRC column holds the CRC of the winner's key, without a winner that of trial 0's.
 *   trial_iterations = the sum of the iterations of the T trials
 *
 * The pool of an entry keeps what a source needs until its trial launch, `cap` sources, as 32-bit words from `base` (recon_guess_pool_layout):
 *   weak [cap][Wn] | hard [cap][Wn] | frame bits [cap][Wn] | erase [cap][Wn] | key handed in [cap][Wk] | |LLR| | key_bits | Alice's CRC | first
 *   decode's iterations [cap] each.
 */
#ifndef QLDPC_RECON_GUESS_CORE_H
#define QLDPC_RECON_GUESS_CORE_H

#include "qldpc_guess_core.h"
#include "qldpc_recon_core.h"

#define RG_FIELDS 6      /* the ints of a qldpc_recon_guess, in its order: tried, winner, n_ok, n_pass, ambiguous, trial_iterations */

RC_FN int rg_pass(int ok, uint32_t crc, uint32_t want) { return ok != 0 && crc == want; }
/* do the key words i of two trials differ in a bit below key_bits? */
RC_FN int rg_differs(uint32_t a, uint32_t b, int i, int key_bits) { return ((a ^ b) & tail_mask(i, (key_bits + 31) / 32, key_bits)) != 0u; }
/* status and iterations of a source from its winner (-1: none): the values of QLDPC_OK / QLDPC_EDECODE come from the caller (include/qldpc.h) */
RC_FN int rg_iterations(int first, int winner, int winner_iters) { return winner >= 0 ? first + winner_iters : first; }

typedef struct recon_guess_pool_view {
    uint32_t *weak, *hard, *bits, *erase, *keys;
    float *mag;
    int *key_bits;
    uint32_t *crc;
    int *iters;
    size_t words;
} recon_guess_pool_view;
RC_FN recon_guess_pool_view recon_guess_pool_layout(uint32_t *base, int cap, int Wk, int Wn)
{
    const size_t C = (size_t)cap, row = C * (size_t)Wn, cols = 4 * row + C * (size_t)Wk;
    recon_guess_pool_view v;
    v.weak = base; v.hard = RC_COL(uint32_t, base, row); v.bits = RC_COL(uint32_t, base, 2 * row); v.erase = RC_COL(uint32_t, base, 3 * row);
    v.keys = RC_COL(uint32_t, base, 4 * row);
    v.mag = RC_COL(float, base, cols); v.key_bits = RC_COL(int, base, cols + C); v.crc = RC_COL(uint32_t, base, cols + 2 * C); v.iters = RC_COL(int, base, cols + 3 * C);
    v.words = cols + 4 * C;
    return v;
}

#endif /* QLDPC_RECON_GUESS_CORE_H */
