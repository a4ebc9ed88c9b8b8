/*
 * qldpc_giveup_core.h -- the definition of "this frame's syndrome weight has stopped falling: give it up" (cfg.giveup_patience), plain C, shared by
 * the status kernel of the early-exit run (qk_status_count in qldpc_kernels_giveup.h) and by its host mirror (qldpc_giveup_host in
 * qldpc_blind_host.c), so that the CPU suite runs what the lanes run.
 *
 *   weight   w of a frame at a syndrome test = the number of checks c with (H x + s)_c = 1 over the sign ballots that test reads.  The tests are
 *            the ones the run makes anyway: flooding after iterations 1 .. n_ite - 1, horizontal layered after every sweep
 *   state    {best, since} per frame: the smallest weight seen so far (< 0: no test yet) and the number of tests since it was seen
 *   observe  first test, or w < best: best = w, since = 0 (a zero weight is a new minimum like any other); otherwise since += 1
 *   converge AFF3CT's cur_syndrome_depth logic, untouched: a frame that converges at a test converges whatever `since` says
 *   give up  a frame that is not done, did not converge at this test, has w > 0 and since >= patience
 */
#ifndef QLDPC_GIVEUP_CORE_H
#define QLDPC_GIVEUP_CORE_H

#if defined(__HIPCC__)
#define GU_FN __host__ __device__ static inline
#else
#define GU_FN static inline
#endif

/* the outcomes of qldpc_giveup_host (qldpc.h: QLDPC_GIVEUP_*) */
#define GU_CONVERGED 0
#define GU_GAVE_UP 1
#define GU_RAN_OUT 2

GU_FN void gu_reset(int *best, int *since) { *best = -1; *since = 0; }

GU_FN void gu_observe(int *best, int *since, int w)
{
    if (*best < 0 || w < *best) { *best = w; *since = 0; }
    else (*since)++;
}

/* the convergence test of the status pass: `zero` = the syndrome is zero at this test; *depth = consecutive zero syndromes so far, modulo
 * syndrome_depth.  Returns 1 when the frame converges at this test */
GU_FN int gu_converges(int *depth, int zero, int syndrome_depth)
{
    *depth = zero ? (*depth + 1) % syndrome_depth : 0;
    return zero && *depth == 0;
}

/* after gu_observe and gu_converges of the same test */
GU_FN int gu_gives_up(int w, int since, int patience, int converged_now) { return !converged_now && w > 0 && since >= patience; }

#endif /* QLDPC_GIVEUP_CORE_H */
