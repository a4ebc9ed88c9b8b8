/*
 * qldpc_polar_int.h -- what the units of the polar subsystem share and the C ABI does not show: the argument checks of a code, worded once.
 * Defined in qldpc_polar_host.c; called by the two device contexts (through qldpc_polar_ctx.h) and by the three host mirrors.  `who` names the
 * call in every message; each returns QLDPC_OK or the status of the first refusal, with the message set.
 */
#ifndef QLDPC_POLAR_INT_H
#define QLDPC_POLAR_INT_H

#include "../../include/qldpc.h"
#include "qldpc_graph.h"
#include "qldpc_polar_core.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the scalars of a code: log2_n in 1 .. max_log2_n, messages one of the two types, maxq in 1 .. PL_MAX_MAXQ with int8 messages */
int pl_args_scalars(const char *who, int log2_n, int max_log2_n, int messages, int maxq);
/* info_pos[n_info] distinct and below N -> the code's frozen mask, a row of pl_words(log2_n) words (1 = frozen) that the caller frees */
int pl_args_frozen_mask(const char *who, int log2_n, int n_info, const int *info_pos, uint32_t **frozen_mask);
/* the argument checks of a host SC decode and, where they pass, the frozen mask */
int pl_host_decode_args(const char *who, int log2_n, int n_info, const int *info_pos, int messages, int maxq, int n_frames, const void *llr, uint32_t **frozen_mask);

/* The Monte-Carlo loop's own (defined in qldpc_polar_mc_host.c; called by the mirror of its frames and by the device object): the two modes, and
   a threshold table -- qldpc_mc_set_channel's rules and, with int8 messages, integer values in [-128, 127] -- built into *t where it passes */
struct mc_soft_table;
int pmc_args_modes(const char *who, int frozen_mode, int source_mode);
int pmc_args_table(const char *who, int messages, int levels, const uint64_t *cum0, const uint64_t *cum1, const float *value, struct mc_soft_table *t);

#ifdef __cplusplus
}
#endif

#endif /* QLDPC_POLAR_INT_H */
