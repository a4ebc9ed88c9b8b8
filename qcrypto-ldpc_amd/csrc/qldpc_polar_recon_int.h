/*
 * qldpc_polar_recon_int.h -- the argument checks that the host mirrors of the polar reconciliation sessions (qldpc_polar_recon_host.c, where they
 * are defined) and the device side (qldpc_polar_recon.hip) share, worded once.  `who` names the call in every message; each returns QLDPC_OK or
 * the status of the first refusal, with the message set.  None of them touches a device.
 */
#ifndef QLDPC_POLAR_RECON_INT_H
#define QLDPC_POLAR_RECON_INT_H

#include "qldpc_polar_int.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the session's CRC on a code of n_info bits: crc_len in 1 .. min(32, n_info), crc_poly within crc_len bits (QLDPC_ESIZE) */
int prc_args_crc(const char *who, int crc_len, uint32_t crc_poly, int n_info);
/* prior and pin against the messages (qldpc_polar_recon_core.h: prc_levels) -> the two integers and the two floats (QLDPC_EINVAL) */
int prc_args_levels(const char *who, int messages, int maxq, double prior, double pin, int *pi, int *qi, float *pf, float *qf);
/* a block count: negative is QLDPC_EINVAL */
int prc_args_count(const char *who, int n_blocks);
/* a verdict call: the size, n_info in 0 .. N, the CRC where no pick decides (then info and crc are required too), x, keys and status */
int prc_args_verdict(const char *who, int log2_n, int n_info, int crc_len, uint32_t crc_poly, int n_blocks, const void *info, const void *x, const void *pick,
                     const void *keys, const void *crc, const void *status);

/* a ladder (qldpc_polar_ladder_core.h: pld_rank_table; defined in qldpc_polar_ladder_host.c) against the code's frozen mask -> rank[N]: n_extra outside
   0 .. n_info is QLDPC_ESIZE, an entry that is no information position or comes twice QLDPC_EINVAL */
int pld_args_ladder(const char *who, int log2_n, const uint32_t *fmask, int n_info, int n_extra, const int *extra_pos, int *rank);
/* the scalars of a rounds call: step >= 1, max_rounds >= 1, resume 0 or 1 (QLDPC_EINVAL) */
int pld_args_rounds(const char *who, int step, int max_rounds, int resume);
/* the slot prior of the host mirrors (defined in qldpc_polar_ladder_host.c): one block's LLR row [N] (int8 or float), frozen values [W] and added
   flags [W] at its count `extra`, from its key row, key_bits as the caller gave it, syndrome row and extra row (either may be NULL where nothing
   of it is looked at); mask, prefix: the code's tables; rank: the ladder's */
void pld_host_slot(int log2_n, int i8, const uint32_t *mask, const int *prefix, const int *rank, int pi, int qi, float pf, float qf, const uint32_t *key,
                   int key_bits, const uint32_t *syn, const uint32_t *xbits, int extra, void *llr, uint32_t *frozen, uint32_t *flags);

/* the scalars of a flip call (qldpc_polar_flip_core.h; defined in qldpc_polar_flip_host.c): n_flips a power of two >= 1 and resume 0 or 1
   (QLDPC_EINVAL), n_flips at most max_flips (QLDPC_ESIZE) */
int pfl_args_flips(const char *who, int n_flips, int max_flips, int resume);

#ifdef __cplusplus
}
#endif

#endif /* QLDPC_POLAR_RECON_INT_H */
