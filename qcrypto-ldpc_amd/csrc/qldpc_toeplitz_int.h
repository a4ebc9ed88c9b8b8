/*
 * qldpc_toeplitz_int.h -- what the two methods of a Toeplitz context share: the context (qldpc_toeplitz.hip owns it and the direct kernel;
 * its staging and the reuse rule of that staging are qldpc_hashbatch.h's) and the entry points of the NTT method (qldpc_toeplitz_ntt.hip),
 * which qldpc_toeplitz_blocks / _blocks_dev call in place of the one direct launch once the rows of a call have been checked and laid out.
 */
#ifndef QLDPC_TOEPLITZ_INT_H
#define QLDPC_TOEPLITZ_INT_H

#include <cstddef>
#include <cstdint>

#include "qldpc_hashbatch.h"

struct tz_desc {                   /* one row per block, written by the host */
    uint32_t key_words, tail_mask, out_bits, seed_words;
    uint64_t key_off, seed_off, out_off;      /* in words from the key / seed / output base of the call */
};

struct tzn_state;                  /* tables, work area and descriptor rows of the NTT method */

struct qldpc_toeplitz_ctx {
    hb_stage st;                          /* the head of a call of n blocks: n descriptor rows; the payload: packed keys, then packed seeds */
    int method;                           /* QLDPC_TOEPLITZ_DIRECT / _NTT */
    uint64_t stats[8];                    /* of the last call (qldpc_toeplitz_stats) */
    tzn_state *ntt;
};

/* allocates everything the method needs into the ledger of tz->st; pass_log2 and work_bytes as in qldpc_toeplitz_cfg */
int tzn_create(qldpc_toeplitz_ctx *tz, int pass_log2, size_t work_bytes);
void tzn_free(qldpc_toeplitz_ctx *tz);      /* the host side of the state; hb_free(&tz->st) frees what is in the ledger */
/* the n blocks of a call whose rows `rows` describe (key_off / seed_off / out_off from d_keys / d_seeds / d_out), queued on s;
   shared: every block reads the seed row at rows[0].seed_off, which holds at least the longest seed of the call.  Fills tz->stats */
int tzn_blocks(qldpc_toeplitz_ctx *tz, int n, const tz_desc *rows, const int *key_bits, int shared,
               const uint32_t *d_keys, const uint32_t *d_seeds, uint32_t *d_out, hipStream_t s);

#endif /* QLDPC_TOEPLITZ_INT_H */
