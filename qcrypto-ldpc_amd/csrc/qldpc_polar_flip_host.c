/*
 * qldpc_polar_flip_host.c -- the host mirrors of SC-Flip trials in the polar reconciliation sessions (qldpc_polar_flip_select_host,
 * qldpc_polar_recon_decode_flip_host): plain C over the functions of qldpc_polar_flip_core.h that the kernels of qldpc_kernels_polar_flip.h run
 * per lane.  The first pass is qldpc_polar_recon_decode_rounds_host with one round; an open block is then taken on its own: the probe and its T
 * trials are 1 + T frames of qldpc_polar_decode_rows_host.  There is no chunking here, and none shows in any output of the device.  And the
 * check of a flip call's scalars that the mirrors and the session share (qldpc_polar_recon_int.h).  No device.
 */
#include <stdlib.h>
#include <string.h>

#include "qldpc_polar_flip_core.h"
#include "qldpc_polar_recon_int.h"

int pfl_args_flips(const char *who, int n_flips, int max_flips, int resume)
{
    if (!pfl_flips_pow2(n_flips) || (resume != 0 && resume != 1)) {
        qldpc_set_error("%s: n_flips=%d, resume=%d (n_flips a power of two in 1 .. %d, resume 0 or 1)", who, n_flips, resume, PFL_MAX_FLIPS);
        return QLDPC_EINVAL;
    }
    if (n_flips > max_flips) { qldpc_set_error("%s: n_flips=%d exceeds max_flips=%d", who, n_flips, max_flips); return QLDPC_ESIZE; }
    return QLDPC_OK;
}

int qldpc_polar_flip_select_host(int log2_n, int messages, int n_frames, const void *leaf, const uint32_t *frozen_mask, const int *rank, const int *extra,
                                 int n_flips, int *pos)
{
    const char *who = "polar_flip_select_host";
    int rc = pl_args_scalars(who, log2_n, PL_MAX_LOG2N, messages, 1);
    if (!rc) rc = prc_args_count(who, n_frames);
    if (!rc) rc = pfl_args_flips(who, n_flips, PFL_MAX_FLIPS, 0);
    if (rc || n_frames == 0) return rc;
    if (!leaf || !frozen_mask || !pos) { qldpc_set_error("%s: NULL pointer (leaf, frozen_mask and pos are required)", who); return QLDPC_EINVAL; }
    const size_t N = (size_t)1 << log2_n, esz = messages == QLDPC_POLAR_I8 ? 1 : sizeof(float);
    for (long f = 0; f < n_frames; f++)
        pfl_select_row(log2_n, messages == QLDPC_POLAR_I8, (const char *)leaf + esz * N * (size_t)f, frozen_mask, rank, rank && extra ? extra[f] : 0, n_flips,
                       pos + (size_t)f * (size_t)n_flips);
    return QLDPC_OK;
}

int qldpc_polar_recon_decode_flip_host(int log2_n, int n_info, const int *info_pos, int messages, int maxq, int crc_len, uint32_t crc_poly, double prior,
                                       double pin, int n_extra, const int *extra_pos, int n_blocks, uint32_t *keys, const int *key_bits,
                                       const uint32_t *syndrome, const uint32_t *crc, const uint32_t *extra_bits, const int *extra, int n_flips, int resume,
                                       int *status, int *corrected, int32_t *flip_pos, int *decodes, int *n_tried)
{
    const char *who = "polar_recon_decode_flip_host";
    uint32_t *mask = NULL;
    int pi, qi;
    float pf, qf;
    int rc = pl_args_scalars(who, log2_n, PL_MAX_LOG2N, messages, maxq);
    if (!rc) rc = prc_args_levels(who, messages, maxq, prior, pin, &pi, &qi, &pf, &qf);
    if (!rc) rc = prc_args_count(who, n_blocks);
    if (!rc) rc = pfl_args_flips(who, n_flips, PFL_MAX_FLIPS, resume);
    if (rc) return rc;
    if ((rc = pl_args_frozen_mask(who, log2_n, n_info, info_pos, &mask))) return rc;
    const long N = 1l << log2_n, W = pl_words(log2_n), Nf = N - n_info, Wf = pmc_words((int)Nf), Wi = pmc_words(n_info);
    if ((rc = prc_args_crc(who, crc_len, crc_poly, n_info))) { free(mask); return rc; }
    int *rank = (int *)malloc(sizeof(int) * (size_t)N);
    if (!rank) { free(mask); return QLDPC_ENOMEM; }
    if ((rc = pld_args_ladder(who, log2_n, mask, n_info, n_extra, extra_pos, rank))) { free(rank); free(mask); return rc; }
    const long We = pld_extra_words(n_extra);
    if (n_blocks > 0 && (!keys || !crc || !status || !flip_pos || (Nf > 0 && !syndrome) || (n_extra > 0 && !extra_bits))) {
        free(rank); free(mask);
        qldpc_set_error("%s: NULL pointer (keys, crc, status and flip_pos are required; syndrome where N > K, extra_bits where n_extra > 0)", who);
        return QLDPC_EINVAL;
    }
    if (n_tried) *n_tried = 0;
    if (n_blocks == 0) { free(rank); free(mask); return QLDPC_OK; }
    const int T = n_flips, i8 = messages == QLDPC_POLAR_I8;
    const size_t esz = i8 ? 1 : sizeof(float), nb = (size_t)n_blocks;
    int *prefix = (int *)malloc(sizeof(int) * (size_t)W), *ex = (int *)malloc(sizeof(int) * nb), *open = (int *)malloc(sizeof(int) * nb);
    void *llr = malloc(esz * (size_t)T * (size_t)N), *leaf = malloc(esz * (size_t)N);
    uint32_t *rows = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)T * (size_t)(3 * W + Wi + 1));
    if (!prefix || !ex || !open || !llr || !leaf || !rows) rc = QLDPC_ENOMEM;
    uint32_t *frozen = rows, *flags = rows ? rows + (size_t)T * (size_t)W : NULL, *xh = rows ? flags + (size_t)T * (size_t)W : NULL, *ih = rows ? xh + (size_t)T * (size_t)W : NULL;
    int pos[PFL_MAX_FLIPS];
    long n_open = 0;
    if (!rc) {
        prc_tables(log2_n, mask, prefix, NULL);
        for (long b = 0; b < n_blocks; b++) { ex[b] = extra ? extra[b] : 0; flip_pos[b] = -1; }
    }
    if (!rc && !resume) {                                         /* the first pass: every valid block once, at its count */
        rc = qldpc_polar_recon_decode_rounds_host(log2_n, n_info, info_pos, messages, maxq, crc_len, crc_poly, prior, pin, n_extra, extra_pos, n_blocks, keys, key_bits, syndrome,
                                                  crc, extra_bits, ex, 1, 1, 0, status, corrected, decodes, NULL);
        for (long b = 0; b < n_blocks && !rc; b++)
            if (status[b] == PRC_EDECODE) open[n_open++] = (int)b;
    } else if (!rc) {                                             /* the entry of a resumed call */
        for (long b = 0; b < n_blocks; b++) {
            if (decodes) decodes[b] = 0;
            const int what = pld_entry(1, status[b], key_bits ? key_bits[b] : (int)N, log2_n, ex[b], n_extra);
            if (what == PLD_OPEN) open[n_open++] = (int)b;
            else if (what == PLD_REFUSE) { status[b] = PRC_ESIZE; if (corrected) corrected[b] = -1; }
        }
    }
    if (!rc && n_tried) *n_tried = (int)n_open;
    for (long o = 0; o < n_open && !rc; o++) {
        const long b = open[o];
        const int kb = key_bits ? key_bits[b] : (int)N;
        /* the probe: the failed decode again, for its leaf beliefs */
        pld_host_slot(log2_n, i8, mask, prefix, rank, pi, qi, pf, qf, keys + b * W, kb, syndrome ? syndrome + b * Wf : NULL, extra_bits ? extra_bits + b * We : NULL, ex[b], llr,
                      frozen, flags);
        if ((rc = qldpc_polar_decode_rows_host(log2_n, n_info, info_pos, messages, maxq, 1, llr, frozen, flags, NULL, NULL, NULL, leaf))) break;
        pfl_select_row(log2_n, i8, leaf, mask, rank, ex[b], T, pos);
        for (int t = T - 1; t >= 0; t--) {                        /* the trials: the base inputs (slot 0, copied last to first) plus the flip */
            if (t) {
                memcpy((char *)llr + esz * (size_t)t * (size_t)N, llr, esz * (size_t)N);
                memcpy(frozen + (size_t)t * (size_t)W, frozen, sizeof(uint32_t) * (size_t)W);
                memcpy(flags + (size_t)t * (size_t)W, flags, sizeof(uint32_t) * (size_t)W);
            }
            const int p = pos[t];
            if (p < 0) continue;
            const unsigned bit = i8 ? pfl_flip_bit_i8(((const int8_t *)leaf)[p]) : pfl_flip_bit_f32(((const float *)leaf)[p]);
            const uint32_t m = 1u << (31 - (p & 31));
            flags[(size_t)t * (size_t)W + (size_t)(p >> 5)] |= m;
            frozen[(size_t)t * (size_t)W + (size_t)(p >> 5)] = (frozen[(size_t)t * (size_t)W + (size_t)(p >> 5)] & ~m) | (bit ? m : 0u);
        }
        if ((rc = qldpc_polar_decode_rows_host(log2_n, n_info, info_pos, messages, maxq, T, llr, frozen, flags, NULL, ih, xh, NULL))) break;
        uint32_t accept = 0u;
        for (int t = 0; t < T; t++)
            if (pos[t] >= 0 && prc_accept_block(log2_n, n_info, crc_len, crc_poly, ih + (size_t)t * (size_t)Wi, xh + (size_t)t * (size_t)W, 0, 0, kb, crc[b])) accept |= 1u << t;
        const int win = pfl_winner(accept);
        if (win >= 0) {
            const int co = prc_take_block(log2_n, xh + (size_t)win * (size_t)W, keys + b * W, kb);
            status[b] = PRC_OK;
            if (corrected) corrected[b] = co;
            flip_pos[b] = pos[win];
        } else {
            status[b] = PRC_EDECODE;
            if (corrected) corrected[b] = -1;
        }
        if (decodes) decodes[b] += 1 + T;
    }
    free(prefix); free(ex); free(open); free(llr); free(leaf); free(rows); free(rank); free(mask);
    return rc;
}
