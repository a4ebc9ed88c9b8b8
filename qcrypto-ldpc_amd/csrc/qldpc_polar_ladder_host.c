/*
 * qldpc_polar_ladder_host.c -- the host mirrors of incremental freezing in the polar reconciliation sessions (qldpc_polar_recon_encode_ladder_host,
 * _decode_rounds_host, _ladder_extra_host): plain C over the functions of qldpc_polar_ladder_core.h that the kernels of
 * qldpc_kernels_polar_ladder.h run per lane, here in a loop over blocks and words; a round runs qldpc_polar_decode_rows_host between the slot
 * prior and the slot verdict.  And the check of a ladder that the mirrors and the session share (qldpc_polar_recon_int.h).  No device.
 */
#include <stdlib.h>
#include <string.h>

#include "qldpc_polar_ladder_core.h"
#include "qldpc_polar_recon_int.h"

int pld_args_ladder(const char *who, int log2_n, const uint32_t *fmask, int n_info, int n_extra, const int *extra_pos, int *rank)
{
    const int rc = pld_rank_table(log2_n, fmask, n_info, n_extra, extra_pos, rank);
    if (rc == PRC_ESIZE) { qldpc_set_error("%s: n_extra=%d (0 .. n_info = %d)", who, n_extra, n_info); return QLDPC_ESIZE; }
    if (rc) { qldpc_set_error("%s: extra_pos must hold n_extra=%d distinct information positions of the code", who, n_extra); return QLDPC_EINVAL; }
    return QLDPC_OK;
}

int pld_args_rounds(const char *who, int step, int max_rounds, int resume)
{
    if (step < 1 || max_rounds < 1 || (resume != 0 && resume != 1)) {
        qldpc_set_error("%s: step=%d, max_rounds=%d, resume=%d (step >= 1, max_rounds >= 1, resume 0 or 1)", who, step, max_rounds, resume);
        return QLDPC_EINVAL;
    }
    return QLDPC_OK;
}

void pld_host_slot(int log2_n, int i8, const uint32_t *mask, const int *prefix, const int *rank, int pi, int qi, float pf, float qf, const uint32_t *key,
                   int key_bits, const uint32_t *syn, const uint32_t *xbits, int extra, void *llr, uint32_t *frozen, uint32_t *flags)
{
    const long N = 1l << log2_n, W = pl_words(log2_n);
    const int kb = prc_key_bits(key_bits, log2_n);
    for (long i = 0; i < N; i++) {
        const unsigned bit = pl_bit(key[i >> 5], (int)(i & 31));
        if (i8) ((int8_t *)llr)[i] = (int8_t)PRC_LEVEL(i, bit, kb, pi, qi);
        else ((float *)llr)[i] = PRC_LEVEL(i, bit, kb, pf, qf);
    }
    for (long w = 0; w < W; w++) {
        uint32_t fl, va;
        pld_ladder_bits(rank, log2_n, (size_t)w, 0, 32, extra, xbits, &fl, &va);
        frozen[w] = prc_frozen_bits(syn, mask[w], (uint32_t)prefix[w], 0, 32) | va;
        flags[w] = fl;
    }
}

static int pld_null(const char *who, const char *what)
{
    qldpc_set_error("%s: %s is NULL", who, what);
    return QLDPC_EINVAL;
}

int qldpc_polar_recon_encode_ladder_host(int log2_n, int n_info, const int *info_pos, int crc_len, uint32_t crc_poly, int n_extra, const int *extra_pos,
                                         int n_blocks, const uint32_t *keys, const int *key_bits, uint32_t *syndrome, uint32_t *crc, uint32_t *extra_bits)
{
    const char *who = "polar_recon_encode_ladder_host";
    uint32_t *mask = NULL;
    if (pl_check_size(log2_n, PL_MAX_LOG2N)) { qldpc_set_error("%s: log2_n=%d (1 .. %d)", who, log2_n, PL_MAX_LOG2N); return QLDPC_ESIZE; }
    int rc = prc_args_count(who, n_blocks);
    if (rc) return rc;
    if ((rc = pl_args_frozen_mask(who, log2_n, n_info, info_pos, &mask))) return rc;
    const long N = 1l << log2_n, W = pl_words(log2_n), We = pld_extra_words(n_extra > 0 ? n_extra : 0);
    int *rank = (int *)malloc(sizeof(int) * (size_t)N);
    uint32_t *urow = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)W);
    if (!rank || !urow) rc = QLDPC_ENOMEM;
    if (!rc) rc = pld_args_ladder(who, log2_n, mask, n_info, n_extra, extra_pos, rank);
    if (!rc && n_blocks > 0 && n_extra > 0 && !extra_bits) rc = pld_null(who, "extra_bits");
    /* syndrome and crc are the plain call's, with its refusals */
    if (!rc) rc = qldpc_polar_recon_encode_host(log2_n, n_info, info_pos, crc_len, crc_poly, n_blocks, keys, key_bits, syndrome, crc);
    for (long f = 0; f < n_blocks && !rc; f++) {
        const int kb = prc_key_bits(key_bits ? key_bits[f] : (int)N, log2_n);
        for (long w = 0; w < W; w++) urow[w] = keys[f * W + w] & prc_key_mask(kb, (uint32_t)w);
        qldpc_polar_encode_host(log2_n, 1, urow, urow);
        for (long j = 0; j < We; j++) extra_bits[f * We + j] = prc_gather_word(urow, extra_pos, n_extra, (size_t)j);
    }
    free(rank); free(urow); free(mask);
    return rc;
}

#define PLD_HOST_CHUNK 256         /* slots whose LLR rows the rounds mirror holds at a time */

int qldpc_polar_recon_decode_rounds_host(int log2_n, int n_info, const int *info_pos, int messages, int maxq, int crc_len, uint32_t crc_poly, double prior,
                                         double pin, int n_extra, const int *extra_pos, int n_blocks, uint32_t *keys, const int *key_bits,
                                         const uint32_t *syndrome, const uint32_t *crc, const uint32_t *extra_bits, int *extra, int step, int max_rounds,
                                         int resume, int *status, int *corrected, int *decodes, int *open_per_round)
{
    const char *who = "polar_recon_decode_rounds_host";
    uint32_t *mask = NULL;
    int pi, qi;
    float pf, qf;
    int rc = pl_args_scalars(who, log2_n, PL_MAX_LOG2N, messages, maxq);
    if (!rc) rc = prc_args_levels(who, messages, maxq, prior, pin, &pi, &qi, &pf, &qf);
    if (!rc) rc = prc_args_count(who, n_blocks);
    if (!rc) rc = pld_args_rounds(who, step, max_rounds, resume);
    if (rc) return rc;
    if ((rc = pl_args_frozen_mask(who, log2_n, n_info, info_pos, &mask))) return rc;
    const long N = 1l << log2_n, W = pl_words(log2_n), Nf = N - n_info, Wf = pmc_words((int)Nf), Wi = pmc_words(n_info);
    if ((rc = prc_args_crc(who, crc_len, crc_poly, n_info))) { free(mask); return rc; }
    int *rank = (int *)malloc(sizeof(int) * (size_t)N);
    if (!rank) { free(mask); return QLDPC_ENOMEM; }
    if ((rc = pld_args_ladder(who, log2_n, mask, n_info, n_extra, extra_pos, rank))) { free(rank); free(mask); return rc; }
    const long We = pld_extra_words(n_extra);
    if (n_blocks > 0 && (!keys || !crc || !status || !extra || (Nf > 0 && !syndrome) || (n_extra > 0 && !extra_bits))) {
        free(rank); free(mask);
        return pld_null(who, !keys ? "keys" : (!crc ? "crc" : (!status ? "status" : (!extra ? "extra" : (Nf > 0 && !syndrome ? "syndrome" : "extra_bits")))));
    }
    const size_t C = PLD_HOST_CHUNK, esz = messages == QLDPC_POLAR_I8 ? 1 : sizeof(float);
    int *prefix = (int *)malloc(sizeof(int) * (size_t)W);
    int *open = (int *)malloc(sizeof(int) * 2 * (size_t)(n_blocks > 0 ? n_blocks : 1));
    void *llr = malloc(esz * C * (size_t)N);
    uint32_t *rows = (uint32_t *)malloc(sizeof(uint32_t) * C * (size_t)(3 * W + Wi + 1));
    if (!prefix || !open || !llr || !rows) rc = QLDPC_ENOMEM;
    uint32_t *frozen = rows, *flags = rows ? rows + C * (size_t)W : NULL, *xh = rows ? flags + C * (size_t)W : NULL, *ih = rows ? xh + C * (size_t)W : NULL;
    int *cur = open, *next = open ? open + (n_blocks > 0 ? n_blocks : 1) : NULL;
    long n_open = 0;
    if (!rc) {
        prc_tables(log2_n, mask, prefix, NULL);
        for (int t = 0; open_per_round && t < max_rounds; t++) open_per_round[t] = 0;
        for (long b = 0; b < n_blocks; b++) {                   /* the entry */
            if (decodes) decodes[b] = 0;
            const int kb = key_bits ? key_bits[b] : (int)N, what = pld_entry(resume, resume ? status[b] : 0, kb, log2_n, extra[b], n_extra);
            if (what == PLD_OPEN) cur[n_open++] = (int)b;
            else if (what == PLD_REFUSE) { status[b] = PRC_ESIZE; if (corrected) corrected[b] = -1; }
        }
    }
    for (int t = 0; t < max_rounds && n_open > 0 && !rc; t++) {
        long n_next = 0;
        if (open_per_round) open_per_round[t] = (int)n_open;
        for (long s0 = 0; s0 < n_open && !rc; s0 += (long)C) {
            const int ns = (int)(n_open - s0 < (long)C ? n_open - s0 : (long)C);
            for (int s = 0; s < ns; s++) {                        /* the slot prior: the block's LLR row, frozen values and added flags */
                const long b = cur[s0 + s];
                pld_host_slot(log2_n, messages == QLDPC_POLAR_I8, mask, prefix, rank, pi, qi, pf, qf, keys + b * W, key_bits ? key_bits[b] : (int)N,
                              syndrome ? syndrome + b * Wf : NULL, extra_bits ? extra_bits + b * We : NULL, extra[b], (char *)llr + esz * (size_t)(s * N), frozen + s * W,
                              flags + s * W);
                if (decodes) decodes[b]++;
            }
            rc = qldpc_polar_decode_rows_host(log2_n, n_info, info_pos, messages, maxq, ns, llr, frozen, flags, NULL, ih, xh, NULL);
            for (int s = 0; s < ns && !rc; s++) {                 /* the slot verdict, and who stays open */
                const long b = cur[s0 + s];
                int st, co;
                prc_verdict_block(log2_n, n_info, crc_len, crc_poly, ih + s * Wi, xh + s * W, 0, 0, keys + b * W, key_bits ? key_bits[b] : (int)N, crc[b], &st, &co);
                status[b] = st;
                if (corrected) corrected[b] = co;
                if (st == PRC_EDECODE && pld_stays_open(extra[b], n_extra, t, max_rounds)) {
                    extra[b] = pld_next_extra(extra[b], n_extra, step);
                    next[n_next++] = (int)b;
                }
            }
        }
        int *sw = cur; cur = next; next = sw;
        n_open = n_next;
    }
    free(prefix); free(open); free(llr); free(rows); free(rank); free(mask);
    return rc;
}

int qldpc_polar_recon_ladder_extra_host(int log2_n, int n_info, int n_extra, int key_bits, double qber, double f)
{
    const char *who = "polar_recon_ladder_extra_host";
    if (pl_check_size(log2_n, PL_MAX_LOG2N)) { qldpc_set_error("%s: log2_n=%d (1 .. %d)", who, log2_n, PL_MAX_LOG2N); return QLDPC_ESIZE; }
    if (n_info < 0 || n_info > (1l << log2_n) || n_extra < 0 || n_extra > n_info || !prc_key_bits_ok(key_bits, log2_n)) {
        qldpc_set_error("%s: n_info=%d, n_extra=%d, key_bits=%d (0 <= n_extra <= n_info <= N = %ld, 1 <= key_bits <= N)", who, n_info, n_extra, key_bits, 1l << log2_n);
        return QLDPC_ESIZE;
    }
    if (!(qber >= 0.0 && qber <= 0.5) || !(f >= 0.0 && f <= 1e6)) { qldpc_set_error("%s: qber=%g, f=%g (0 <= qber <= 0.5, 0 <= f <= 1e6)", who, qber, f); return QLDPC_EINVAL; }
    return pld_start_extra(log2_n, n_info, n_extra, key_bits, qber, f);
}
