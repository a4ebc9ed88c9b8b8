/*
 * qldpc_polar_recon_host.c -- the host mirrors of the polar reconciliation sessions (qldpc_polar_recon_*_host): plain C over the functions of
 * qldpc_polar_recon_core.h that the kernels of qldpc_kernels_polar_recon.h run per lane, here in a loop over blocks and words; the decode mirror
 * runs the existing host decoders between the prior mirror and the verdict mirror.  And the argument checks that the mirrors and the device side
 * (qldpc_polar_recon.hip) share (qldpc_polar_recon_int.h).  No device.
 */
#include <stdlib.h>
#include <string.h>

#include "qldpc_polar_recon_core.h"
#include "qldpc_polar_recon_int.h"

int prc_args_crc(const char *who, int crc_len, uint32_t crc_poly, int n_info)
{
    if (crc_len < 1 || pll_check_crc(crc_len, crc_poly, n_info)) {
        qldpc_set_error("%s: crc_len=%d, crc_poly=0x%x, n_info=%d (crc_len 1 .. 32 and at most n_info; crc_poly holds the low crc_len coefficients, x^crc_len is implied)",
                        who, crc_len, (unsigned)crc_poly, n_info);
        return QLDPC_ESIZE;
    }
    return QLDPC_OK;
}

int prc_args_levels(const char *who, int messages, int maxq, double prior, double pin, int *pi, int *qi, float *pf, float *qf)
{
    if (prc_levels(messages == QLDPC_POLAR_I8, maxq, prior, pin, pi, qi, pf, qf)) {
        qldpc_set_error("%s: prior=%g, pin=%g (QLDPC_POLAR_I8: integers, 1 <= prior <= pin <= maxq = %d; QLDPC_POLAR_F32: finite, 0 < prior <= pin <= 1e30)", who, prior,
                        pin, maxq);
        return QLDPC_EINVAL;
    }
    return QLDPC_OK;
}

int prc_args_count(const char *who, int n_blocks)
{
    if (n_blocks < 0) { qldpc_set_error("%s: n_blocks=%d is negative", who, n_blocks); return QLDPC_EINVAL; }
    return QLDPC_OK;
}

static int prc_null(const char *who, const char *what)
{
    qldpc_set_error("%s: %s is NULL", who, what);
    return QLDPC_EINVAL;
}

int qldpc_polar_recon_tables_host(int log2_n, int n_info, const int *info_pos, uint32_t *frozen_mask, int *frozen_prefix, int *frozen_pos)
{
    const char *who = "polar_recon_tables_host";
    uint32_t *mask = NULL;
    if (pl_check_size(log2_n, PL_MAX_LOG2N)) { qldpc_set_error("%s: log2_n=%d (1 .. %d)", who, log2_n, PL_MAX_LOG2N); return QLDPC_ESIZE; }
    const int rc = pl_args_frozen_mask(who, log2_n, n_info, info_pos, &mask);
    if (rc) return rc;
    prc_tables(log2_n, mask, frozen_prefix, frozen_pos);
    if (frozen_mask) memcpy(frozen_mask, mask, sizeof(uint32_t) * (size_t)pl_words(log2_n));
    free(mask);
    return QLDPC_OK;
}

int qldpc_polar_recon_encode_host(int log2_n, int n_info, const int *info_pos, int crc_len, uint32_t crc_poly, int n_blocks, const uint32_t *keys,
                                  const int *key_bits, uint32_t *syndrome, uint32_t *crc)
{
    const char *who = "polar_recon_encode_host";
    uint32_t *mask = NULL;
    if (pl_check_size(log2_n, PL_MAX_LOG2N)) { qldpc_set_error("%s: log2_n=%d (1 .. %d)", who, log2_n, PL_MAX_LOG2N); return QLDPC_ESIZE; }
    int rc = prc_args_count(who, n_blocks);
    if (rc) return rc;
    if ((rc = pl_args_frozen_mask(who, log2_n, n_info, info_pos, &mask))) return rc;
    const long N = 1l << log2_n, W = pl_words(log2_n), Nf = N - n_info, Wf = pmc_words((int)Nf), Wi = pmc_words(n_info);
    if ((rc = prc_args_crc(who, crc_len, crc_poly, n_info))) { free(mask); return rc; }
    if (n_blocks > 0 && (!keys || !crc || (Nf > 0 && !syndrome))) { free(mask); return prc_null(who, !keys ? "keys" : (!crc ? "crc" : "syndrome")); }
    int *fpos = (int *)malloc(sizeof(int) * (size_t)(Nf > 0 ? Nf : 1));
    uint32_t *rows = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)(W + Wi));
    if (!fpos || !rows) { free(fpos); free(rows); free(mask); return QLDPC_ENOMEM; }
    uint32_t *urow = rows, *irow = rows + W;
    prc_tables(log2_n, mask, NULL, fpos);
    for (long f = 0; f < n_blocks; f++) {
        const int kb = prc_key_bits(key_bits ? key_bits[f] : (int)N, log2_n);
        for (long w = 0; w < W; w++) urow[w] = keys[f * W + w] & prc_key_mask(kb, (uint32_t)w);
        qldpc_polar_encode_host(log2_n, 1, urow, urow);
        for (long j = 0; j < Wf; j++) syndrome[f * Wf + j] = prc_gather_word(urow, fpos, (int)Nf, (size_t)j);
        for (long j = 0; j < Wi; j++) irow[j] = prc_gather_word(urow, info_pos, n_info, (size_t)j);
        crc[f] = prc_row_crc(irow, n_info, crc_len, crc_poly);
    }
    free(fpos); free(rows); free(mask);
    return QLDPC_OK;
}

/* the prior of blocks [0, n) with the code's tables: the loop both mirrors below run */
static void prc_prior_rows(int log2_n, const uint32_t *mask, const int *prefix, int i8, int pi, int qi, float pf, float qf, long n, const uint32_t *keys,
                           const int *key_bits, const uint32_t *syndrome, long Wf, void *llr, uint32_t *frozen)
{
    const long N = 1l << log2_n, W = pl_words(log2_n);
    for (long f = 0; f < n; f++) {
        const int kb = prc_key_bits(key_bits ? key_bits[f] : (int)N, log2_n);
        for (long i = 0; i < N; i++) {
            const unsigned bit = pl_bit(keys[f * W + (i >> 5)], (int)(i & 31));
            if (i8) ((int8_t *)llr)[f * N + i] = (int8_t)PRC_LEVEL(i, bit, kb, pi, qi);
            else ((float *)llr)[f * N + i] = PRC_LEVEL(i, bit, kb, pf, qf);
        }
        for (long w = 0; w < W; w++) frozen[f * W + w] = prc_frozen_bits(syndrome ? syndrome + f * Wf : NULL, mask[w], (uint32_t)prefix[w], 0, 32);
    }
}

int qldpc_polar_recon_prior_host(int log2_n, int n_info, const int *info_pos, int messages, int maxq, double prior, double pin, int n_blocks,
                                 const uint32_t *keys, const int *key_bits, const uint32_t *syndrome, void *llr, uint32_t *frozen)
{
    const char *who = "polar_recon_prior_host";
    uint32_t *mask = NULL;
    int pi, qi;
    float pf, qf;
    int rc = pl_args_scalars(who, log2_n, PL_MAX_LOG2N, messages, maxq);
    if (!rc) rc = prc_args_levels(who, messages, maxq, prior, pin, &pi, &qi, &pf, &qf);
    if (!rc) rc = prc_args_count(who, n_blocks);
    if (rc) return rc;
    if ((rc = pl_args_frozen_mask(who, log2_n, n_info, info_pos, &mask))) return rc;
    const long N = 1l << log2_n, W = pl_words(log2_n), Nf = N - n_info;
    if (n_blocks > 0 && (!keys || !llr || !frozen || (Nf > 0 && !syndrome))) {
        free(mask);
        return prc_null(who, !keys ? "keys" : (!llr ? "llr" : (!frozen ? "frozen" : "syndrome")));
    }
    int *prefix = (int *)malloc(sizeof(int) * (size_t)W);
    if (!prefix) { free(mask); return QLDPC_ENOMEM; }
    prc_tables(log2_n, mask, prefix, NULL);
    prc_prior_rows(log2_n, mask, prefix, messages == QLDPC_POLAR_I8, pi, qi, pf, qf, n_blocks, keys, key_bits, syndrome, pmc_words((int)Nf), llr, frozen);
    free(prefix); free(mask);
    return QLDPC_OK;
}

/* the checks of a verdict call, the device's too: the size, n_info, the CRC where no pick decides, and the pointers */
int prc_args_verdict(const char *who, int log2_n, int n_info, int crc_len, uint32_t crc_poly, int n_blocks, const void *info, const void *x, const void *pick,
                     const void *keys, const void *crc, const void *status)
{
    if (pl_check_size(log2_n, PL_MAX_LOG2N)) { qldpc_set_error("%s: log2_n=%d (1 .. %d)", who, log2_n, PL_MAX_LOG2N); return QLDPC_ESIZE; }
    if (n_info < 0 || n_info > (1l << log2_n)) { qldpc_set_error("%s: n_info=%d (0 .. N = %ld)", who, n_info, 1l << log2_n); return QLDPC_ESIZE; }
    int rc = prc_args_count(who, n_blocks);
    if (!rc && !pick) rc = prc_args_crc(who, crc_len, crc_poly, n_info);
    if (rc || n_blocks == 0) return rc;
    if (!x || !keys || !status) return prc_null(who, !x ? "x" : (!keys ? "keys" : "status"));
    if (!pick && (!info || !crc)) return prc_null(who, !info ? "info" : "crc");
    return QLDPC_OK;
}

int qldpc_polar_recon_verdict_host(int log2_n, int n_info, int crc_len, uint32_t crc_poly, int n_blocks, const uint32_t *info, const uint32_t *x,
                                   const int32_t *pick, uint32_t *keys, const int *key_bits, const uint32_t *crc, int *status, int *corrected)
{
    const int rc = prc_args_verdict("polar_recon_verdict_host", log2_n, n_info, crc_len, crc_poly, n_blocks, info, x, pick, keys, crc, status);
    if (rc) return rc;
    const long N = 1l << log2_n, W = pl_words(log2_n), Wi = pmc_words(n_info);
    for (long f = 0; f < n_blocks; f++) {
        int co;
        prc_verdict_block(log2_n, n_info, crc_len, crc_poly, info ? info + f * Wi : NULL, x + f * W, pick != NULL, pick ? pick[f] : 0, keys + f * W,
                          key_bits ? key_bits[f] : (int)N, crc ? crc[f] : 0u, &status[f], &co);
        if (corrected) corrected[f] = co;
    }
    return QLDPC_OK;
}

#define PRC_HOST_CHUNK 256         /* blocks whose LLR rows the decode mirror holds at a time */

int qldpc_polar_recon_decode_host(int log2_n, int n_info, const int *info_pos, int messages, int maxq, int form, int rule, int list_size, int crc_len,
                                  uint32_t crc_poly, double prior, double pin, int n_blocks, uint32_t *keys, const int *key_bits, const uint32_t *syndrome,
                                  const uint32_t *crc, int *status, int *corrected, int32_t *pick)
{
    const char *who = "polar_recon_decode_host";
    uint32_t *mask = NULL;
    int pi, qi;
    float pf, qf;
    int rc = pl_args_scalars(who, log2_n, list_size ? PLL_MAX_LOG2N : PL_MAX_LOG2N, messages, maxq);
    if (!rc) rc = prc_args_levels(who, messages, maxq, prior, pin, &pi, &qi, &pf, &qf);
    if (!rc) rc = prc_args_count(who, n_blocks);
    if (rc) return rc;
    if (list_size) {
        if (pll_check_list(list_size)) { qldpc_set_error("%s: list_size=%d (0: SC, or 1, 2, 4, 8)", who, list_size); return QLDPC_ESIZE; }
        if (form != QLDPC_POLAR_LANES || rule != QLDPC_POLAR_SC) { qldpc_set_error("%s: the list decoder has neither forms nor rules (form = rule = 0)", who); return QLDPC_EINVAL; }
    } else {
        if (form != QLDPC_POLAR_LANES && form != QLDPC_POLAR_WIDE) { qldpc_set_error("%s: form=%d (QLDPC_POLAR_LANES or QLDPC_POLAR_WIDE)", who, form); return QLDPC_EINVAL; }
        if (rule != QLDPC_POLAR_SC && rule != QLDPC_POLAR_SSC) { qldpc_set_error("%s: rule=%d (QLDPC_POLAR_SC or QLDPC_POLAR_SSC)", who, rule); return QLDPC_EINVAL; }
        if (rule == QLDPC_POLAR_SSC && form == QLDPC_POLAR_WIDE && log2_n > PL_SUB_LOG) {
            qldpc_set_error("%s: the SSC rule has no wide form", who);
            return QLDPC_EUNSUPPORTED;
        }
        if (pick) { qldpc_set_error("%s: pick is the list decoder's (list_size = 0 is SC)", who); return QLDPC_EINVAL; }
    }
    if ((rc = pl_args_frozen_mask(who, log2_n, n_info, info_pos, &mask))) return rc;
    const long N = 1l << log2_n, W = pl_words(log2_n), Nf = N - n_info, Wf = pmc_words((int)Nf), Wi = pmc_words(n_info);
    if ((rc = prc_args_crc(who, crc_len, crc_poly, n_info))) { free(mask); return rc; }
    if (n_blocks > 0 && (!keys || !crc || !status || (Nf > 0 && !syndrome))) {
        free(mask);
        return prc_null(who, !keys ? "keys" : (!crc ? "crc" : (!status ? "status" : "syndrome")));
    }
    const size_t C = PRC_HOST_CHUNK, esz = messages == QLDPC_POLAR_I8 ? 1 : sizeof(float);
    int *prefix = (int *)malloc(sizeof(int) * (size_t)W);
    void *llr = malloc(esz * C * (size_t)N);
    uint32_t *rows = (uint32_t *)malloc(sizeof(uint32_t) * C * (size_t)(2 * W + Wi + 1));
    int32_t *pk = (int32_t *)malloc(sizeof(int32_t) * C);
    if (!prefix || !llr || !rows || !pk) rc = QLDPC_ENOMEM;
    uint32_t *frozen = rows, *xh = rows ? rows + C * (size_t)W : NULL, *ih = rows ? xh + C * (size_t)W : NULL;
    if (!rc) prc_tables(log2_n, mask, prefix, NULL);
    for (long f0 = 0; f0 < n_blocks && !rc; f0 += (long)C) {
        const int nb = (int)(n_blocks - f0 < (long)C ? n_blocks - f0 : (long)C);
        const int *kbs = key_bits ? key_bits + f0 : NULL;
        prc_prior_rows(log2_n, mask, prefix, messages == QLDPC_POLAR_I8, pi, qi, pf, qf, nb, keys + f0 * W, kbs, syndrome ? syndrome + f0 * Wf : NULL, Wf, llr, frozen);
        if (list_size)
            rc = qldpc_polar_list_decode_host(log2_n, n_info, info_pos, messages, maxq, list_size, crc_len, crc_poly, nb, llr, frozen, crc + f0, NULL, ih, xh, pk, NULL, NULL);
        else if (rule == QLDPC_POLAR_SSC)
            rc = qldpc_polar_decode_ssc_host(log2_n, n_info, info_pos, messages, maxq, nb, llr, frozen, NULL, ih, xh);
        else if (form == QLDPC_POLAR_WIDE)
            rc = qldpc_polar_decode_wide_host(log2_n, n_info, info_pos, messages, maxq, nb, llr, frozen, NULL, ih, xh, NULL);
        else
            rc = qldpc_polar_decode_host(log2_n, n_info, info_pos, messages, maxq, nb, llr, frozen, NULL, ih, xh, NULL);
        if (rc) break;
        rc = qldpc_polar_recon_verdict_host(log2_n, n_info, crc_len, crc_poly, nb, ih, xh, list_size ? pk : NULL, keys + f0 * W, kbs, crc + f0, status + f0,
                                            corrected ? corrected + f0 : NULL);
        if (!rc && pick) memcpy(pick + f0, pk, sizeof(int32_t) * (size_t)nb);
    }
    free(prefix); free(llr); free(rows); free(pk); free(mask);
    return rc;
}
