/*
 * qldpc_polar_mc_host.c -- the host side of the Monte-Carlo loop around the polar decoders: the mirror of its frames (qldpc_polar_mc_frames_host),
 * plain C over the functions of qldpc_polar_mc_core.h that the kernels of qldpc_kernels_polar_mc.h run per lane, here in a loop over frames, words
 * and quads; the table builder of the quantised AWGN channel in the two roundings of the reference's scripts (qldpc_polar_mc_awgn_table); and the
 * argument checks that the mirror and the device object (qldpc_polar_mc.hip) share, worded once (qldpc_polar_int.h).  No device.
 */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "qldpc_polar_int.h"
#include "qldpc_polar_mc_core.h"

int pmc_args_modes(const char *who, int frozen_mode, int source_mode)
{
    if (frozen_mode != QLDPC_POLAR_MC_FROZEN_ZERO && frozen_mode != QLDPC_POLAR_MC_FROZEN_RANDOM) {
        qldpc_set_error("%s: frozen_mode=%d (QLDPC_POLAR_MC_FROZEN_ZERO or QLDPC_POLAR_MC_FROZEN_RANDOM)", who, frozen_mode);
        return QLDPC_EINVAL;
    }
    if (source_mode != QLDPC_MC_SOURCE_RANDOM && source_mode != QLDPC_MC_SOURCE_ZERO) {
        qldpc_set_error("%s: source mode=%d (QLDPC_MC_SOURCE_RANDOM or QLDPC_MC_SOURCE_ZERO)", who, source_mode);
        return QLDPC_EINVAL;
    }
    return QLDPC_OK;
}

int pmc_args_table(const char *who, int messages, int levels, const uint64_t *cum0, const uint64_t *cum1, const float *value, mc_soft_table *t)
{
    const int rc = pmc_table_build(messages == QLDPC_POLAR_I8, levels, cum0, cum1, value, t);
    if (rc == -1) { qldpc_set_error("%s: levels=%d outside 2 .. %d", who, levels, MC_SOFT_MAX_LEVELS); return QLDPC_ESIZE; }
    if (rc == -2) { qldpc_set_error("%s: a missing array, a row that decreases or an entry above 2^32", who); return QLDPC_EINVAL; }
    if (rc) { qldpc_set_error("%s: with QLDPC_POLAR_I8 messages every value must be an integer in [-128, 127]", who); return QLDPC_EINVAL; }
    return QLDPC_OK;
}

int qldpc_polar_mc_awgn_table(double sigma, double rmax, int maxq, int rounding, uint64_t *cum0, uint64_t *cum1, float *value)
{
    if (rounding != 0 && rounding != 1) { qldpc_set_error("polar_mc_awgn_table: rounding=%d (0: floor, 1: round)", rounding); return QLDPC_EINVAL; }
    if (rounding == 0) {
        const int rc = qldpc_mc_awgn_table(sigma, rmax, maxq, cum0, cum1, value);
        return rc ? rc : 2 * maxq + 2;
    }
    if (!(sigma > 0.0 && sigma < INFINITY) || !(rmax > 0.0 && rmax < INFINITY) || maxq < 1 || 2 * maxq + 1 > MC_SOFT_MAX_LEVELS) {
        qldpc_set_error("polar_mc_awgn_table: sigma=%g rmax=%g (positive, finite), maxq=%d (1 .. %d with rounding = 1)", sigma, rmax, maxq, (MC_SOFT_MAX_LEVELS - 1) / 2);
        return QLDPC_ESIZE;
    }
    if (!cum0 || !cum1 || !value) return QLDPC_EINVAL;
    const int Q = 2 * maxq + 1;
    uint64_t *cum[2] = {cum0, cum1};
    for (int b = 0; b < 2; b++)
        for (int k = 0; k < Q - 1; k++) {      /* the same Phi as qldpc_mc_awgn_table, at the boundaries of round() */
            const double boundary = ((double)(k - maxq) + 0.5) * rmax / (double)maxq, x = (boundary - (double)(1 - 2 * b)) / sigma;
            cum[b][k] = (uint64_t)floor(4294967296.0 * (0.5 * erfc(-x / sqrt(2.0))));
        }
    for (int l = 0; l < Q; l++) value[l] = (float)(l - maxq);
    return Q;
}

int qldpc_polar_mc_frames_host(int log2_n, int n_info, const int *info_pos, int messages, int crc_len, uint32_t crc_poly, int frozen_mode, int source_mode,
                               uint64_t seed, int levels, const uint64_t *cum0, const uint64_t *cum1, const float *value, uint64_t first_frame,
                               int n_frames, uint32_t *info, uint32_t *u, uint32_t *x, void *llr, uint32_t *flips)
{
    const char *who = "polar_mc_frames_host";
    uint32_t *mask = NULL;
    int rc = pl_args_scalars(who, log2_n, PL_MAX_LOG2N, messages, 1);
    if (!rc) rc = pmc_args_modes(who, frozen_mode, source_mode);
    if (rc) return rc;
    if (n_frames < 0) { qldpc_set_error("%s: n_frames=%d is negative", who, n_frames); return QLDPC_EINVAL; }
    rc = pl_args_frozen_mask(who, log2_n, n_info, info_pos, &mask);
    if (rc) return rc;
    if (pll_check_crc(crc_len, crc_poly, n_info)) {
        qldpc_set_error("%s: crc_len=%d, crc_poly=0x%x, n_info=%d (crc_len 0 .. 32 and at most n_info; crc_poly holds the low crc_len coefficients, x^crc_len is implied)",
                        who, crc_len, (unsigned)crc_poly, n_info);
        free(mask);
        return QLDPC_ESIZE;
    }
    mc_soft_table *t = NULL;
    if (llr || flips) {
        if (levels == 0) { qldpc_set_error("%s: llr or flips without a table (levels = 0)", who); free(mask); return QLDPC_ESTATE; }
        t = (mc_soft_table *)malloc(sizeof(*t));
        if (!t) { free(mask); return QLDPC_ENOMEM; }
        if ((rc = pmc_args_table(who, messages, levels, cum0, cum1, value, t))) { free(t); free(mask); return rc; }
    }
    const int A = n_info - crc_len;
    const long N = 1l << log2_n, W = pl_words(log2_n), Wa = pmc_words(A), Wi = pmc_words(n_info);
    int *rank = (int *)malloc(sizeof(int) * 32 * (size_t)W);
    uint32_t *rows = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)(Wi + 2 * W));
    if (!rank || !rows) { free(rank); free(rows); free(t); free(mask); return QLDPC_ENOMEM; }
    uint32_t *irow = rows, *urow = rows + Wi, *xrow = urow + W;
    pmc_rank(log2_n, n_info, info_pos, rank);
    const uint32_t quads = pmc_quads(log2_n), valid = pmc_quad_valid(log2_n);
    for (long f = 0; f < n_frames; f++) {
        const uint64_t frame = first_frame + (uint64_t)f;
        uint32_t r = 0u;
        for (long j = 0; j < Wa && crc_len; j++) r = pmc_crc_word(r, pmc_msg_word(seed, frame, (uint32_t)j, A, source_mode), pmc_msg_bits((uint32_t)j, A), crc_len, crc_poly);
        for (long j = 0; j < Wi; j++) irow[j] = pmc_info_word(j < Wa ? pmc_msg_word(seed, frame, (uint32_t)j, A, source_mode) : 0u, (uint32_t)j, A, crc_len, r);
        for (long w = 0; w < W; w++)
            urow[w] = pmc_u_word(irow, rank + 32 * w, frozen_mode == PMC_FROZEN_RANDOM ? pmc_frozen_word(seed, frame, (uint32_t)w) & mask[w] : 0u);
        if (info && Wi) memcpy(info + f * Wi, irow, sizeof(uint32_t) * (size_t)Wi);
        if (u) memcpy(u + f * W, urow, sizeof(uint32_t) * (size_t)W);
        if (!x && !t) continue;
        qldpc_polar_encode_host(log2_n, 1, urow, xrow);
        if (x) memcpy(x + f * W, xrow, sizeof(uint32_t) * (size_t)W);
        if (!t) continue;
        uint32_t fl = 0u;
        for (uint32_t q = 0; q < quads; q++) {
            float l[4];
            fl += pmc_quad(seed, frame, q, pmc_quad_bits(xrow, q), valid, t->thr[0], t->live[0], t->thr[1], t->live[1], t->value, l);
            for (uint32_t b = 0; b < valid && llr; b++) {
                if (messages == QLDPC_POLAR_I8) ((int8_t *)llr)[f * N + 4 * (long)q + b] = (int8_t)pmc_i8(l[b]);
                else ((float *)llr)[f * N + 4 * (long)q + b] = l[b];
            }
        }
        if (flips) flips[f] = fl;
    }
    free(rank); free(rows); free(t); free(mask);
    return QLDPC_OK;
}
