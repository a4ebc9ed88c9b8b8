/*
 * qldpc_recon_guess_host.c -- the host mirror of the verdict of a guessing round inside a session (rk_guess_crc + rk_guess_settle of
 * qldpc_kernels_recon_guess.h) that needs no device: the same functions of qldpc_recon_guess_core.h, and the serial CRC-32 of qldpc_recon_core.h
 * (what qldpc_crc32_words computes) in place of the chunked fold.
 */
#include <string.h>

#include "../../include/qldpc.h"
#include "qldpc_graph.h"
#include "qldpc_recon_guess_core.h"

int qldpc_recon_guess_settle_host(int g, int n_src, int Wk, int Wn, const uint32_t *trial_rows, const int *ok, const int *iters, const uint32_t *keys,
                                  const int *key_bits, const uint32_t *crc_want, const int *first_iters, int *pass_out, uint32_t *crc_out, uint32_t *res_keys,
                                  int *res, int *guess)
{
    if (!trial_rows || !ok || !iters || !keys || !key_bits || !crc_want || !first_iters || !pass_out || !crc_out || !res_keys || !res || !guess) return QLDPC_EINVAL;
    if (g < 0 || g > GS_MAX_BITS || n_src < 0 || Wk < 1 || Wn < Wk || ((uint64_t)n_src << g) > GS_MAX_SLOTS) {
        qldpc_set_error("recon_guess_settle_host: guess bits=%d (0 .. %d), n_src=%d (not negative, n_src 2^g <= %u), key row of %d words (at least 1) in trial rows of %d",
                        g, GS_MAX_BITS, n_src, GS_MAX_SLOTS, Wk, Wn);
        return QLDPC_ESIZE;
    }
    for (int s = 0; s < n_src; s++)
        if (key_bits[s] < 1 || key_bits[s] > 32 * Wk) {
            qldpc_set_error("recon_guess_settle_host: source %d has key_bits=%d, outside 1 .. %d (key rows of %d words)", s, key_bits[s], 32 * Wk, Wk);
            return QLDPC_ESIZE;
        }
    uint32_t table[256];
    for (uint32_t i = 0; i < 256; i++) table[i] = crc_table_entry(i);
    const size_t T = (size_t)1 << g;
    for (int s = 0; s < n_src; s++) {
        const int kb = key_bits[s], nw = (kb + 31) / 32;
        const uint32_t *rows = trial_rows + (size_t)s * T * (size_t)Wn, *old = keys + (size_t)s * Wk;
        const int *f_ok = ok + (size_t)s * T, *f_it = iters + (size_t)s * T;
        int *f_pass = pass_out + (size_t)s * T;
        uint32_t *f_crc = crc_out + (size_t)s * T, *dst = res_keys + (size_t)s * Wk;
        int best = -1, n_ok = 0, n_pass = 0, amb = 0, it_sum = 0, flips = 0;
        for (size_t t = 0; t < T; t++) {
            f_crc[t] = crc_serial(rows + t * (size_t)Wn, kb, table);
            f_pass[t] = rg_pass(f_ok[t], f_crc[t], crc_want[s]);
            best = gs_better(best, (int)t, f_pass[t]);
            n_ok += f_ok[t] != 0; n_pass += f_pass[t]; it_sum += f_it[t];
        }
        if (best >= 0) {
            const uint32_t *win = rows + (size_t)best * Wn;
            for (size_t t = 0; t < T; t++) {
                if (!f_pass[t] || (int)t == best) continue;
                for (int w = 0; w < nw; w++) amb |= rg_differs(rows[t * (size_t)Wn + w], win[w], w, kb);
            }
            for (int i = 0; i < nw; i++) {
                const uint32_t m = tail_mask(i, nw, kb), x = win[i] & m;
                flips += (int)gs_popc((old[i] & m) ^ x);
                dst[i] = x;
            }
        } else
            memcpy(dst, old, sizeof(uint32_t) * (size_t)nw);
        res[s] = best >= 0 ? QLDPC_OK : QLDPC_EDECODE;
        res[(size_t)n_src + s] = best >= 0 ? flips : 0;
        res[2 * (size_t)n_src + s] = rg_iterations(first_iters[s], best, best >= 0 ? f_it[best] : 0);
        res[3 * (size_t)n_src + s] = (int)f_crc[best >= 0 ? best : 0];
        int *gr = guess + (size_t)s * RG_FIELDS;
        gr[0] = 1; gr[1] = best; gr[2] = n_ok; gr[3] = n_pass; gr[4] = amb; gr[5] = it_sum;
    }
    return QLDPC_OK;
}
