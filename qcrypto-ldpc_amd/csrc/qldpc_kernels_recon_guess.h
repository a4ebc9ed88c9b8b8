/*
 * qldpc_kernels_recon_guess.h -- the kernels of a guessing round inside a reconciliation session (qldpc_recon_decode_guess, qldpc_recon_guess_settle_dev).
 * The verdict is stated in qldpc_recon_guess_core.h; these lanes and the host mirror call the same functions.  Included by qldpc_recon.hip after
 * rk_block_crc.  No atomics anywhere: every output word has one writer.
 *
 * rk_guess_cand: the candidate rows of the weakest-VN select of a job that had a failure.
 * rk_guess_capture: after the first decode of a job, one workgroup per block.  A block that failed takes the pool slot base + (the failed blocks of the
 *     job before it) and copies what its trials need, device to device: guess row, hard row, frame bits, erase row, the key handed in and its scalars.
 * rk_guess_sources: a trial launch of n_src sources.  The frame rows of a source are replicated onto its T slots, [n_src][Wn] -> [n_src T][Wn]: a lane
 *     loads a source word once and stores it to the trials of its slice (blockIdx.z deals the trials), one plain 4-byte store per lane and trial, 1 KiB
 *     contiguous per workgroup.  The workgroups of the first column write the |LLR| and key_bits of the slots as well.
 * rk_guess_crc: grid (n_src, T).  rk_block_crc over a trial's decoded row, the source's key_bits: pass(t) and the CRC.
 * rk_guess_settle: one workgroup per source, the structure of qk_guess_pick.  The T pass / ok flags and iteration counts a trip of RK_LANES at a time:
 *     every wave ballots its flags and sums its counts by shuffles, the lowest set bit, the popcounts and the sums per wave go through LDS and every lane
 *     folds them.  Then the waves deal the trials among them: a wave compares the key words of a passing trial with the winner's (tail masked).  Last
 *     the block's result is written as rk_verify writes it -- status, flips, iterations, CRC and key words, the key handed in without a winner -- and
 *     the six ints of its qldpc_recon_guess.
 */
#ifndef QLDPC_KERNELS_RECON_GUESS_H
#define QLDPC_KERNELS_RECON_GUESS_H

#include "qldpc_recon_guess_core.h"

#define RG_WAVES (RK_LANES / 64)

/* key_bits as the kernels use it: nothing is read past a key row whatever the column holds */
__device__ static inline int rg_key_bits(int kb, int Wk) { return min(max(kb, 0), 32 * Wk); }

/* the candidates of the select after a first decode, cand [n][Wn]: the key positions below the block's length (job_load_blind's row with nothing known) */
static __global__ __launch_bounds__(RK_LANES) void rk_guess_cand(const int *__restrict__ key_bits, uint32_t *__restrict__ cand, int Wk, int Wn)
{
    const int b = (int)blockIdx.y, w = (int)(blockIdx.x * RK_LANES + threadIdx.x);
    if (w >= Wn) return;
    const int kb = rg_key_bits(key_bits[b], Wk), nw = (kb + 31) / 32;
    cand[(size_t)b * Wn + w] = w < nw ? tail_mask(w, nw, kb) : 0u;
}

static __global__ __launch_bounds__(RK_LANES) void rk_guess_capture(const int *__restrict__ status, const int *__restrict__ iters, const uint32_t *__restrict__ weak,
                                                                    const uint32_t *__restrict__ hard, const uint32_t *__restrict__ bits,
                                                                    const uint32_t *__restrict__ erase, recon_in_view in, recon_guess_pool_view pool, int base,
                                                                    int cap, int Wk, int Wn)
{
    const int b = (int)blockIdx.x, t0 = (int)threadIdx.x;
    if (status[b] == QLDPC_OK) return;      /* uniform per workgroup */
    int rank = 0;
    for (int t = 0; t < b; t++) rank += status[t] != QLDPC_OK;
    const int slot = base + rank;
    if (slot >= cap) return;
    const size_t src = (size_t)b * Wn, dst = (size_t)slot * Wn;
    for (int w = t0; w < Wn; w += RK_LANES) {
        pool.weak[dst + w] = weak[src + w];
        pool.hard[dst + w] = hard[src + w];
        pool.bits[dst + w] = bits[src + w];
        pool.erase[dst + w] = erase[src + w];
    }
    const int kb = rg_key_bits(in.key_bits[b], Wk), nw = (kb + 31) / 32;
    for (int w = t0; w < nw; w += RK_LANES) pool.keys[(size_t)slot * Wk + w] = in.keys[(size_t)b * Wk + w];
    if (t0 == 0) { pool.mag[slot] = in.mag[b]; pool.key_bits[slot] = in.key_bits[b]; pool.crc[slot] = in.crc[b]; pool.iters[slot] = iters[b]; }
}

/* bits, erase [n_src][Wn], mag, key_bits [n_src] -> t_bits, t_erase [n_src T][Wn], t_mag, t_key_bits [n_src T] */
static __global__ __launch_bounds__(RK_LANES) void rk_guess_sources(const uint32_t *__restrict__ bits, const uint32_t *__restrict__ erase, const float *__restrict__ mag,
                                                                    const int *__restrict__ key_bits, uint32_t *__restrict__ t_bits, uint32_t *__restrict__ t_erase,
                                                                    float *__restrict__ t_mag, int *__restrict__ t_key_bits, int Wn, int g)
{
    const unsigned T = 1u << g;
    const size_t s = blockIdx.y;
    const int w = (int)(blockIdx.x * RK_LANES + threadIdx.x);
    if (w < Wn) {
        const uint32_t x = bits[s * (size_t)Wn + w], er = erase[s * (size_t)Wn + w];
        for (unsigned t = blockIdx.z; t < T; t += gridDim.z) {
            const size_t dst = (s * T + t) * (size_t)Wn + (size_t)w;
            t_bits[dst] = x;
            t_erase[dst] = er;
        }
    }
    if (blockIdx.x == 0 && blockIdx.z == 0) {
        const float m = mag[s];
        const int kb = key_bits[s];
        for (unsigned t = threadIdx.x; t < T; t += RK_LANES) { t_mag[s * T + t] = m; t_key_bits[s * T + t] = kb; }
    }
}

/* rows [n_src T][Wn], ok [n_src T]; key_bits, crc_want [n_src] -> pass, crc [n_src T] */
static __global__ __launch_bounds__(RK_LANES) void rk_guess_crc(const uint32_t *__restrict__ rows, const int *__restrict__ ok, const int *__restrict__ key_bits,
                                                                const uint32_t *__restrict__ crc_want, int *__restrict__ pass, uint32_t *__restrict__ crc_out,
                                                                int Wk, int Wn)
{
    __shared__ uint32_t s_tab[256], s_reg[RK_LANES];
    __shared__ int s_cnt[RK_LANES];
    const size_t s = blockIdx.x, trial = s * gridDim.y + blockIdx.y;
    const uint32_t crc = rk_block_crc(rows + trial * (size_t)Wn, rg_key_bits(key_bits[s], Wk), nullptr, nullptr, nullptr, s_tab, s_reg, s_cnt);
    if (threadIdx.x == 0) { crc_out[trial] = crc; pass[trial] = rg_pass(ok[trial], crc, crc_want[s]); }
}

/* rows, ok, pass, crc, iters per trial; keys [n_src][Wk], key_bits, first_iters [n_src] -> res_keys [n_src][Wk], the four result columns res + k res_stride
 * (status, flips, iterations, CRC: recon_bob_layout), guess [n_src][RG_FIELDS] */
static __global__ __launch_bounds__(RK_LANES) void rk_guess_settle(const uint32_t *__restrict__ rows, const int *__restrict__ ok, const int *__restrict__ pass,
                                                                   const uint32_t *__restrict__ crc, const int *__restrict__ iters, const uint32_t *__restrict__ keys,
                                                                   const int *__restrict__ key_bits, const int *__restrict__ first_iters,
                                                                   uint32_t *__restrict__ res_keys, int *__restrict__ res, int res_stride, int *__restrict__ guess,
                                                                   int Wk, int Wn, int g)
{
    __shared__ int s_first[RG_WAVES], s_pass[RG_WAVES], s_ok[RG_WAVES], s_it[RG_WAVES], s_amb, s_cnt[RK_LANES];
    const unsigned t0 = threadIdx.x, lane = t0 & 63u, wave = t0 >> 6, T = 1u << g;
    const size_t s = blockIdx.x;
    const int kb = rg_key_bits(key_bits[s], Wk), nw = (kb + 31) / 32;
    const int *f_ok = ok + s * T, *f_pass = pass + s * T, *f_it = iters + s * T;
    const uint32_t *trial_rows = rows + s * T * (size_t)Wn;
    int best = -1, n_ok = 0, n_pass = 0, it_sum = 0;
    if (t0 == 0) s_amb = 0;
    for (unsigned base = 0; base < T; base += RK_LANES) {      /* T is uniform: every lane takes every trip */
        const unsigned t = base + t0, tc = min(t, T - 1u);
        const unsigned long long mp = __ballot(t < T && f_pass[tc] != 0), mo = __ballot(t < T && f_ok[tc] != 0);
        int it = t < T ? f_it[tc] : 0;
        for (int d = 32; d; d >>= 1) it += __shfl_down(it, d, 64);
        if (lane == 0) {
            s_first[wave] = mp ? (int)(base + wave * 64u) + __ffsll((long long)mp) - 1 : -1;
            s_pass[wave] = __popcll(mp); s_ok[wave] = __popcll(mo); s_it[wave] = it;
        }
        __syncthreads();
        for (unsigned k = 0; k < RG_WAVES; k++) { best = gs_better(best, s_first[k], s_first[k] >= 0); n_pass += s_pass[k]; n_ok += s_ok[k]; it_sum += s_it[k]; }
        __syncthreads();
    }
    const uint32_t *old = keys + s * (size_t)Wk;
    uint32_t *dst = res_keys + s * (size_t)Wk;
    int flips = 0;
    if (best >= 0) {      /* uniform per workgroup */
        const uint32_t *win = trial_rows + (size_t)best * Wn;
        for (unsigned t = wave; t < T; t += RG_WAVES) {      /* t is wave-uniform */
            if (t == (unsigned)best || f_pass[t] == 0) continue;
            int differs = 0;
            for (int w = (int)lane; w < nw; w += 64) differs |= rg_differs(trial_rows[(size_t)t * Wn + w], win[w], w, kb);
            if (__any(differs) && lane == 0) s_amb = 1;
        }
        for (int i = (int)t0; i < nw; i += RK_LANES) {
            const uint32_t m = tail_mask(i, nw, kb), x = win[i] & m;
            flips += __popc((old[i] & m) ^ x);
            dst[i] = x;
        }
    } else
        for (int i = (int)t0; i < nw; i += RK_LANES) dst[i] = old[i];
    s_cnt[t0] = flips;
    __syncthreads();
    for (int st = 1; st < RK_LANES; st <<= 1) {
        if ((t0 & (2 * st - 1)) == 0) s_cnt[t0] += s_cnt[t0 + st];
        __syncthreads();
    }
    if (t0 == 0) {
        res[s] = best >= 0 ? QLDPC_OK : QLDPC_EDECODE;
        res[(size_t)res_stride + s] = best >= 0 ? s_cnt[0] : 0;
        res[2 * (size_t)res_stride + s] = rg_iterations(first_iters[s], best, best >= 0 ? f_it[best] : 0);
        res[3 * (size_t)res_stride + s] = (int)crc[s * T + (size_t)(best >= 0 ? best : 0)];
        int *gr = guess + s * RG_FIELDS;
        gr[0] = 1; gr[1] = best; gr[2] = n_ok; gr[3] = n_pass; gr[4] = s_amb; gr[5] = it_sum;
    }
}

#endif /* QLDPC_KERNELS_RECON_GUESS_H */
