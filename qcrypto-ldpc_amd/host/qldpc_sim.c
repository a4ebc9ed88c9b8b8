/*
 * qldpc_sim.c -- the reference's QKD-over-BSC simulation loop (BS/src/main.cpp:213-409,
 * VAR/main.cpp (dvb-v1.0.2):427-458) written in C against libqldpc's C ABI.
 *
 *   for each BER: pick the code, then per batch of frames
 *     source -> encoder -> BSC(ber) on the key VNs -> LLR = +-ln((1-p)/p)            (main.cpp:340-348)
 *     parity VNs pinned to +-CONFIRMED_BIT_LLR                                        (main.cpp:351-354)
 *     decoder->decode_siho, compare the K info bits, count bit / frame errors         (main.cpp:365-388)
 *   one AFF3CT-style row per BER: FRA | BE | FE | BER | FER | SIM_THR (Mb/s)          (Reporter_BFER/_throughput)
 *
 * usage: qldpc_sim [-N n] [-K k | -a alist | -q qc] [-r MS|OMS|NMS|SPA|LSPA|AMS_MIN|AMS_MINSTAR_L2|AMS_MINSTAR] [-p param]
 *                  [-i n_ite] [-f frames_per_ber] [-b batch] [-s ber_min:ber_max:ber_step] [-S seed] [-l (horizontal layered)] [-v (vertical layered)] [-n (no syndrome)]
 *                  [-P depth (progressive-edge-growth information part instead of the seeded socket shuffle)]
 *                  [-d parity_ber (dirty disclosed parity bits, BS/data_dvb/data5)]
 *                  [-G IDENTITY|LU_DEC|QC (encoder construction: p.G_method / Encoder_LDPC_from_QC)]
 *                  [-R (with -e: report every random pattern -- one per batch -- and keep the best; -o file writes its VN indices)]
 *                  [-Q 32|16|8 (message storage: fp32 = the AFF3CT float build, binary16, 8-bit fixed-point min-sum)]
 *                  [-e f (puncture parity bits to reach the rate min_cr(ber, f); random pattern re-drawn per batch, main.cpp:321-333,359-362)]
 *                  [-D (the loop on the device: qldpc_mc_run generates, encodes, decodes and counts, nothing per bit crosses the host; frames
 *                      [0, frames_per_ber) of seed -S at every BER, so the rows of a table share their random numbers; SIM_THR is the decode
 *                      time by hipEvents; -e and -R are host-only and refused)]
 *                  [-E n (with -D: stop a BER point at the first batch boundary with n frame errors, Monitor_BFER's max_fe)]
 *                  [-X f (with -D: the puncture-pattern search of BS/src/main.cpp:235-411 on the device, qldpc_mc_search: per BER point up to
 *                      frames_per_ber (-f) random patterns of the n_punct parity bits that -e f would puncture, each over -F frames of its own,
 *                      batch / F patterns per decoder launch; stops after the first round that holds a pattern with FER = 0 / F; prints one
 *                      `#   pattern` line per evaluated pattern and the `best of` line of -R; -o file writes the best pattern's VN indices;
 *                      -E does not apply)]
 *                  [-F n (with -X: frames per pattern, default 64)]
 *                  [-A ebno_db[:rmax:maxq] (with -D: BPSK over AWGN quantised to 2 maxq + 2 levels, floor(r / rmax * maxq) clamped to [-maxq - 1, maxq],
 *                      defaults 3 and 31, in place of the BSC -- the experiment of the reference's fixed-point MATLAB sims -- through
 *                      qldpc_mc_set_channel; every VN goes through the channel but the -u first ones; sigma from the rate K / (N - u); one row, with
 *                      Eb/N0 in place of the QBER; -s and -X do not apply)]
 *                  [-T lo:hi:step[:rmax:maxq] (with -D: the Eb/N0 points lo, lo + step, .. <= hi of the channel of -A from ONE qldpc_mc_sweep_tables, a table per
 *                      point, the rows side by side in every batch, in the format of the -A rows; -u and -z as with -A, -E as the stop rule of each
 *                      row; -A, -W, -X, -w and -B do not apply)]
 *                  [-u n (with -A or -T: the first n VNs are punctured, LLR 0: the 2 z of the 5G NR matrices)]
 *                  [-z (with -D: the all-zero codeword instead of random info words, qldpc_mc_set_source)]
 *                  [-W (with -D: the -s table from ONE qldpc_mc_sweep instead of one qldpc_mc_run per row: the rows side by side in every batch,
 *                      -E as the stop rule of each row, the lanes of a finished row passing to the others; with -W, -e f is legal under -D: the
 *                      row at `ber` punctures parity_bits_to_punct(N, K, min_cr(ber, f)) parity VNs, a prefix of ONE order of the parity VNs
 *                      (bit-reversed positions along the accumulator, so that every prefix is evenly spaced, the spacing the sessions use); a row
 *                      whose count is negative is skipped with the harness's message; -X and -A do not apply)]
 *                  [-w lo:hi:step[:design_qber] (with -D: fixed-weight error strata, ONE qldpc_mc_strata over the weights lo, lo + step, .. <= hi: every frame of
 *                      a row flips exactly that many key VNs, the ones with the smallest channel words, and is decoded with |LLR| = ln((1-p)/p) of
 *                      design_qber (default: the first QBER of -s; the letter -q is the QC file); one row per weight with the weight in the EP
 *                      column, -E as the stop rule of each row; then one `# strata ber` line per QBER of the -s table with the four numbers of
 *                      qldpc_mc_strata_fer_host: FER over the simulated weights, the binomial mass below and above them, the standard error;
 *                      -A, -X and -W do not apply)]
 *                  [-B ask:rounds (with -D: blind reconciliation rounds, ONE qldpc_mc_blind per row of -s: a frame whose decode ends with a non-zero syndrome
 *                      asks for its `ask` weakest unknown key VNs, gets Alice's bits there and is decoded again, up to `rounds` times; only the frames
 *                      still open are decoded again, pooled per round.  Per BER one row per round (EP = the round in which those frames closed, `open`
 *                      = still open after the last round) with the key bits those frames asked for in a last column ASKED, then a `# blind` line with
 *                      the sums, the decodes per frame and the efficiency f = (N - K + asked / frames) / (K h2(ber)); -E as the stop rule of the input;
 *                      the decoder is created with compact = 2; -A, -X, -W and -w do not apply)]
 *                  [-G g (a NUMBER, with -D: guessing rounds, ONE qldpc_mc_guess per row of -s: a frame whose decode ends with a non-zero syndrome is
 *                      decoded again with its g weakest key VNs pinned to each of the 2^g possible values and is rescued iff a trial ends with a zero
 *                      syndrome; nothing is disclosed.  Per BER three rows (EP = closed at once / rescued / open) with the undetected errors in a last
 *                      column UNDET, then a `# guess` line with the sums and a `# guess stages` line with the stage times; -E as the stop rule of the
 *                      input; the decoder is created with compact = 2; -A, -X, -W, -w and -B do not apply.  A NAME after -G stays the encoder's method)]
 *                  [-c scale (with -Q 8: quantiser steps per LLR unit, default 8; 1 for LLRs that are integers already, as -A gives them)]
 *                  [-g patience (give a frame up once its syndrome weight has not reached a new minimum for `patience` syndrome tests in a row,
 *                      qldpc_decoder_cfg.giveup_patience; flooding and -l, needs the syndrome test; on the host loop and with -D.  Every row -- with -B
 *                      the `# blind` line -- is followed by a `# given up` line with the frames given up in the decodes of that row.  With -D -B the
 *                      decoder is created with freeze_messages = 1, which the rounds ask for, and the head of the table says so)]
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>
#include <unistd.h>

#include "qldpc.h"

static uint64_t rng_state;
static inline uint64_t rng_next(void)
{
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
static inline double rng_unit(void) { return (double)(rng_next() >> 11) * (1.0 / 9007199254740992.0); }

static double now_s(void)
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

static int die(const char *what, int rc)
{
    fprintf(stderr, "qldpc_sim: %s: %s (%d) %s\n", what, qldpc_strerror(rc), rc, qldpc_last_error());
    return 1;
}
static int usage(const char *msg) { fprintf(stderr, "%s\n", msg); return 2; }

/* the command line (parse); setup() replaces N and K by the code's and the encoder's */
static int N = 8192, K = 6554, n_ite = 50, frames = 256, batch = 256, layered = 0, synd = 1, peg = 0, msg_bits = 32, search = 0, on_device = 0, rule = -1;
static uint64_t max_fe = 0, seed = 0;
static double search_eff = 0.0;      /* -X: > 0 = the pattern search on the device towards this efficiency */
static int frames_per_pattern = 64;
static int awgn = 0, awgn_maxq = 31, awgn_punct = 0, zero_source = 0, sweep = 0;      /* -A, -u, -z, -W */
static double ebno_db = 0.0, awgn_rmax = 3.0, quant_scale = 0.0;
static int tsweep = 0;      /* -T */
static double t_lo = 0.0, t_hi = 0.0, t_step = 0.0;
static int strata = 0, w_lo = 0, w_hi = 0, w_step = 1;      /* -w */
static double design_qber = 0.0;
static int blind = 0, ask_bits = 0, max_rounds = 0;      /* -B */
static int guess = 0, guess_bits = 0;      /* -G with a number */
static int giveup = 0;      /* -g */
static uint64_t gave_before = 0;
static double parity_ber = 0.0;      /* > 0: the disclosed parity bits are themselves wrong with this probability (main.cpp (test effect of dirty parities)) */
static double target_eff = 0.0;      /* > 0: puncture parity bits up to min_cr(ber, f), as BS/src/main.cpp:235-333 does */
static const char *alist = NULL, *qc = NULL, *rule_name = "NMS", *g_method = NULL, *pattern_out = NULL;
static float param = 0.75f;
static double ber_min = 0.01, ber_max = 0.03, ber_step = 0.005;
#define FOR_EACH_BER(ber) for (double ber = ber_min; ber <= ber_max + 1e-12; ber += ber_step)
#define MAX_FRAMES ((uint64_t)(frames > 0 ? frames : 0))

/* what setup() builds; mc only with -D */
static qldpc_code *H; static qldpc_encoder *enc; static qldpc_decoder *dec; static qldpc_mc *mc;
static int *pos; static char *is_info;

/* the result row: EP, already formatted, | FRA | BE | FE | BER | FER | SIM_THR, the last from thr_frames frames decoded in sec seconds */
static void row(const char *ep, uint64_t fra, uint64_t be, uint64_t fe, double thr_frames, double sec)
{
    printf("  %s | %8llu | %8llu | %8llu | %9.2e | %9.2e | %10.3f\n", ep, (unsigned long long)fra, (unsigned long long)be, (unsigned long long)fe,
           (double)be / ((double)fra * K), (double)fe / (double)fra, thr_frames * K / sec / 1e6);
}
static void row_f(double ep, uint64_t fra, uint64_t be, uint64_t fe, double thr_frames, double sec) { char s[64]; snprintf(s, sizeof(s), "%8.4f", ep); row(s, fra, be, fe, thr_frames, sec); }
static void row_d(int ep, uint64_t fra, uint64_t be, uint64_t fe, double thr_frames, double sec) { char s[64]; snprintf(s, sizeof(s), "%8d", ep); row(s, fra, be, fe, thr_frames, sec); }

/* -g: the `# given up` line of a row: the frames given up since the line before */
static int gave_line(double ber)
{
    if (!giveup) return 0;
    uint64_t now = 0;
    const int rc = qldpc_giveup_total(dec, &now);
    if (rc) return die("giveup_total", rc);
    printf("# ber %.4f: given up %llu frames (patience %d)\n", ber, (unsigned long long)(now - gave_before), giveup);
    gave_before = now;
    return 0;
}

/* parity_bits_to_punct(INFO_B, TTL_B, GOAL_CR) with GOAL_CR = min_cr(QBER, EFF) (BS/src/main.cpp:29,34,280), at most all the parity bits, and its
 * lines.  Where the count is negative, the mother code's rate being above the goal already: puncture nothing, or with `skip` return -1. */
static int punct_count(double ber, double eff, int skip)
{
    const int n_par = N - K;
    int n_punct = qldpc_parity_bits_to_punct(N, K, qldpc_min_code_rate((float)ber, (float)eff));
    if (n_punct < 0) printf("# ber %.4f: mother code rate already above the goal, nothing to puncture\n", ber);
    if (n_punct < 0 && skip) return -1;
    n_punct = n_punct < 0 ? 0 : n_punct > n_par ? n_par : n_punct;
    printf("# ber %.4f: puncturing %d of %d parity bits -> rate %.4f, efficiency f = %.3f\n", ber, n_punct, n_par, (double)K / (N - n_punct),
           ((double)(n_par - n_punct) / K) / (double)qldpc_binary_entropy((float)ber));
    return n_punct;
}

static int write_pattern(double ber, int n_punct, const int *vn, long long fe)
{
    FILE *fo = fopen(pattern_out, "w");
    if (!fo) { perror(pattern_out); return 1; }
    fprintf(fo, "# qldpc_sim puncture pattern: N %d K %d ber %.4f punctured %d FE %lld\n", N, K, ber, n_punct, fe);
    for (int i = 0; i < n_punct; i++) fprintf(fo, "%d\n", vn[i]);
    fclose(fo);
    return 0;
}

static int parse(int argc, char **argv)
{
    int opt;
    while ((opt = getopt(argc, argv, "N:K:a:q:r:p:i:f:b:s:S:P:e:d:Q:o:G:E:X:F:A:T:u:c:w:B:g:DRWlvnz")) != -1) {
        switch (opt) {
        case 'N': N = atoi(optarg); break;
        case 'K': K = atoi(optarg); break;
        case 'a': alist = optarg; break;
        case 'q': qc = optarg; break;
        case 'r': rule_name = optarg; break;
        case 'p': param = (float)atof(optarg); break;
        case 'i': n_ite = atoi(optarg); break;
        case 'f': frames = atoi(optarg); break;
        case 'b': batch = atoi(optarg); break;
        case 's': if (sscanf(optarg, "%lf:%lf:%lf", &ber_min, &ber_max, &ber_step) != 3) return usage("-s min:max:step"); break;
        case 'S': seed = strtoull(optarg, NULL, 0); break;
        case 'P': peg = atoi(optarg); break;
        case 'e': target_eff = atof(optarg); break;
        case 'd': parity_ber = atof(optarg); break;
        case 'Q': msg_bits = atoi(optarg); break;
        case 'R': search = 1; break;
        case 'D': on_device = 1; break;
        case 'E': max_fe = strtoull(optarg, NULL, 0); break;
        case 'X': search_eff = atof(optarg); break;
        case 'F': frames_per_pattern = atoi(optarg); break;
        case 'A': { const int got = sscanf(optarg, "%lf:%lf:%d", &ebno_db, &awgn_rmax, &awgn_maxq); if (got != 1 && got != 3) return usage("-A ebno_db[:rmax:maxq]"); awgn = 1; break; }
        case 'T': { const int got = sscanf(optarg, "%lf:%lf:%lf:%lf:%d", &t_lo, &t_hi, &t_step, &awgn_rmax, &awgn_maxq); if (got != 3 && got != 5) return usage("-T lo:hi:step[:rmax:maxq]"); tsweep = 1; break; }
        case 'u': awgn_punct = atoi(optarg); break;
        case 'z': zero_source = 1; break;
        case 'W': sweep = 1; break;
        case 'w': { const int got = sscanf(optarg, "%d:%d:%d:%lf", &w_lo, &w_hi, &w_step, &design_qber); if (got != 3 && got != 4) return usage("-w lo:hi:step[:design_qber]"); strata = 1; break; }
        case 'B': if (sscanf(optarg, "%d:%d", &ask_bits, &max_rounds) != 2) return usage("-B ask:rounds"); blind = 1; break;
        case 'c': quant_scale = atof(optarg); break;
        case 'g': giveup = atoi(optarg); break;
        case 'o': pattern_out = optarg; break;
        case 'G':      /* a number: the guess bits of the guessing rounds; a name: the encoder's method */
            if (optarg[0] >= '0' && optarg[0] <= '9' && optarg[strspn(optarg, "0123456789")] == 0) { guess = 1; guess_bits = atoi(optarg); break; }
            g_method = optarg; break;      /* p.G_method (VAR/main.cpp (alist-v1.0.1):135): IDENTITY | LU_DEC; QC = Encoder_LDPC_from_QC ((qc):145) */
        case 'l': layered = 1; break;
        case 'v': layered = 2; break;      /* Decoder_LDPC_BP_vertical_layered, VAR/main.cpp (alist-v1.0.1):240-256 */
        case 'n': synd = 0; break;
        default: return usage("see the header of qldpc_sim.c for usage");
        }
    }
    static const char *names[] = {"MS", "OMS", "NMS", "SPA", "LSPA", "AMS_MIN", "AMS_MINSTAR_L2", "AMS_MINSTAR"};
    for (int i = 0; i < 8; i++) if (!strcmp(rule_name, names[i])) rule = i;
    if (rule < 0) { fprintf(stderr, "unknown rule %s\n", rule_name); return 2; }
    const int search_x = search_eff != 0.0;
    if (tsweep && !on_device) return usage("qldpc_sim: -T is the Eb/N0 sweep on the device and needs -D");
    if (tsweep && (awgn || sweep || search_x || strata || blind)) return usage("qldpc_sim: -T sweeps Eb/N0 points of the table channel and runs with none of -A, -W, -X, -w and -B");
    if (tsweep && !(t_step > 0.0 && t_lo <= t_hi)) return usage("qldpc_sim: -T lo:hi:step with lo <= hi and step > 0");
    if (sweep && !on_device) return usage("qldpc_sim: -W is the sweep on the device and needs -D");
    if (sweep && (search_x || awgn)) return usage("qldpc_sim: -W sweeps the BSC rows of -s and runs neither with the pattern search (-X) nor with -A");
    if (strata && !on_device) return usage("qldpc_sim: -w runs the error strata on the device and needs -D");
    if (strata && (search_x || awgn || sweep)) return usage("qldpc_sim: -w runs fixed error weights on the BSC's words and runs neither with -X, -A nor -W");
    if (strata && (w_step < 1 || w_lo < 0 || w_hi < w_lo)) return usage("qldpc_sim: -w lo:hi:step with 0 <= lo <= hi and step >= 1");
    if (blind && !on_device) return usage("qldpc_sim: -B runs the blind reconciliation rounds on the device and needs -D");
    if (blind && (search_x || awgn || sweep || strata)) return usage("qldpc_sim: -B runs on the BSC rows of -s and runs neither with -X, -A, -W nor -w");
    if (guess && !on_device) return usage("qldpc_sim: -G g runs the guessing rounds on the device and needs -D");
    if (guess && (search_x || awgn || sweep || strata || blind || tsweep)) return usage("qldpc_sim: -G g runs on the BSC rows of -s and runs neither with -X, -A, -W, -w, -T nor -B");
    if (on_device && ((target_eff > 0.0 && !sweep) || search)) return usage("qldpc_sim: -e and -R draw a puncture pattern per batch on the host and do not run with -D");
    if (max_fe && !on_device) return usage("qldpc_sim: -E needs -D");
    if (search_x && !on_device) return usage("qldpc_sim: -X is the pattern search on the device and needs -D");
    if (search_x && max_fe) return usage("qldpc_sim: -E does not apply to the pattern search (-X), which stops at the first pattern without frame errors");
    if (search_eff < 0.0) return usage("qldpc_sim: -X f with f > 0");
    if ((awgn || zero_source) && !on_device) return usage("qldpc_sim: -A and -z belong to the loop on the device and need -D");
    if (awgn && search_x) return usage("qldpc_sim: -A does not run with the pattern search (-X)");
    if (awgn_punct && !awgn && !tsweep) return usage("qldpc_sim: -u needs -A or -T");
    if (giveup < 0) return usage("qldpc_sim: -g patience with patience >= 1 (0 = off)");
    if (giveup && (!synd || layered == 2)) return usage("qldpc_sim: -g works on the syndrome tests of the flooding and the horizontal-layered (-l) schedule: drop -n / -v");
    return 0;
}

/* code, encoder and decoder, the head of the table, and with -D the loop object */
static int setup(void)
{
    int rc = alist ? qldpc_code_from_alist(alist, &H) : qc ? qldpc_code_from_qc(qc, &H) : peg ? qldpc_code_ira_peg(N, K, 0.125f, 11, 3, peg, 7, &H) : qldpc_code_ira(N, K, 0.125f, 11, 3, 7, &H);
    if (rc) return die("code", rc);
    N = qldpc_code_n(H);
    if ((rc = qldpc_encoder_create(H, g_method ? g_method : qldpc_code_is_ira(H) ? "IRA" : "IDENTITY", 0, &enc))) return die("encoder", rc);
    K = qldpc_encoder_k(enc);
    pos = (int *)malloc(sizeof(int) * (size_t)K);
    qldpc_encoder_info_bits_pos(enc, pos);
    is_info = (char *)calloc((size_t)N, 1);
    for (int i = 0; i < K; i++) is_info[pos[i]] = 1;

    qldpc_decoder_cfg cfg;
    qldpc_decoder_cfg_default(&cfg);
    cfg.schedule = layered == 2 ? QLDPC_SCHED_VLAYERED : (layered ? QLDPC_SCHED_HLAYERED : QLDPC_SCHED_FLOODING);
    cfg.rule = rule; cfg.rule_param = param; cfg.n_ite = n_ite; cfg.enable_syndrome = synd; cfg.syndrome_depth = 1; cfg.max_frames = batch;
    if (msg_bits != 32 && msg_bits != 16 && msg_bits != 8) return usage("-Q 32 | 16 | 8");
    cfg.msg_dtype = msg_bits == 16 ? 1 : (msg_bits == 8 ? 2 : 0);      /* 16: binary16 message storage; 8: fixed-point min-sum */
    cfg.quant_scale = (float)quant_scale;
    if (blind || guess) cfg.compact = 2;      /* the select of the weakest VNs needs every frame's posteriors: no active-frame compaction */
    cfg.giveup_patience = giveup;
    if (giveup && (blind || guess)) cfg.freeze_messages = 1;      /* a frame given up asks, or guesses, with the posteriors it stopped at */
    if ((rc = qldpc_decoder_create(H, K, pos, &cfg, &dec))) return die("decoder", rc);

    printf("# * libqldpc %d on HIP device 0; Decoder_LDPC_BP_%s_Update_rule_%s (param %g), n_ite %d, syndrome %d, %d-bit messages\n", qldpc_version(),
           layered == 2 ? "vertical_layered" : (layered ? "horizontal_layered" : "flooding"), rule_name, (double)param, n_ite, synd, msg_bits);
    if (giveup) printf("#    ** frames are given up after %d syndrome tests without a new minimum of the syndrome weight%s\n", giveup,
                       blind ? " (-B: decoder created with freeze_messages = 1)" : guess ? " (-G: decoder created with freeze_messages = 1)" : "");
    printf("#    ** Info. bits (K) = %d\n#    ** Frame size (N) = %d\n#    ** Code rate  (R) = %f\n#    ** max CN degree   = %d\n", K, N, (double)K / N, qldpc_code_max_cn_degree(H));
    printf("#    ** Est. QKD Key Rate After Priv Amp = %f\n", (double)(K - (N - K)) / (double)K);
    printf("# %8s | %8s | %8s | %8s | %9s | %9s | %10s\n", "EP", "FRA", "BE", "FE", "BER", "FER", "SIM_THR");
    printf("# %8s | %8s | %8s | %8s | %9s | %9s | %10s\n", "", "", "", "", "", "", "(Mb/s)");
    if (!on_device) return 0;

    qldpc_mc_cfg mcfg;
    qldpc_mc_cfg_default(&mcfg);
    mcfg.seed = seed; mcfg.batch = batch; mcfg.parity_ber = parity_ber;
    if ((awgn || tsweep) && (awgn_punct < 0 || awgn_punct >= N)) { fprintf(stderr, "qldpc_sim: -u %d outside [0, N = %d)\n", awgn_punct, N); return 2; }
    uint8_t *cls = awgn || tsweep ? (uint8_t *)calloc((size_t)N, 1) : NULL;      /* -A, -T: every VN through the channel (class 0) but the punctured ones */
    for (int v = 0; cls && v < awgn_punct; v++) cls[v] = QLDPC_VN_PUNCTURED;
    if ((rc = qldpc_mc_create(dec, enc, cls, &mcfg, &mc))) return die("mc_create", rc);      /* NULL: info VNs through the BSC, the others pinned, as in run_host */
    free(cls);
    if (zero_source && (rc = qldpc_mc_set_source(mc, QLDPC_MC_SOURCE_ZERO))) return die("mc_set_source", rc);
    return 0;
}

/* -A: one row, the loop at this Eb/N0 */
static int mode_awgn(void)
{
    const double rate = (double)K / (double)(N - awgn_punct), sigma = sqrt(1.0 / (2.0 * rate * pow(10.0, ebno_db / 10.0)));
    const int Q = 2 * awgn_maxq + 2;
    int rc;
    uint64_t *cum = (uint64_t *)malloc(sizeof(uint64_t) * 2 * 256);
    float *value = (float *)malloc(sizeof(float) * 256);
    if (!cum || !value) return die("mc_awgn_table", QLDPC_ENOMEM);
    if ((rc = qldpc_mc_awgn_table(sigma, awgn_rmax, awgn_maxq, cum, cum + 256, value))) return die("mc_awgn_table", rc);
    const qldpc_mc_channel table = {Q, {cum, cum + 256}, value, {0, 0}};
    if ((rc = qldpc_mc_set_channel(mc, &table))) return die("mc_set_channel", rc);
    free(cum); free(value);
    printf("# Eb/N0 %.4f dB at rate %d / %d: sigma %.6f, %d levels, rmax %g\n", ebno_db, K, N - awgn_punct, sigma, Q, awgn_rmax);
    qldpc_mc_result r;
    if ((rc = qldpc_mc_run(mc, 0.25 /* not used with a table */, 0, MAX_FRAMES, max_fe, &r))) return die("mc_run", rc);
    row_f(ebno_db, r.frames, r.bit_errors, r.frame_errors, (double)r.frames, r.decode_ms * 1e-3);
    return 0;
}

/* -T: the Eb/N0 points from ONE qldpc_mc_sweep_tables, a table per row */
static int mode_tsweep(void)
{
    const double rate = (double)K / (double)(N - awgn_punct);
    const int Q = 2 * awgn_maxq + 2;
    int P = 0, rc;
    while (t_lo + (double)P * t_step <= t_hi + 1e-9 && P <= QLDPC_MC_SWEEP_MAX_POINTS) P++;
    if (P > QLDPC_MC_SWEEP_MAX_POINTS) { fprintf(stderr, "qldpc_sim: -T gives more than %d points\n", QLDPC_MC_SWEEP_MAX_POINTS); return 2; }
    qldpc_mc_table_point *pts = (qldpc_mc_table_point *)calloc((size_t)P, sizeof(*pts));
    qldpc_mc_point_stat *rows = (qldpc_mc_point_stat *)malloc(sizeof(*rows) * (size_t)P);
    uint64_t *cum = (uint64_t *)malloc(sizeof(uint64_t) * 2 * 256 * (size_t)P);
    float *value = (float *)malloc(sizeof(float) * 256 * (size_t)P);
    if (!pts || !rows || !cum || !value) return die("mc_sweep_tables", QLDPC_ENOMEM);
    for (int q = 0; q < P; q++) {
        const double db = t_lo + (double)q * t_step, sigma = sqrt(1.0 / (2.0 * rate * pow(10.0, db / 10.0)));
        uint64_t *c = cum + 512 * (size_t)q;
        if ((rc = qldpc_mc_awgn_table(sigma, awgn_rmax, awgn_maxq, c, c + 256, value + 256 * (size_t)q))) return die("mc_awgn_table", rc);
        pts[q].table.levels = Q; pts[q].table.cum[0] = c; pts[q].table.cum[1] = c + 256; pts[q].table.value = value + 256 * (size_t)q;
        pts[q].label = db;
        printf("# Eb/N0 %.4f dB at rate %d / %d: sigma %.6f, %d levels, rmax %g\n", db, K, N - awgn_punct, sigma, Q, awgn_rmax);
    }
    qldpc_mc_sweep_tables_cfg tcfg;
    memset(&tcfg, 0, sizeof(tcfg));
    tcfg.points = pts; tcfg.n_points = P; tcfg.max_frames = MAX_FRAMES; tcfg.max_frame_errors = max_fe;
    qldpc_mc_sweep_result w;
    if ((rc = qldpc_mc_sweep_tables(mc, &tcfg, &w))) return die("mc_sweep_tables", rc);
    if ((rc = qldpc_mc_sweep_stats(mc, rows, P)) < 0) return die("mc_sweep_stats", rc);
    printf("# table sweep: %d points in %llu rounds, %llu frames\n", P, (unsigned long long)w.rounds, (unsigned long long)w.frames);
    for (int q = 0; q < P; q++)      /* SIM_THR: the sweep's decode time is shared by the rows, as under -W */
        row_f(rows[q].qber, rows[q].frames, rows[q].bit_errors, rows[q].frame_errors, (double)w.frames, w.decode_ms * 1e-3);
    free(pts); free(rows); free(cum); free(value);
    return 0;
}

/* -w: one qldpc_mc_strata over the weights, then FER(q) for the QBERs of -s from its rows */
static int mode_strata(void)
{
    const int P = (w_hi - w_lo) / w_step + 1;
    int rc;
    if (P > QLDPC_MC_SWEEP_MAX_POINTS) { fprintf(stderr, "qldpc_sim: -w gives %d weights, at most %d\n", P, QLDPC_MC_SWEEP_MAX_POINTS); return 2; }
    int *weights = (int *)malloc(sizeof(int) * (size_t)P);
    qldpc_mc_stratum_stat *rows = (qldpc_mc_stratum_stat *)malloc(sizeof(*rows) * (size_t)P);
    uint64_t *fr = (uint64_t *)malloc(sizeof(uint64_t) * 2 * (size_t)P), *fe = fr ? fr + P : NULL;
    if (!weights || !rows || !fr) return die("mc_strata", QLDPC_ENOMEM);
    for (int i = 0; i < P; i++) weights[i] = w_lo + i * w_step;
    qldpc_mc_strata_cfg tcfg;
    memset(&tcfg, 0, sizeof(tcfg));
    tcfg.weights = weights; tcfg.n_strata = P; tcfg.design_qber = design_qber > 0.0 ? design_qber : ber_min;
    tcfg.max_frames = MAX_FRAMES; tcfg.max_frame_errors = max_fe;
    qldpc_mc_strata_result t;
    if ((rc = qldpc_mc_strata(mc, &tcfg, &t))) return die("mc_strata", rc);
    if ((rc = qldpc_mc_strata_stats(mc, rows, P)) < 0) return die("mc_strata_stats", rc);
    printf("# strata: %d weights in %llu rounds, %llu frames, |LLR| of QBER %.4f; EP = the error weight\n", P, (unsigned long long)t.rounds,
           (unsigned long long)t.frames, tcfg.design_qber);
    for (int i = 0; i < P; i++) {      /* SIM_THR: the run's decode time is shared by the rows, as under -W */
        row_d(rows[i].weight, rows[i].frames, rows[i].bit_errors, rows[i].frame_errors, (double)t.frames, t.decode_ms * 1e-3);
        fr[i] = rows[i].frames; fe[i] = rows[i].frame_errors;
    }
    FOR_EACH_BER(ber) {
        double est[4];
        if ((rc = qldpc_mc_strata_fer_host(K, P, weights, fr, fe, ber, est))) return die("mc_strata_fer_host", rc);
        printf("# strata ber %.4f: FER %.6e over weights %d .. %d, binomial mass below %.6e, above %.6e, standard error %.6e\n", ber, est[0], w_lo,
               weights[P - 1], est[1], est[2], est[3]);
    }
    free(weights); free(rows); free(fr);
    return 0;
}

/* -W: the table from ONE qldpc_mc_sweep, a point per row */
static int mode_sweep(void)
{
    const int n_par = N - K;
    int n_rows = 0, bits = 0, n_order = 0, P = 0, rc;
    FOR_EACH_BER(ber) n_rows++;
    qldpc_mc_point *pts = (qldpc_mc_point *)calloc((size_t)(n_rows ? n_rows : 1), sizeof(*pts));
    int *order = (int *)malloc(sizeof(int) * (size_t)(n_par ? n_par : 1)), *par = (int *)malloc(sizeof(int) * (size_t)(n_par ? n_par : 1));
    if (!pts || !order || !par) return die("mc_sweep", QLDPC_ENOMEM);
    if (target_eff > 0.0) {      /* parity VN j along the accumulator, visited in bit-reversed j: every prefix is evenly spaced */
        int m = 0;
        for (int v = 0; v < N; v++) if (!is_info[v]) par[m++] = v;
        while ((1 << bits) < n_par) bits++;
        for (int i = 0; i < (1 << bits); i++) {
            int j = 0;
            for (int b = 0; b < bits; b++) j |= ((i >> b) & 1) << (bits - 1 - b);
            if (j < n_par) order[n_order++] = par[j];
        }
    }
    FOR_EACH_BER(ber) {
        const int n_punct = target_eff > 0.0 ? punct_count(ber, target_eff, 1) : 0;
        if (n_punct < 0) continue;
        pts[P].qber = ber; pts[P].n_punct = n_punct; P++;
    }
    if (P > 0) {
        qldpc_mc_sweep_cfg wcfg;
        memset(&wcfg, 0, sizeof(wcfg));
        wcfg.points = pts; wcfg.n_points = P; wcfg.punct_order = n_order ? order : NULL; wcfg.n_order = n_order;
        wcfg.max_frames = MAX_FRAMES; wcfg.max_frame_errors = max_fe;
        qldpc_mc_sweep_result w;
        if ((rc = qldpc_mc_sweep(mc, &wcfg, &w))) return die("mc_sweep", rc);
        qldpc_mc_point_stat *rows = (qldpc_mc_point_stat *)malloc(sizeof(*rows) * (size_t)P);
        if (!rows || (rc = qldpc_mc_sweep_stats(mc, rows, P)) < 0) return die("mc_sweep_stats", rows ? rc : QLDPC_ENOMEM);
        printf("# sweep: %d points in %llu rounds, %llu frames\n", P, (unsigned long long)w.rounds, (unsigned long long)w.frames);
        for (int q = 0; q < P; q++)      /* SIM_THR: the sweep's decode time is shared by the rows, so it is the sweep's throughput in every row */
            row_f(rows[q].qber, rows[q].frames, rows[q].bit_errors, rows[q].frame_errors, (double)w.frames, w.decode_ms * 1e-3);
        free(rows);
    }
    free(pts); free(order); free(par);
    return 0;
}

/* -X: every row one qldpc_mc_search */
static int mode_search(void)
{
    int rc;
    FOR_EACH_BER(ber) {
        const int n_punct = punct_count(ber, search_eff, 0);      /* as -e computes it */
        qldpc_mc_search_cfg scfg;
        memset(&scfg, 0, sizeof(scfg));
        scfg.n_punct = n_punct; scfg.frames_per_pattern = frames_per_pattern; scfg.stop_at_goal = 1;
        qldpc_mc_search_result r;
        if ((rc = qldpc_mc_search(mc, ber, &scfg, 0, MAX_FRAMES, &r))) return die("mc_search", rc);
        qldpc_mc_pattern_stat *rows = (qldpc_mc_pattern_stat *)malloc(sizeof(*rows) * (size_t)(r.patterns ? r.patterns : 1));
        if (!rows || (rc = qldpc_mc_search_stats(mc, rows, (int)r.patterns)) < 0) return die("mc_search_stats", rows ? rc : QLDPC_ENOMEM);
        uint64_t be = 0, fe = 0;
        for (uint64_t i = 0; i < r.patterns; i++) {
            printf("#   pattern %3llu: FE %llu / %d, BE %llu\n", (unsigned long long)rows[i].pattern, (unsigned long long)rows[i].frame_errors, frames_per_pattern,
                   (unsigned long long)rows[i].bit_errors);
            be += rows[i].bit_errors; fe += rows[i].frame_errors;
        }
        free(rows);
        if (r.goal != UINT64_MAX) printf("# ber %.4f: goal puncture pattern %llu (FER = 0 / %d)\n", ber, (unsigned long long)r.goal, frames_per_pattern);
        if (r.patterns) {
            printf("# ber %.4f: best of %llu patterns: FE %llu, BE %llu per %d frames\n", ber, (unsigned long long)r.patterns, (unsigned long long)r.best_frame_errors,
                   (unsigned long long)r.best_bit_errors, frames_per_pattern);
            if (pattern_out) {
                int *vn = (int *)malloc(sizeof(int) * (size_t)(n_punct ? n_punct : 1));
                if (!vn || (rc = qldpc_mc_pattern_vns(mc, r.best, n_punct, 0, vn))) return die("mc_pattern_vns", vn ? rc : QLDPC_ENOMEM);
                if (write_pattern(ber, n_punct, vn, (long long)r.best_frame_errors)) return 1;
                free(vn);
            }
            row_f(ber, r.frames, be, fe, (double)r.frames, r.decode_ms * 1e-3);
        }
        fflush(stdout);
    }
    return 0;
}

/* -B: every row of -s one qldpc_mc_blind, a row per round */
static int mode_blind(void)
{
    int rc;
    if (max_rounds < 0 || max_rounds > QLDPC_MC_BLIND_MAX_ROUNDS) { fprintf(stderr, "qldpc_sim: -B rounds=%d outside 0 .. %d\n", max_rounds, QLDPC_MC_BLIND_MAX_ROUNDS); return 2; }
    qldpc_mc_blind_round_stat *rows = (qldpc_mc_blind_round_stat *)malloc(sizeof(*rows) * (size_t)(max_rounds + 2));
    if (!rows) return die("mc_blind", QLDPC_ENOMEM);
    FOR_EACH_BER(ber) {
        qldpc_mc_blind_cfg bcfg;
        memset(&bcfg, 0, sizeof(bcfg));
        bcfg.qber = ber; bcfg.ask_bits = ask_bits; bcfg.max_rounds = max_rounds; bcfg.max_frames = MAX_FRAMES; bcfg.max_frame_errors = max_fe;
        qldpc_mc_blind_result b;
        if ((rc = qldpc_mc_blind(mc, &bcfg, &b))) return die("mc_blind", rc);
        if ((rc = qldpc_mc_blind_stats(mc, rows, max_rounds + 2)) < 0) return die("mc_blind_stats", rc);
        printf("# ber %.4f: blind rounds, %d bits asked per round, at most %d rounds; EP = the round in which the frames closed; last column = key bits asked\n", ber,
               ask_bits, max_rounds);
        for (int r = 0; r <= max_rounds + 1; r++) {      /* SIM_THR: the call's decode time is shared by the rows, as under -W */
            char ep[64];
            if (r <= max_rounds) snprintf(ep, sizeof(ep), "%8d", r); else snprintf(ep, sizeof(ep), "%8s", "open");
            const double fra = rows[r].frames ? (double)rows[r].frames : 1.0;
            printf("  %s | %8llu | %8llu | %8llu | %9.2e | %9.2e | %10.3f | %8llu\n", ep, (unsigned long long)rows[r].frames, (unsigned long long)rows[r].bit_errors,
                   (unsigned long long)rows[r].frame_errors, (double)rows[r].bit_errors / (fra * K), (double)rows[r].frame_errors / fra,
                   (double)b.frames * K / (b.decode_ms * 1e-3) / 1e6, (unsigned long long)rows[r].disclosed);
        }
        double f = 0.0;
        if (b.frames && (rc = qldpc_mc_blind_efficiency_host(K, N - K, b.frames, b.disclosed, ber, &f))) return die("mc_blind_efficiency_host", rc);
        printf("# blind: %llu frames, %llu open, %llu key bits disclosed, %llu decodes in %llu launches = %.4f per frame; FER %.3e; f = %.4f\n",
               (unsigned long long)b.frames, (unsigned long long)b.open, (unsigned long long)b.disclosed, (unsigned long long)b.decodes, (unsigned long long)b.launches,
               b.frames ? (double)b.decodes / (double)b.frames : 0.0, b.frames ? (double)b.frame_errors / (double)b.frames : 0.0, f);
        if (gave_line(ber)) return 1;
        fflush(stdout);
    }
    free(rows);
    return 0;
}

/* -G g: every row of -s one qldpc_mc_guess, three rows */
static int mode_guess(void)
{
    int rc;
    static const char *const name[3] = {"closed", "rescued", "open"};
    FOR_EACH_BER(ber) {
        qldpc_mc_guess_cfg gcfg;
        memset(&gcfg, 0, sizeof(gcfg));
        gcfg.qber = ber; gcfg.guess_bits = guess_bits; gcfg.max_frames = MAX_FRAMES; gcfg.max_frame_errors = max_fe;
        qldpc_mc_guess_result r;
        qldpc_mc_blind_round_stat rows[3];
        if ((rc = qldpc_mc_guess(mc, &gcfg, &r))) return die("mc_guess", rc);
        if ((rc = qldpc_mc_guess_stats(mc, rows, 3)) < 0) return die("mc_guess_stats", rc);
        printf("# ber %.4f: guessing rounds, %d guess bits = %d trials per failed frame; EP = how the frames ended; last column = undetected errors\n", ber, guess_bits,
               1 << guess_bits);
        for (int i = 0; i < 3; i++) {      /* SIM_THR: the call's decode time is shared by the rows, as under -W */
            const double fra = rows[i].frames ? (double)rows[i].frames : 1.0;
            printf("  %8s | %8llu | %8llu | %8llu | %8llu | %9.2e | %9.2e | %10.3f\n", name[i], (unsigned long long)rows[i].frames, (unsigned long long)rows[i].bit_errors,
                   (unsigned long long)rows[i].frame_errors, (unsigned long long)rows[i].undetected, (double)rows[i].bit_errors / (fra * K), (double)rows[i].frame_errors / fra,
                   (double)r.frames * K / (r.decode_ms * 1e-3) / 1e6);
        }
        printf("# guess: %llu frames, %llu rescued, %llu open, %llu ambiguous, %llu trials (%llu ok) in %llu launches = %.4f decodes per frame, %.2f iterations per trial; "
               "FER %.3e, rescued wrong %llu\n",
               (unsigned long long)r.frames, (unsigned long long)r.rescued, (unsigned long long)r.open, (unsigned long long)r.ambiguous, (unsigned long long)r.trials,
               (unsigned long long)r.n_ok_sum, (unsigned long long)r.launches, r.frames ? (double)r.decodes / (double)r.frames : 0.0,
               r.trials ? (double)r.trial_iter_sum / (double)r.trials : 0.0, r.frames ? (double)(r.open + rows[0].frame_errors + rows[1].frame_errors) / (double)r.frames : 0.0,
               (unsigned long long)rows[1].frame_errors);
        printf("# guess stages (ms): source %.3f, encode %.3f, channel %.3f, load %.3f, decode %.3f, select %.3f, expand %.3f, pick %.3f, advance %.3f; total %.3f\n",
               r.source_ms, r.encode_ms, r.channel_ms, r.load_ms, r.decode_ms, r.select_ms, r.expand_ms, r.pick_ms, r.advance_ms, r.total_ms);
        if (gave_line(ber)) return 1;
        fflush(stdout);
    }
    return 0;
}

/* -D alone: the same table, every row one qldpc_mc_run */
static int mode_rows(void)
{
    FOR_EACH_BER(ber) {
        qldpc_mc_result r;
        const int rc = qldpc_mc_run(mc, ber, 0, MAX_FRAMES, max_fe, &r);
        if (rc) return die("mc_run", rc);
        row_f(ber, r.frames, r.bit_errors, r.frame_errors, (double)r.frames, r.decode_ms * 1e-3);
        if (gave_line(ber)) return 1;
        fflush(stdout);
    }
    return 0;
}

/* the harness's own loop: source, BSC and monitor on the host, one decode_siho per batch */
static int run_host(void)
{
    int rc;
    int *ref_bits = (int *)malloc(sizeof(int) * (size_t)batch * K), *enc_bits = (int *)malloc(sizeof(int) * (size_t)batch * N);
    int *dec_bits = (int *)malloc(sizeof(int) * (size_t)batch * K);
    float *llr = (float *)malloc(sizeof(float) * (size_t)batch * N);
    rng_state = seed;
    int *par_pos = (int *)malloc(sizeof(int) * (size_t)(N - K + 1));
    int n_par = 0;
    for (int v = 0; v < N; v++) if (!is_info[v]) par_pos[n_par++] = v;
    FOR_EACH_BER(ber) {
        const float L = qldpc_bsc_llr((float)ber);
        const int n_punct = target_eff > 0.0 ? punct_count(ber, target_eff, 0) : 0;
        long fra = 0, be = 0, fe = 0, best_fe = -1, best_be = -1, n_pat = 0;
        int *best_pat = (search && n_punct > 0) ? (int *)malloc(sizeof(int) * (size_t)n_punct) : NULL;
        double t_dec = 0.0;
        while (fra < frames) {
            long pat_be = 0, pat_fe = 0;
            const int nb = frames - fra < batch ? (int)(frames - fra) : batch;
            for (long i = 0; i < (long)nb * K; i++) ref_bits[i] = (int)(rng_next() & 1);
            if ((rc = qldpc_encode(enc, ref_bits, enc_bits, nb))) return die("encode", rc);
            for (int f = 0; f < nb; f++)
                for (int v = 0; v < N; v++) {
                    const int x = enc_bits[(size_t)f * N + v];
                    if (is_info[v]) { const int y = x ^ (rng_unit() < ber); llr[(size_t)f * N + v] = y ? -L : L; }      /* BSC + demodulate */
                    else { const int y = x ^ (parity_ber > 0.0 && rng_unit() < parity_ber); llr[(size_t)f * N + v] = y ? -QLDPC_CONFIRMED_BIT_LLR : QLDPC_CONFIRMED_BIT_LLR; }   /* disclosed parity (possibly dirty) */
                }
            if (n_punct > 0) {      /* new random pattern per batch: partial Fisher-Yates over the parity positions */
                for (int i = 0; i < n_punct; i++) { const int j = i + (int)(rng_next() % (uint64_t)(n_par - i)); const int t = par_pos[i]; par_pos[i] = par_pos[j]; par_pos[j] = t; }
                for (int f = 0; f < nb; f++) for (int i = 0; i < n_punct; i++) llr[(size_t)f * N + par_pos[i]] = 0.0f;          /* main.cpp:359-362 */
            }
            const double t0 = now_s();
            if ((rc = qldpc_decode_siho(dec, llr, dec_bits, nb))) return die("decode_siho", rc);
            t_dec += now_s() - t0;
            qldpc_decoder_reset(dec);
            for (int f = 0; f < nb; f++) {
                long e = 0;
                for (int i = 0; i < K; i++) e += dec_bits[(size_t)f * K + i] != ref_bits[(size_t)f * K + i];
                be += e; fe += e > 0; pat_be += e; pat_fe += e > 0;
            }
            fra += nb;
            if (best_pat) {      /* the reference's random search (main.cpp:321-333): one shuffled pattern per simulation round, keep the best */
                printf("#   pattern %3ld: FE %ld / %d, BE %ld\n", n_pat, pat_fe, nb, pat_be);
                if (best_fe < 0 || pat_fe < best_fe || (pat_fe == best_fe && pat_be < best_be)) { best_fe = pat_fe; best_be = pat_be; memcpy(best_pat, par_pos, sizeof(int) * (size_t)n_punct); }
                n_pat++;
            }
        }
        if (best_pat) {
            printf("# ber %.4f: best of %ld patterns: FE %ld, BE %ld per %d frames\n", ber, n_pat, best_fe, best_be, batch);
            if (pattern_out && write_pattern(ber, n_punct, best_pat, best_fe)) return 1;
            free(best_pat);
        }
        row_f(ber, (uint64_t)fra, (uint64_t)be, (uint64_t)fe, (double)fra, t_dec);
        if (gave_line(ber)) return 1;
        fflush(stdout);
    }
    free(par_pos); free(ref_bits); free(enc_bits); free(dec_bits); free(llr);
    return 0;
}

int main(int argc, char **argv)
{
    int rc = parse(argc, argv);
    if (!rc) rc = setup();
    if (!rc) rc = !on_device ? run_host() : awgn ? mode_awgn() : tsweep ? mode_tsweep() : strata ? mode_strata() : blind ? mode_blind() : guess ? mode_guess() : sweep ? mode_sweep() : search_eff > 0.0 ? mode_search() : mode_rows();
    if (rc) return rc;
    qldpc_mc_free(mc);
    qldpc_decoder_free(dec); qldpc_encoder_free(enc); qldpc_code_free(H);
    free(pos); free(is_info);
    return 0;
}
