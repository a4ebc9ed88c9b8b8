/*
 * qldpc_stream.c -- BASELINE config 3 timed from C: a stream of sifted-key epochs whose code rate is picked per epoch from the
 * estimated QBER (BS/src/main.cpp:29,235-266), through the reconciliation sessions the ecd2 handlers call
 * (qldpc_recon_encode_blocks on Alice's side, ONE qldpc_recon_decode_blocks call on Bob's), host buffers in and out.
 * Nothing but the C ABI is inside the timed region: no interpreter, no list building.
 *
 *   epochs x key_bits sifted bits, QBER per epoch ~ U[qmin, qmax] (what the daemon would have estimated), Bob's copy = Alice's
 *   through a BSC of that QBER; reconciled = status OK and Bob's words == Alice's.
 *
 * usage: qldpc_stream [-e epochs] [-k key_bits] [-b max_blocks] [-S seed] [-r reps] [-q qmin:qmax] [-l (layered) | -f (flooding); default: the sessions' choice = layered for batches] [-P depth (PEG mothers)]
 *                     [-g rate_gap] [-G gap_profile] [-p (per-kernel profile of Bob's decoders in a second pass)]
 *                     [-H (privacy amplification of the reconciled blocks after every timed decode: ONE qldpc_privamp_blocks call, final_bits =
 *                          key_bits - leaked bits, seed from the block index; adds pa_ms_mean, pa_ms_best, distill_Mbit_s_mean)]
 *                     [-U (Toeplitz hashing of the reconciled blocks after every timed decode: ONE qldpc_toeplitz_blocks call, out_bits =
 *                          key_bits - leaked bits, one seed of 2 key_bits - 1 bits shared by the call.  The seed comes from this tool's own
 *                          deterministic generator: a MEASUREMENT seed, not a random one, and nothing to deploy.  Adds tpa_ms_mean,
 *                          tpa_ms_best, tdistill_Mbit_s_mean; may be given together with -H)]
 *                     [-N (the -U stage on an NTT context, qldpc_toeplitz_create_cfg with QLDPC_TOEPLITZ_NTT; implies -U.  After every timed call
 *                          the same blocks go through a direct context, untimed, and the words are compared: adds tpa_method,
 *                          tpa_equals_direct (1 when every word of every call was equal) and tpa_checksum (FNV-1a of the last call's words))]
 *                     [-V (error verification after every timed decode: Alice's tags of her keys and Bob's tags of what he now holds, the
 *                          blocks that failed included, are each ONE qldpc_polyhash_blocks call over all epochs under one key shared by the
 *                          call.  The key comes from this tool's own deterministic generator: a MEASUREMENT key, not a random one, and
 *                          nothing to deploy.  Adds vt_ms_mean, vt_ms_best (Bob's call), vt_agree (blocks with status OK whose tags are
 *                          equal: must equal reconciled), vt_failed_differ (failed blocks whose tags differ) beside vt_failed_words_differ
 *                          (failed blocks whose words differ from Alice's: the two must be equal), vt_equals_host (1 when every device tag
 *                          of the last call equals qldpc_polyhash_host, untimed) and vt_leak_bits; may be given together with -H / -U / -N)]
 *                     [-Y (verification inside the decode call: the timed call is ONE qldpc_recon_decode_blocks_tagged under the measurement key of -V,
 *                          which hashes Bob's decoded rows where they lie on the device, and Alice's tags come from ONE qldpc_recon_tag_blocks
 *                          call on her session.  Adds yt_equal (blocks with status OK whose tag is Alice's: must equal reconciled), yt_failed_zero
 *                          (failed blocks, whose tag must be zeros), yt_leak_bits, and a line "tags equal: a / b" on stderr; ms_mean and ms_best
 *                          are then the tagged call's wall time.  With -V as well both stages run and yt_equals_vt says whether every tag of a
 *                          reconciled block equals the polyhash context's: it must be 1)]
 *                     (defaults: 512 epochs x 52 429 bits, max_blocks 512, PEG depth 2 = the library's default)
 * prints one JSON object on stdout.
 */
#include <math.h>
#include <pthread.h>
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
    fprintf(stderr, "qldpc_stream: %s: %s (%d) %s\n", what, qldpc_strerror(rc), rc, qldpc_last_error());
    return 1;
}

struct part { qldpc_recon *r; int n; uint32_t **keys; int *kb; float *qber; qldpc_recon_msg *msgs; const uint32_t **pars; int *status, *corrected, *iters; int rc; };
static void *part_main(void *arg)
{
    struct part *p = arg;
    p->rc = qldpc_recon_decode_blocks(p->r, p->n, p->keys, p->kb, p->qber, p->msgs, p->pars, p->status, p->corrected, p->iters);
    return NULL;
}

int main(int argc, char **argv)
{
    int epochs = 512, key_bits = 52429, batch = 512, reps = 3, layered = -1, profile = 0, peg = 2, opt, a_lanes = 0, b_lanes = 0, verbose = 0, split = 1, gap_profile = 0, hash = 0, toeplitz = 0, ntt = 0, verify = 0, intag = 0;
    uint64_t seed = 42;
    double qmin = 0.005, qmax = 0.06, gap = 0.0;
    while ((opt = getopt(argc, argv, "e:k:b:S:r:q:lfpP:g:A:B:vT:G:HUNVY")) != -1) {
        switch (opt) {
        case 'e': epochs = atoi(optarg); break;
        case 'k': key_bits = atoi(optarg); break;
        case 'b': batch = atoi(optarg); break;
        case 'S': seed = strtoull(optarg, NULL, 0); break;
        case 'r': reps = atoi(optarg); break;
        case 'q': if (sscanf(optarg, "%lf:%lf", &qmin, &qmax) != 2) { fprintf(stderr, "-q qmin:qmax\n"); return 2; } break;
        case 'l': layered = 1; break;
        case 'f': layered = 0; break;
        case 'p': profile = 1; break;
        case 'P': peg = atoi(optarg); break;
        case 'g': gap = atof(optarg); break;
        case 'A': a_lanes = atoi(optarg); break;      /* lanes of Alice's / Bob's calls (QLDPC_RECON_LANES, set per call): diagnostics */
        case 'B': b_lanes = atoi(optarg); break;
        case 'v': verbose = 1; break;
        case 'G': gap_profile = atoi(optarg); break;      /* qldpc_recon_cfg.gap_profile */
        case 'H': hash = 1; break;
        case 'U': toeplitz = 1; break;
        case 'N': toeplitz = 1; ntt = 1; break;
        case 'V': verify = 1; break;
        case 'Y': intag = 1; break;
        case 'T': split = atoi(optarg); break;      /* experiment: T sessions on T host threads, each decoding every T-th epoch */
        default: fprintf(stderr, "usage: see the head of qldpc_stream.c\n"); return 2;
        }
    }
    if (epochs < 1 || key_bits < 32 || batch < 1 || reps < 1) return 2;
    rng_state = seed;
    const int W = (key_bits + 31) / 32;
    uint32_t *alice = calloc((size_t)epochs * W, 4), *bob = calloc((size_t)epochs * W, 4), *work = calloc((size_t)epochs * W, 4);
    float *qber = calloc((size_t)epochs, sizeof(float));
    if (!alice || !bob || !work || !qber) return 1;
    for (int e = 0; e < epochs; e++) {
        qber[e] = (float)(qmin + (qmax - qmin) * rng_unit());
        for (int w = 0; w < W; w++) alice[(size_t)e * W + w] = (uint32_t)rng_next();
        if (key_bits & 31) alice[(size_t)e * W + W - 1] &= 0xFFFFFFFFu << (32 - (key_bits & 31));
        memcpy(bob + (size_t)e * W, alice + (size_t)e * W, (size_t)W * 4);
        for (int i = 0; i < key_bits; i++)
            if (rng_unit() < qber[e]) bob[(size_t)e * W + (i >> 5)] ^= 1u << (31 - (i & 31));
    }

    qldpc_recon_cfg cfg;
    qldpc_recon_cfg_default(&cfg);
    cfg.max_blocks = batch;
    if (layered >= 0) cfg.schedule = layered ? QLDPC_SCHED_HLAYERED : QLDPC_SCHED_FLOODING;      /* else the default: layered for batches of more than 8 blocks */
    else layered = batch > 8;
    cfg.rate_gap = (float)gap;
    cfg.peg_depth = peg;
    cfg.gap_profile = gap_profile;
    qldpc_recon *ra = NULL, *rb = NULL;
    int rc;
    if ((rc = qldpc_recon_create(&cfg, &ra)) || (rc = qldpc_recon_create(&cfg, &rb))) return die("recon_create", rc);

    qldpc_recon_msg *msgs = calloc((size_t)epochs, sizeof(*msgs));
    const uint32_t **akeys = calloc((size_t)epochs, sizeof(*akeys));
    uint32_t **bkeys = calloc((size_t)epochs, sizeof(*bkeys)), **pars = calloc((size_t)epochs, sizeof(*pars));
    int *kb = calloc((size_t)epochs, sizeof(int)), *cap = calloc((size_t)epochs, sizeof(int));
    int *status = calloc((size_t)epochs, sizeof(int)), *corrected = calloc((size_t)epochs, sizeof(int)), *iters = calloc((size_t)epochs, sizeof(int));
    int max_par = 0;
    for (int e = 0; e < epochs; e++) {
        qldpc_recon_msg m;
        if ((rc = qldpc_recon_plan(ra, key_bits, qber[e], &m))) return die("recon_plan", rc);
        if ((int)((m.code_m + 31) / 32) > max_par) max_par = (int)((m.code_m + 31) / 32);
    }
    uint32_t *parbuf = calloc((size_t)epochs * max_par, 4);
    for (int e = 0; e < epochs; e++) {
        akeys[e] = alice + (size_t)e * W; bkeys[e] = work + (size_t)e * W; pars[e] = parbuf + (size_t)e * max_par;
        kb[e] = key_bits; cap[e] = max_par;
    }

    /* Alice: first call builds the codes of the table, the second is timed */
    char num[16];
    if (a_lanes) { snprintf(num, sizeof(num), "%d", a_lanes); setenv("QLDPC_RECON_LANES", num, 1); }
    if ((rc = qldpc_recon_encode_blocks(ra, epochs, akeys, kb, qber, msgs, pars, cap))) return die("recon_encode_blocks", rc);
    uint32_t *par_first = NULL;
    qldpc_recon_msg *msg_first = NULL;
    if (verbose) {
        par_first = malloc((size_t)epochs * max_par * 4); msg_first = malloc((size_t)epochs * sizeof(*msgs));
        memcpy(par_first, parbuf, (size_t)epochs * max_par * 4); memcpy(msg_first, msgs, (size_t)epochs * sizeof(*msgs));
    }
    double t0 = now_s();
    if ((rc = qldpc_recon_encode_blocks(ra, epochs, akeys, kb, qber, msgs, pars, cap))) return die("recon_encode_blocks", rc);
    const double t_enc = now_s() - t0;
    if (verbose) {
        int diff = 0;
        for (int e = 0; e < epochs; e++)
            if (memcmp(&msg_first[e], &msgs[e], sizeof(*msgs)) || memcmp(par_first + (size_t)e * max_par, parbuf + (size_t)e * max_par, 4 * (size_t)qldpc_recon_parity_words(&msgs[e]))) {
                if (diff < 8) fprintf(stderr, "alice: block %d (rate index %u) differs between her two calls (crc %08x vs %08x)\n", e, msgs[e].rate_index, msg_first[e].crc32, msgs[e].crc32);
                diff++;
            }
        fprintf(stderr, "alice: %d of %d blocks differ between two identical encode calls\n", diff, epochs);
        for (int e = 0; e < epochs; e++)
            if (msgs[e].crc32 != qldpc_crc32_words(akeys[e], key_bits)) { fprintf(stderr, "alice: block %d: device CRC %08x, host CRC %08x\n", e, msgs[e].crc32, qldpc_crc32_words(akeys[e], key_bits)); break; }
    }
    if (b_lanes) { snprintf(num, sizeof(num), "%d", b_lanes); setenv("QLDPC_RECON_LANES", num, 1); }

    if (split > 1) {
        /* experiment: the stream dealt to `split` sessions, each on its own host thread (every split-th epoch), timed together */
        struct part P[8];
        pthread_t th[8];
        if (split > 8) split = 8;
        for (int t = 0; t < split; t++) {
            struct part *p = &P[t];
            memset(p, 0, sizeof(*p));
            if ((rc = qldpc_recon_create(&cfg, &p->r))) return die("recon_create", rc);
            p->keys = calloc((size_t)epochs, sizeof(*p->keys)); p->pars = calloc((size_t)epochs, sizeof(*p->pars)); p->kb = calloc((size_t)epochs, sizeof(int));
            p->qber = calloc((size_t)epochs, sizeof(float)); p->msgs = calloc((size_t)epochs, sizeof(*msgs));
            p->status = calloc((size_t)epochs, sizeof(int)); p->corrected = calloc((size_t)epochs, sizeof(int)); p->iters = calloc((size_t)epochs, sizeof(int));
            int seen[8] = {0};
            for (int e = 0; e < epochs; e++) {
                const int ri = msgs[e].rate_index & 7;
                if (seen[ri]++ % split != t) continue;      /* every split-th epoch OF EACH RATE: the rate groups are halved */
                p->keys[p->n] = bkeys[e]; p->pars[p->n] = pars[e]; p->kb[p->n] = kb[e]; p->qber[p->n] = qber[e]; p->msgs[p->n] = msgs[e]; p->n++;
            }
        }
        double bestT = 1e30;
        int goodT = 0;
        for (int rep = -1; rep < reps; rep++) {
            memcpy(work, bob, (size_t)epochs * W * 4);
            t0 = now_s();
            for (int t = 0; t < split; t++) pthread_create(&th[t], NULL, part_main, &P[t]);
            for (int t = 0; t < split; t++) pthread_join(th[t], NULL);
            const double dt = now_s() - t0;
            if (rep >= 0 && dt < bestT) bestT = dt;
            goodT = 0;
            for (int t = 0; t < split; t++) { if (P[t].rc) return die("decode (split)", P[t].rc); for (int i = 0; i < P[t].n; i++) goodT += P[t].status[i] == QLDPC_OK; }
        }
        printf("{\"experiment\": \"%d sessions on %d threads\", \"reconciled\": %d, \"ms_best\": %.3f, \"Mbit_s_best\": %.1f}\n", split, split, goodT, bestT * 1e3, (double)goodT * key_bits / bestT / 1e6);
        return 0;
    }
    /* Bob: one untimed pass builds his decoders, then `reps` timed passes over fresh copies of his keys */
    double best = 1e30, sum = 0.0;
    int good = 0;
    long leaked = 0;
    double it_sum = 0.0;
    /* -H: the hash stage on the blocks Bob has just reconciled; the context and its argument arrays exist before the timed region */
    qldpc_privamp_ctx *pa = NULL;
    const uint32_t **pa_keys = NULL;
    uint32_t **pa_out = NULL, *pa_seed = NULL, *pa_buf = NULL;
    int *pa_wb = NULL, *pa_fb = NULL;
    double pa_best = 1e30, pa_sum = 0.0, final_sum = 0.0;
    if (hash) {
        if ((rc = qldpc_privamp_create(cfg.device, epochs, key_bits, key_bits, &pa))) return die("privamp_create", rc);
        pa_keys = calloc((size_t)epochs, sizeof(*pa_keys)); pa_out = calloc((size_t)epochs, sizeof(*pa_out)); pa_seed = calloc((size_t)epochs, 4);
        pa_wb = calloc((size_t)epochs, sizeof(int)); pa_fb = calloc((size_t)epochs, sizeof(int)); pa_buf = calloc((size_t)epochs * W, 4);
        if (!pa_keys || !pa_out || !pa_seed || !pa_wb || !pa_fb || !pa_buf) return 1;
    }
    /* -U: the same stage with the Toeplitz hash, one measurement seed shared by the blocks of the call */
    qldpc_toeplitz_ctx *tz = NULL, *tz_direct = NULL;
    uint32_t **tz_out2 = NULL, *tz_buf2 = NULL;
    int tz_equal = 1;
    uint64_t tz_checksum = 0;
    const uint32_t **tz_keys = NULL, **tz_seeds = NULL;
    uint32_t **tz_out = NULL, *tz_seed = NULL, *tz_buf = NULL;
    int *tz_kb = NULL, *tz_ob = NULL;
    double tz_best = 1e30, tz_sum = 0.0, tz_final_sum = 0.0;
    if (toeplitz) {
        if (ntt) {
            qldpc_toeplitz_cfg tc;
            qldpc_toeplitz_cfg_default(&tc);
            tc.device = cfg.device; tc.max_blocks = epochs; tc.max_key_bits = key_bits; tc.max_out_bits = key_bits; tc.method = QLDPC_TOEPLITZ_NTT;
            if ((rc = qldpc_toeplitz_create_cfg(&tc, &tz))) return die("toeplitz_create_cfg", rc);
            if ((rc = qldpc_toeplitz_create(cfg.device, epochs, key_bits, key_bits, &tz_direct))) return die("toeplitz_create", rc);
            tz_out2 = calloc((size_t)epochs, sizeof(*tz_out2)); tz_buf2 = calloc((size_t)epochs * W, 4);
            if (!tz_out2 || !tz_buf2) return 1;
        } else if ((rc = qldpc_toeplitz_create(cfg.device, epochs, key_bits, key_bits, &tz))) return die("toeplitz_create", rc);
        const size_t sw = qldpc_toeplitz_seed_words(key_bits, key_bits);
        tz_keys = calloc((size_t)epochs, sizeof(*tz_keys)); tz_seeds = calloc((size_t)epochs, sizeof(*tz_seeds)); tz_out = calloc((size_t)epochs, sizeof(*tz_out));
        tz_kb = calloc((size_t)epochs, sizeof(int)); tz_ob = calloc((size_t)epochs, sizeof(int)); tz_buf = calloc((size_t)epochs * W, 4); tz_seed = calloc(sw, 4);
        if (!tz_keys || !tz_seeds || !tz_out || !tz_kb || !tz_ob || !tz_buf || !tz_seed) return 1;
        for (size_t w = 0; w < sw; w++) tz_seed[w] = (uint32_t)rng_next();
    }
    /* -V: error verification of every block, one measurement key shared by the call */
    qldpc_polyhash_ctx *vt = NULL;
    const uint32_t **vt_hk = NULL;
    uint32_t **vt_a = NULL, **vt_b = NULL, *vt_buf = NULL, vt_key[2] = {0, 0};
    double vt_best = 1e30, vt_sum = 0.0;
    int vt_agree = 0, vt_failed_differ = 0, vt_failed_words_differ = 0, vt_equals_host = 1;
    if (verify || intag) { vt_key[0] = (uint32_t)rng_next(); vt_key[1] = (uint32_t)rng_next(); }      /* one measurement key for both stages */
    /* -Y: the tags of the decode call itself, and Alice's from her session */
    const uint32_t **yt_hk = NULL;
    uint32_t **yt_a = NULL, **yt_b = NULL, *yt_buf = NULL;
    int yt_equal = 0, yt_failed_zero = 0, yt_failed = 0, yt_equals_vt = 1;
    if (intag) {
        yt_hk = calloc((size_t)epochs, sizeof(*yt_hk)); yt_a = calloc((size_t)epochs, sizeof(*yt_a)); yt_b = calloc((size_t)epochs, sizeof(*yt_b));
        yt_buf = calloc((size_t)epochs * 4, 4);
        if (!yt_hk || !yt_a || !yt_b || !yt_buf) return 1;
        for (int e = 0; e < epochs; e++) { yt_hk[e] = vt_key; yt_a[e] = yt_buf + (size_t)e * 4; yt_b[e] = yt_a[e] + 2; }
        if ((rc = qldpc_recon_tag_blocks(ra, epochs, akeys, kb, 1, yt_hk, yt_a))) return die("recon_tag_blocks", rc);
    }
    if (verify) {
        qldpc_polyhash_cfg vc;
        qldpc_polyhash_cfg_default(&vc);
        vc.device = cfg.device; vc.max_blocks = epochs; vc.max_key_bits = key_bits;
        if ((rc = qldpc_polyhash_create_cfg(&vc, &vt))) return die("polyhash_create_cfg", rc);
        vt_hk = calloc((size_t)epochs, sizeof(*vt_hk)); vt_a = calloc((size_t)epochs, sizeof(*vt_a)); vt_b = calloc((size_t)epochs, sizeof(*vt_b));
        vt_buf = calloc((size_t)epochs * 4, 4);
        if (!vt_hk || !vt_a || !vt_b || !vt_buf) return 1;
        for (int e = 0; e < epochs; e++) { vt_hk[e] = vt_key; vt_a[e] = vt_buf + (size_t)e * 4; vt_b[e] = vt_a[e] + 2; }
    }
    for (int rep = -1; rep < reps; rep++) {
        memcpy(work, bob, (size_t)epochs * W * 4);
        t0 = now_s();
        if (intag) rc = qldpc_recon_decode_blocks_tagged(rb, epochs, bkeys, kb, qber, msgs, (const uint32_t *const *)pars, 1, yt_hk, yt_b, status, corrected, iters);
        else rc = qldpc_recon_decode_blocks(rb, epochs, bkeys, kb, qber, msgs, (const uint32_t *const *)pars, status, corrected, iters);
        const double dt = now_s() - t0;
        if (rc) return die(intag ? "recon_decode_blocks_tagged" : "recon_decode_blocks", rc);
        if (intag) {
            yt_equal = 0; yt_failed_zero = 0; yt_failed = 0;
            for (int e = 0; e < epochs; e++) {
                if (status[e] == QLDPC_OK) yt_equal += !memcmp(yt_a[e], yt_b[e], 8);
                else { yt_failed++; yt_failed_zero += yt_b[e][0] == 0 && yt_b[e][1] == 0; }
            }
        }
        if (verbose) {
            int bad = 0, pos[8] = {0};
            fprintf(stderr, "bob rep %d:", rep);
            for (int e = 0; e < epochs; e++) {
                const int ri = msgs[e].rate_index & 7;
                if (status[e] != QLDPC_OK) { if (bad < 12) fprintf(stderr, " [blk %d rate %d pos-in-group %d it %d]", e, ri, pos[ri], iters[e]); bad++; }
                pos[ri]++;
            }
            fprintf(stderr, " -> %d failed\n", bad);
        }
        if (hash) {
            int m = 0;
            long bits = 0;
            for (int e = 0; e < epochs; e++) {
                if (status[e] != QLDPC_OK) continue;
                const int fb = key_bits - qldpc_recon_leaked_bits(&msgs[e]);
                pa_keys[m] = work + (size_t)e * W; pa_out[m] = pa_buf + (size_t)e * W; pa_wb[m] = key_bits; pa_fb[m] = fb > 0 ? fb : 0;
                pa_seed[m] = 0x9e3779b9u * (uint32_t)(e + 1) | 1u;
                bits += pa_fb[m];
                m++;
            }
            t0 = now_s();
            rc = qldpc_privamp_blocks(pa, m, pa_keys, pa_wb, pa_seed, pa_fb, pa_out);
            const double dp = now_s() - t0;
            if (rc) return die("privamp_blocks", rc);
            if (rep >= 0) { pa_sum += dp; final_sum += (double)bits; if (dp < pa_best) pa_best = dp; }
        }
        if (toeplitz) {
            int m = 0;
            long bits = 0;
            for (int e = 0; e < epochs; e++) {
                if (status[e] != QLDPC_OK) continue;
                const int ob = key_bits - qldpc_recon_leaked_bits(&msgs[e]);
                tz_keys[m] = work + (size_t)e * W; tz_seeds[m] = tz_seed; tz_out[m] = tz_buf + (size_t)e * W; tz_kb[m] = key_bits; tz_ob[m] = ob > 0 ? ob : 0;
                bits += tz_ob[m];
                m++;
            }
            t0 = now_s();
            rc = qldpc_toeplitz_blocks(tz, m, tz_keys, tz_kb, tz_seeds, tz_ob, tz_out);
            const double dp = now_s() - t0;
            if (rc) return die("toeplitz_blocks", rc);
            if (rep >= 0) { tz_sum += dp; tz_final_sum += (double)bits; if (dp < tz_best) tz_best = dp; }
            if (ntt) {
                for (int i = 0; i < m; i++) tz_out2[i] = tz_buf2 + (tz_out[i] - tz_buf);
                if ((rc = qldpc_toeplitz_blocks(tz_direct, m, tz_keys, tz_kb, tz_seeds, tz_ob, tz_out2))) return die("toeplitz_blocks (direct)", rc);
                tz_checksum = 0xcbf29ce484222325ull;
                for (int i = 0; i < m; i++) {
                    const size_t ow = ((size_t)tz_ob[i] + 31) / 32;
                    if (memcmp(tz_out[i], tz_out2[i], 4 * ow)) tz_equal = 0;
                    for (size_t w = 0; w < ow; w++) tz_checksum = (tz_checksum ^ tz_out[i][w]) * 0x100000001b3ull;
                }
            }
        }
        if (verify) {
            if ((rc = qldpc_polyhash_blocks(vt, epochs, akeys, kb, vt_hk, vt_a))) return die("polyhash_blocks (alice)", rc);
            t0 = now_s();
            rc = qldpc_polyhash_blocks(vt, epochs, (const uint32_t *const *)bkeys, kb, vt_hk, vt_b);
            const double dv = now_s() - t0;
            if (rc) return die("polyhash_blocks (bob)", rc);
            if (rep >= 0) { vt_sum += dv; if (dv < vt_best) vt_best = dv; }
            vt_agree = 0; vt_failed_differ = 0; vt_failed_words_differ = 0;
            for (int e = 0; e < epochs; e++) {
                const int same = !memcmp(vt_a[e], vt_b[e], 8);
                if (status[e] == QLDPC_OK) vt_agree += same;
                else { vt_failed_differ += !same; vt_failed_words_differ += memcmp(work + (size_t)e * W, alice + (size_t)e * W, (size_t)W * 4) != 0; }
            }
            if (intag)      /* both stages: the tag of the decode call is the context's tag of the same key */
                for (int e = 0; e < epochs; e++)
                    if (status[e] == QLDPC_OK && (memcmp(yt_b[e], vt_b[e], 8) || memcmp(yt_a[e], vt_a[e], 8))) yt_equals_vt = 0;
            if (rep == reps - 1)
                for (int e = 0; e < epochs; e++) {
                    uint32_t tag[2];
                    if ((rc = qldpc_polyhash_host(bkeys[e], key_bits, vt_key, 256, 0, tag))) return die("polyhash_host", rc);
                    if (memcmp(tag, vt_b[e], 8)) vt_equals_host = 0;
                }
        }
        if (rep < 0) continue;
        sum += dt;
        if (dt < best) best = dt;
        good = 0; leaked = 0; it_sum = 0.0;
        for (int e = 0; e < epochs; e++) {
            it_sum += iters[e];
            if (status[e] == QLDPC_OK && !memcmp(work + (size_t)e * W, alice + (size_t)e * W, (size_t)W * 4)) { good++; leaked += qldpc_recon_leaked_bits(&msgs[e]); }
        }
    }
    int per_rate[8] = {0}, fail_rate[8] = {0}, maxed[8] = {0}, it_max[8] = {0};
    double it_mean[8] = {0};
    for (int e = 0; e < epochs; e++) {
        if (iters[e] > it_max[msgs[e].rate_index & 7]) it_max[msgs[e].rate_index & 7] = iters[e];
        it_mean[msgs[e].rate_index & 7] += iters[e];
        per_rate[msgs[e].rate_index & 7]++;
        if (!(status[e] == QLDPC_OK && !memcmp(work + (size_t)e * W, alice + (size_t)e * W, (size_t)W * 4))) fail_rate[msgs[e].rate_index & 7]++;
        if (iters[e] >= cfg.n_ite) maxed[msgs[e].rate_index & 7]++;
    }
    const double mean = sum / reps;
    printf("{\"workload\": \"%d epochs x %d bits, QBER ~ U[%.3f, %.3f] seed %llu, batches of <= %d blocks, %s, one %s call\", "
           "\"reconciled\": %d, \"epochs\": %d, \"ms_mean\": %.3f, \"ms_best\": %.3f, \"Mbit_s_mean\": %.1f, \"Mbit_s_best\": %.1f, "
           "\"leaked_fraction\": %.4f, \"avg_iterations\": %.2f, \"alice_encode_ms\": %.3f, \"epochs_per_rate\": [%d, %d, %d, %d], \"failed_per_rate\": [%d, %d, %d, %d], "
           "\"at_max_iterations_per_rate\": [%d, %d, %d, %d], \"mean_iterations_per_rate\": [%.1f, %.1f, %.1f, %.1f], \"max_iterations_per_rate\": [%d, %d, %d, %d]",
           epochs, key_bits, qmin, qmax, (unsigned long long)seed, batch, layered ? "layered" : "flooding", intag ? "decode_blocks_tagged" : "decode_blocks", good, epochs, mean * 1e3, best * 1e3,
           (double)good * key_bits / mean / 1e6, (double)good * key_bits / best / 1e6, (double)leaked / fmax(1.0, (double)good * key_bits), it_sum / epochs,
           t_enc * 1e3, per_rate[0], per_rate[1], per_rate[2], per_rate[3], fail_rate[0], fail_rate[1], fail_rate[2], fail_rate[3], maxed[0], maxed[1], maxed[2], maxed[3],
           it_mean[0] / fmax(1, per_rate[0]), it_mean[1] / fmax(1, per_rate[1]), it_mean[2] / fmax(1, per_rate[2]), it_mean[3] / fmax(1, per_rate[3]), it_max[0], it_max[1], it_max[2], it_max[3]);
    if (hash)
        printf(", \"pa_ms_mean\": %.3f, \"pa_ms_best\": %.3f, \"distill_Mbit_s_mean\": %.1f", pa_sum / reps * 1e3, pa_best * 1e3, final_sum / (sum + pa_sum) / 1e6);
    if (toeplitz)
        printf(", \"tpa_ms_mean\": %.3f, \"tpa_ms_best\": %.3f, \"tdistill_Mbit_s_mean\": %.1f", tz_sum / reps * 1e3, tz_best * 1e3, tz_final_sum / (sum + tz_sum) / 1e6);
    if (ntt)
        printf(", \"tpa_method\": \"ntt\", \"tpa_equals_direct\": %d, \"tpa_checksum\": \"%016llx\"", tz_equal, (unsigned long long)tz_checksum);
    if (verify)
        printf(", \"vt_ms_mean\": %.3f, \"vt_ms_best\": %.3f, \"vt_agree\": %d, \"vt_failed_differ\": %d, \"vt_failed_words_differ\": %d, \"vt_equals_host\": %d, \"vt_leak_bits\": %d",
               vt_sum / reps * 1e3, vt_best * 1e3, vt_agree, vt_failed_differ, vt_failed_words_differ, vt_equals_host, qldpc_polyhash_leaked_bits(1));
    if (intag) {
        printf(", \"yt_equal\": %d, \"yt_failed\": %d, \"yt_failed_zero\": %d, \"yt_leak_bits\": %d", yt_equal, yt_failed, yt_failed_zero, qldpc_recon_leaked_bits_tagged(&msgs[0], 1) - qldpc_recon_leaked_bits(&msgs[0]));
        if (verify) printf(", \"yt_equals_vt\": %d", yt_equals_vt);
        fprintf(stderr, "qldpc_stream: tags equal: %d / %d, decode_blocks_tagged %.3f ms mean, %.3f ms best\n", yt_equal, epochs, mean * 1e3, best * 1e3);
    }
    if (profile) {
        qldpc_kernel_stat st[16];
        qldpc_recon_profile_enable(rb, 1);
        memcpy(work, bob, (size_t)epochs * W * 4);
        if ((rc = qldpc_recon_decode_blocks(rb, epochs, bkeys, kb, qber, msgs, (const uint32_t *const *)pars, status, corrected, iters))) return die("recon_decode_blocks", rc);
        const int n = qldpc_recon_profile_read(rb, st, 16);
        printf(", \"kernels\": {");
        for (int i = 0; i < n; i++)
            printf("%s\"%s\": {\"launches\": %llu, \"ms\": %.3f, \"alg_GB\": %.3f}", i ? ", " : "", st[i].name, (unsigned long long)st[i].launches, st[i].total_ms, st[i].alg_bytes / 1e9);
        printf("}");
    }
    printf("}\n");
    qldpc_privamp_free(pa);
    qldpc_toeplitz_free(tz);
    qldpc_toeplitz_free(tz_direct);
    qldpc_polyhash_free(vt);
    qldpc_recon_free(ra);
    qldpc_recon_free(rb);
    if (intag && (yt_equal != good || yt_failed_zero != yt_failed || !yt_equals_vt)) return 4;
    return good == epochs ? 0 : 3;
}
