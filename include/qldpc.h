/*
 * qldpc.h -- C ABI of libqldpc.so: MI355X (gfx950) batched LDPC belief-propagation reconciliation.
 *
 * This is the drop-in boundary for the LDPC path of JarryChou/qcrypto-ldpc.  Plain C types only
 * (pointers, sizes, ints, floats); no C++/torch types.  Every entry point returns QLDPC_OK (0) or a
 * negative qldpc_status; nothing throws.  One decoder instance is not re-entrant (neither is an
 * AFF3CT module); use one per host thread / stream.
 *
 * Reference interfaces replaced (paths under /root/reference/errorcorrection/, BS =
 * ldpc_examples/my_project_with_aff3ct/examples/bootstrap, VAR = BS/src/variants (copy out as main.cpp to use)):
 *
 *   qldpc_code_from_alist / _from_qc      tools::LDPC_matrix_handler::read_matrix_size / read
 *                                         VAR/main.cpp (alist-v1.0.1):324,338 ; VAR/main.cpp (qc):145
 *   qldpc_code_ira                        tools::build_dvbs2 + tools::build_H        BS/src/main.cpp:175-176
 *                                         (DVB-S2 tables are AFF3CT built-ins and not in the tree; this
 *                                         builds a DVB-like IRA code of any (N,K) instead)
 *   qldpc_code_max_cn_degree              H.get_cols_max_degree()                    BS/src/main.cpp:178
 *   qldpc_decoder_create                  module::Decoder_LDPC_BP_flooding<B,Q,Rule>(K, N, n_ite, H, info_bits_pos,
 *                                         rule(param), enable_syndrome, syndrome_depth, n_frames)
 *                                         BS/src/main.cpp:193 ; VAR/main.cpp (alist-v1.0.1):179-256
 *   qldpc_decode_siho                     decoder->decode_siho(LLRs, dec_bits)       BS/src/main.cpp:365
 *   qldpc_decoder_reset                   (*(m.decoder)).reset()                     BS/src/main.cpp:389
 *   qldpc_llr_from_ber, QLDPC_CONFIRMED_BIT_LLR   LLR(BER), CONFIRMED_BIT_LLR        BS/src/main.cpp:19-20
 *   qldpc_load_bits_*  (frame formation)  modem->demodulate + parity pinning + puncturing
 *                                         BS/src/main.cpp:348-362 ; VAR/main.cpp (5g-qc):514-531
 *   qldpc_encoder_* / qldpc_encode_*      m.encoder->encode(ref_bits, enc_bits)      BS/src/main.cpp:341 ;
 *                                         Encoder_LDPC_from_H(K,N,H,"IDENTITY",...)  VAR/main.cpp (alist-v1.0.1):142-145
 *   qldpc_min_code_rate, qldpc_parity_bits_to_punct   min_cr(), parity_bits_to_punct()   BS/src/main.cpp:23-34
 *   packed-bit layout (bit i <-> word[i/32] & (1u << (31 - i%32)))                  subcomponents/helpers.h:65-70
 *   qldpc_code_ira_peg / qldpc_code_qc_peg   ldpc_examples/improved-peg.py:136-195 / psd-peg.py:281-447 (H-matrix construction)
 *   qldpc_decoder_cfg.msg_dtype = 2       the fixed-point layered min-sum of ldpc_examples/.../BPSK_nrldpc_sim_RM_FP.m:37-98
 *   qldpc_recon_* (sessions)              what the two `return 81` arms of subcomponents/qber_estim.c:337-340,420-423 need:
 *                                         rate choice (BS/src/main.cpp:29,235-266), frame formation, verification; bound by
 *                                         qcrypto-ldpc_amd/host/ldpc_reconcile.c (packet handlers, cascade fallback, batched ingest)
 *   qldpc_privamp*                        the hash loop of privAmp_doPrivAmp         subcomponents/priv_amp.c:190-218
 *   qldpc_toeplitz*                       (not in the reference) Toeplitz hashing, the sound replacement of that loop
 *   qldpc_polyhash*                       (not in the reference) error verification by a universal hash, beside the sessions' CRC-32
 *   qldpc_recon_*_tagged / _tag_blocks    (not in the reference) the same tag inside Bob's verify step, over his decoded rows on the device
 *   qldpc_qber_* / _recon_estimate_blocks (not in the reference, which samples disclosed bits: subcomponents/qber_estim.c) the QBER out of the parity message
 *   qldpc_mc_*                            the simulation loop itself: source, encoder, BSC, decoder, Monitor_BFER   BS/src/main.cpp:335-393
 *   qldpc_mc_search / _patterns_dev       the puncture-pattern search around it: shuffle, erase, first FER = 0 / n  BS/src/main.cpp:235-411
 *   qldpc_mc_sweep                        the BER loop around both, with its puncture count per BER                BS/src/main.cpp:233-272
 *   qldpc_mc_strata / _weight_frames_*    the same loop over fixed error weights instead of BERs: FER(q) for every q   (no counterpart)
 *   qldpc_mc_set_channel / _awgn_table   the channel of the fixed-point sims: BPSK over AWGN, 6-bit received values  ML/BPSK_nrldpc_sim_RM_FP.m
 *   qldpc_mc_sweep_tables                 the Eb/N0 points of those sims side by side in one batch, a table per point    ML/sim_results.m
 *   qldpc_polar_*                         the polar encoder and SC decoder of the fourth curve of that figure   ML/nrpolar_encode.m, nrpolar_scdecode.m, nrpolar_scdecode_FP.m
 *   qldpc_polar_list_* / _crc_host        the list decoder with a CRC of the fifth curve (list 4, CRC 11)          ML/nrpolar_sclistdecode_FP.m
 *   qldpc_polar_mc_*                      the frame loop of those two scripts around either decoder, on the device   the while loops of the same scripts
 *   qldpc_polar_tally_* / _construct_*    (not in the reference, which reads the 5G sequence) the information set fitted to a channel by genie-aided Monte Carlo
 *   qldpc_polar_recon_*                   (not in the reference) reconciliation sessions around either polar decoder: syndrome, crc, prior, verdict, leak
 *   qldpc_polar_decode_rows_* / _recon_*_ladder, _decode_rounds   (not in the reference) a frozen set per frame, and incremental freezing rounds on it
 *   qldpc_polar_recon_*_flip / qldpc_polar_flip_select_*   (not in the reference) SC-Flip trials for the blocks of a session that failed
 */
#ifndef QLDPC_H
#define QLDPC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QLDPC_VERSION 100

typedef enum qldpc_status {
    QLDPC_OK = 0,
    QLDPC_EINVAL = -1,       /* bad argument                                                    */
    QLDPC_ENOMEM = -2,       /* host or device allocation failed                                */
    QLDPC_EIO = -3,          /* matrix file unreadable / malformed                              */
    QLDPC_EHIP = -4,         /* a HIP call failed (qldpc_last_error() has the text)             */
    QLDPC_ENODEV = -5,       /* no gfx950-capable device visible                                */
    QLDPC_ESIZE = -6,        /* size mismatch (AFF3CT throws tools::length_error here)          */
    QLDPC_EUNSUPPORTED = -7, /* valid request this build does not implement                     */
    QLDPC_ESTATE = -8,       /* call sequence error (e.g. run before load)                      */
    QLDPC_EDECODE = -9       /* reconciliation failed: no codeword found or CRC mismatch        */
} qldpc_status;

/* tools::Update_rule_* selected at VAR/main.cpp (alist-v1.0.1):203-218 */
typedef enum qldpc_rule {
    QLDPC_RULE_MS = 0,            /* Update_rule_MS                                  */
    QLDPC_RULE_OMS = 1,           /* Update_rule_OMS(offset)        param = offset   */
    QLDPC_RULE_NMS = 2,           /* Update_rule_NMS(norm_factor)   param = factor   */
    QLDPC_RULE_SPA = 3,           /* Update_rule_SPA(max_CN_degree)                  */
    QLDPC_RULE_LSPA = 4,          /* Update_rule_LSPA                                */
    QLDPC_RULE_AMS_MIN = 5,       /* Update_rule_AMS<min>                            */
    QLDPC_RULE_AMS_MINSTAR_L2 = 6,/* Update_rule_AMS<min_star_linear2>               */
    QLDPC_RULE_AMS_MINSTAR = 7    /* Update_rule_AMS<min_star>                       */
} qldpc_rule;

/* Decoder_LDPC_BP_{flooding,horizontal_layered,vertical_layered}; VAR/main.cpp (alist-v1.0.1):203-237, 240-256 */
typedef enum qldpc_schedule {
    QLDPC_SCHED_FLOODING = 0,
    QLDPC_SCHED_HLAYERED = 1,     /* horizontal layered, checks visited in the code's layer order; compact = 1 is honoured with fp32 messages and a launch per layer */
#define QLDPC_RECON_SCHED_AUTO 2  /* qldpc_recon_cfg.schedule only: chosen by the batch size of the session's decoders */
    QLDPC_SCHED_VLAYERED = 3      /* vertical layered (VAR/main.cpp (alist-v1.0.1):240-256), VNs visited in the code's vlayer order: per (VN, check) pair the
                                     horizontal recursion with only the VN's own message and posterior written.  FRAMES engine (auto resolves to it), fp32
                                     messages, all rules, freeze_messages 0 / 1, frames_per_lane 0 / 1 / 2 / 4, syndrome form, erasures; engine = EDGES,
                                     msg_dtype 1 / 2, layer_chain = 1 and compact = 1 are refused with QLDPC_EUNSUPPORTED, and sessions (qldpc_recon_cfg)
                                     refuse it with QLDPC_EINVAL.  AFF3CT's source is not in the reference tree: parity is unpinned against AFF3CT,
                                     bit-exact means against the project's CPU reference of the recursion (tests/vlayered_ref.py) */
} qldpc_schedule;

/*
 * Two kernel families behind the same calls:
 *   FRAMES  frame-interleaved: a wavefront lane = a frame; thousands of frames per launch (HBM-bound)
 *   EDGES   edge-parallel: lanes run over the edges of ONE frame, check groups staged in LDS, min/sign
 *           fold by wavefront shuffles; the daemon's one-block-at-a-time case (flooding; MS/OMS/NMS/SPA;
 *           check degree <= 64, VN degree <= 32)
 */
typedef enum qldpc_engine { QLDPC_ENGINE_AUTO = 0, QLDPC_ENGINE_FRAMES = 1, QLDPC_ENGINE_EDGES = 2 } qldpc_engine;

/* Per-VN class for QKD frame formation (BS/src/main.cpp:348-362) */
enum {
    QLDPC_VN_CHANNEL = 0,   /* sifted-key bit seen through the BSC:  LLR = (1-2y) ln((1-p)/p)      */
    QLDPC_VN_PINNED = 1,    /* bit disclosed by Alice (parity):      LLR = y ? -23.02585 : +23.02585 */
    QLDPC_VN_PUNCTURED = 2  /* punctured parity VN:                  LLR = 0                         */
};

#define QLDPC_CONFIRMED_BIT_LLR 23.025850929840455f /* -log(1e-10 / (1 - 1e-10)), BS/src/main.cpp:19 */

typedef struct qldpc_code qldpc_code;
typedef struct qldpc_decoder qldpc_decoder;
typedef struct qldpc_encoder qldpc_encoder;

/* ------------------------------------------------------------------ library ------------------ */
int qldpc_version(void);
const char *qldpc_strerror(int status);
const char *qldpc_last_error(void);           /* thread-local text of the last failure          */
int qldpc_device_count(void);                 /* HIP devices visible (0 on a CPU-only host)     */
/* Measurement aid (bench.py): the rate at which `device` copies `bytes` (read once + written once, non-temporal) in the decoder's own
 * access shape -- wide = 0: 256-byte rows, one dword per lane, eight rows in flight per wavefront; wide = 1: 16 bytes per lane.
 * The figure counts bytes read + bytes written, like the kernels' rooflines.  No reference counterpart. */
int qldpc_copy_probe(int device, size_t bytes, int reps, int wide, double *gbytes_per_s);

/* ------------------------------------------------------------------ scalar helpers ----------- */
float qldpc_llr_from_ber(float ber);                          /* LLR(BER) = -log(p/(1-p)) in double, BS/src/main.cpp:20 */
float qldpc_bsc_llr(float ber);                               /* Modem_OOK_BSC: logf((1-p)/p) in float, BS/src/main.cpp:317,348 */
float qldpc_binary_entropy(float q);                          /* h(q), BS/src/main.cpp:23-26       */
float qldpc_min_code_rate(float qber, float efficiency);      /* 1/(1+f h(q))... BS/src/main.cpp:29 */
int qldpc_parity_bits_to_punct(int N, int K, float target_cr);/* BS/src/main.cpp:34                */

/* ------------------------------------------------------------------ code (H matrix) ---------- */
int qldpc_code_from_alist(const char *path, qldpc_code **out);
int qldpc_code_from_qc(const char *path, qldpc_code **out);
/* (var[e], chk[e]) in add_connection order: that order is each check's edge order. */
int qldpc_code_from_edges(int N, int M, int E, const int *var, const int *chk, qldpc_code **out);
/*
 * DVB-like IRA code: info VNs 0..K-1 (the first hi_frac*K have degree dv_hi, the rest dv_lo),
 * parity VNs K..N-1 on a dual diagonal, every check the same number of info edges, seeded
 * socket shuffle.  (N=65536,K=52429,hi_frac=.125,dv_hi=11,dv_lo=3,seed=7) is BASELINE config 2.
 */
int qldpc_code_ira(int N, int K, float hi_frac, int dv_hi, int dv_lo, uint64_t seed, qldpc_code **out);
/*
 * The same profile with the information part built by progressive edge growth (what the reference's
 * ldpc_examples/improved-peg.py:136-195 / psd-peg.py set out to do): each new edge goes to a lowest-degree
 * check not reached from its variable node within `depth` check levels, so no cycle shorter than
 * 2 (depth + 1) is closed while avoidable (depth 2: no 4-cycles).  Deterministic in (profile, depth, seed).
 */
int qldpc_code_ira_peg(int N, int K, float hi_frac, int dv_hi, int dv_lo, int depth, uint64_t seed, qldpc_code **out);
/*
 * Quasi-cyclic code whose base graph is grown by PEG with a circulant shift per edge chosen so that the cycles closed in
 * the base graph stay open in the lifted graph (what the reference's ldpc_examples/psd-peg.py:281-447 does, regular
 * information-column degree dv, parity part = identity, output also as an AFF3CT .qc file when qc_path != NULL):
 * N = (n_cols + m_rows) Z, M = m_rows Z.  *base_girth (optional) = shortest cycle closed in the base graph (0 = none);
 * no cycle of length 4 exists in the lifted graph.  Deterministic in (n_cols, m_rows, dv, Z, seed).
 */
int qldpc_code_qc_peg(int n_cols, int m_rows, int dv, int Z, uint64_t seed, const char *qc_path, qldpc_code **out, int *base_girth);
void qldpc_code_free(qldpc_code *code);
int qldpc_code_n(const qldpc_code *code);
int qldpc_code_m(const qldpc_code *code);
int qldpc_code_e(const qldpc_code *code);
int qldpc_code_max_cn_degree(const qldpc_code *code);
int qldpc_code_max_vn_degree(const qldpc_code *code);
int qldpc_code_is_ira(const qldpc_code *code);     /* 1 if parity VNs K..N-1 form a dual diagonal */
/* The chain of an IRA code as the posterior form of the flooding run uses it (see qldpc_decoder_flood_post): one word per check c,
 * byte 0 / 1 = positions of VN K + c - 1 / K + c in the row of check c, byte 2 = position of VN K + c - 1 in the row of check c - 1,
 * byte 3 = position of VN K + c in the row of check c + 1 (0xff: no such edge).  Verified edge by edge; check degrees <= 27.
 * Returns 1 and fills tab[M] (NULL: only the verdict), 0 if the graph does not qualify. */
int qldpc_code_chain_table(const qldpc_code *code, uint32_t *tab);
/* CN-major edge list, E entries each (pass NULL to skip one). */
int qldpc_code_export_edges(const qldpc_code *code, int *var, int *chk);
/* Number of conflict-free layers of the horizontal-layered order, and that order (M entries). */
int qldpc_code_layer_count(const qldpc_code *code);
int qldpc_code_layer_order(const qldpc_code *code, int *check_order, int *layer_ptr /* layers+1 */);
/* The same for the vertical-layered order: classes of VNs that share no check (N entries; built on first use).  Both return 1 when the
 * classes in order are the sequential sweep in index order, 0 when the sweep runs in the exported (coloured) order. */
int qldpc_code_vlayer_count(const qldpc_code *code);
int qldpc_code_vlayer_order(const qldpc_code *code, int *vn_order, int *vlayer_ptr /* classes+1 */);
/* H x over GF(2) for one host word of 0/1 ints; returns the syndrome weight (>= 0) or a status. */
int qldpc_code_syndrome_host(const qldpc_code *code, const int *x, int *s);

/* ------------------------------------------------------------------ decoder ------------------ */
typedef struct qldpc_decoder_cfg {
    int schedule;        /* qldpc_schedule                                                       */
    int rule;            /* qldpc_rule                                                           */
    float rule_param;    /* OMS offset / NMS factor                                              */
    int n_ite;           /* maximum BP iterations (AFF3CT n_ite)                                 */
    int enable_syndrome; /* stop a frame once its syndrome is zero (AFF3CT enable_syndrome)      */
    int syndrome_depth;  /* consecutive zero syndromes required (AFF3CT syndrome_depth), >= 1    */
    int max_frames;      /* capacity: frames decoded concurrently in one call (AFF3CT n_frames)  */
    int device;          /* HIP device ordinal                                                   */
    int frames_per_lane; /* 0 = auto; 1, 2 or 4 frames per wavefront lane (64/128/256-frame groups) */
    int engine;          /* qldpc_engine: 0 = auto (edge-parallel for <= 8 frames when supported) */
    int freeze_messages; /* FRAMES engine with enable_syndrome: 1 = a converged frame's messages are frozen bit-for-bit
                            (lane-masked stores; qldpc_fetch_post_dev is then exact for every frame, ~15 % slower);
                            0 = only its hard decisions / iteration count / success flag are frozen (default)      */
    int msg_dtype;       /* 0 = fp32 messages (the AFF3CT float build, bit-exact class); 1 = messages rounded to
                            binary16 in HBM, fp32 arithmetic (half the bytes per iteration; FER-tolerance class against
                            AFF3CT, bit-exact against the oracle run with the same rounding; FRAMES engine, flooding);
                            2 = 8-bit fixed point: channel LLRs quantised to clamp(rint(LLR * quant_scale), +-127), messages
                            saturating at +-127, integer min-sum (MS / OMS / NMS; flooding, or horizontal layered with the posterior
                            kept in 8 bits as well; FRAMES engine, 4 frames per lane):
                            a quarter of the bytes per iteration, FER-tolerance class against AFF3CT, bit-exact against the
                            oracle's integer decoder; qldpc_fetch_post_dev then returns the integer posteriors           */
    float quant_scale;   /* msg_dtype 2: quantiser steps per LLR unit (0 = 8.0); OMS offset = rint(rule_param * quant_scale)
                            steps, NMS factor = rint(rule_param * 128) / 128                                          */
    int compact;         /* FRAMES engine, enable_syndrome, freeze_messages = 0: active-frame compaction.
                            Once the frames that have not converged fit into <= 0.6 of the groups in flight they are dealt into fewer,
                            full groups (the message arrays are not copied: the next check pass reads them through a slot map), so a
                            group no longer runs until its slowest frame.  Decisions, iteration counts and success flags are unchanged;
                            qldpc_fetch_post_dev is refused after a run that compacted.  0 = auto (flooding: batches of >= 4 groups;
                            layered schedules: never), 1 = whenever a group can be saved, 2 = never.
                            Horizontal layered: only 1 compacts -- fp32 messages (explicit or the compressed check state), frames_per_lane
                            1 / 2 / 4, a launch per layer; the posteriors are gathered into a side buffer and the first sweep afterwards reads
                            the old generation's messages through the slot map into a second one (two pairs, allocated at the first compaction
                            and counted by qldpc_decoder_device_bytes).  layer_chain = 1, msg_dtype = 2, freeze_messages = 1 and
                            enable_syndrome = 0 run as without it.  The vertical-layered schedule refuses 1.                */
    int layer_chain;     /* horizontal layered, fp32 messages, 64-frame groups, freeze_messages = 0, check degree <= 40: run a sweep as ONE launch in
                            which a check waits for the earlier checks on its own variable nodes (per-VN version counters, agent-coherent posterior
                            rows) instead of one launch per layer of mutually VN-disjoint checks.  Same results bit for bit.  0 = auto (fixed-iteration
                            runs with 2 to 8 frame groups and a layer launch of 8 192 .. 65 535 waves: measured +10 .. 13 % on the N = 10^6 code with 128 - 256
                            frames; no gain with one group or with the per-sweep early exit, a loss with many groups or several decoders side by side),
                            1 = on, 2 = off.  The one-launch sweep works on explicit messages.  Layered MS / OMS / NMS sweeps (fp32, 64-frame groups,
                            check degree <= 32, freeze_messages = 0) otherwise keep a COMPRESSED CHECK STATE -- the two magnitudes a check's messages
                            take and two dc-bit masks per frame instead of the dc messages (csrc/qldpc_kernels_cst.h): the same floats, 0.61 x the
                            bytes on the N = 10^6 code -- so for those rules auto never picks the one-launch sweep, and 1 gives up the state for it */
    int giveup_patience; /* FRAMES engine, enable_syndrome = 1, flooding or horizontal layered: 0 = off (the run launches what it always did);
                            p >= 1 = give a frame up once its syndrome weight has not reached a new minimum for p tests in a row.  The weight of a
                            frame at a test is the number of checks with (H x + s)_c = 1 over the sign ballots the test reads; the tests are the
                            ones the early exit makes anyway (flooding: after iterations 1 .. n_ite - 1, layered: after every sweep).  At the
                            first test, or when w < best: best = w, since = 0; otherwise since += 1.  The convergence logic (syndrome_depth) is
                            untouched and wins; a frame that is not done, has w > 0 and since >= p is given up: its done bit is set, its
                            iteration count is the iterations executed, and from there it is a finished frame in every respect (ballots, hard
                            decisions and iteration count frozen, messages frozen with freeze_messages = 1, its group skipped once all its frames
                            are done, left behind by a compaction).  Its success flag, the syndrome of the hard decisions it stopped with, is 0.
                            p >= n_ite never gives up and only counts (qldpc_fetch_giveup_dev).  The rule is stated once, in
                            csrc/qldpc_giveup_core.h; qldpc_giveup_host is its mirror.  Negative: QLDPC_EINVAL; enable_syndrome = 0:
                            QLDPC_EINVAL; engine = EDGES or the vertical-layered schedule: QLDPC_EUNSUPPORTED; engine auto picks FRAMES.
                            qldpc_gang_create refuses such a member; qldpc_mc_blind asks for freeze_messages = 1 with it; the sessions
                            (qldpc_recon_*) create their decoders without it.  (This word was reserved[1], must be zero, before.)   */
} qldpc_decoder_cfg;

void qldpc_decoder_cfg_default(qldpc_decoder_cfg *cfg);
/* info_bits_pos may be NULL (= 0..K-1, the harness default VAR/main.cpp (alist-v1.0.1):147-159). */
int qldpc_decoder_create(const qldpc_code *code, int K, const int *info_bits_pos,
                         const qldpc_decoder_cfg *cfg, qldpc_decoder **out);
void qldpc_decoder_free(qldpc_decoder *dec);
/* hipStream_t to launch on (NULL = the null stream).  All *_dev calls are asynchronous on it.
 * STREAM SWITCH, the rule of every set_stream call of the library (qldpc_decoder_, qldpc_gang_, qldpc_qber_, qldpc_polar_ and qldpc_polar_list_set_stream)
 * and of a gang that takes a member back: a switch to another stream orders the new stream after everything the context has queued on the old one
 * (an event recorded on the old stream that the new one waits for; the call itself waits for nothing), so load on A, set_stream(B), run is a run
 * after the load.  The same stream again does nothing.  The old stream must still exist when the switch is made.  The caller's own buffers are the
 * caller's to order: what another stream writes into an input is not known to the context. */
int qldpc_decoder_set_stream(qldpc_decoder *dec, void *hip_stream);
int qldpc_decoder_reset(qldpc_decoder *dec);
size_t qldpc_decoder_device_bytes(const qldpc_decoder *dec);   /* HBM held by this decoder        */
/* 1 if fixed-iteration flooding runs of this decoder take the posterior form: the variable-node passes write one posterior row per information VN,
 * the checks rebuild their previous messages from three state rows each and fold the IRA chain in (0.83 x the rows of an iteration, bit-identical
 * results).  Decided once at creation: FRAMES engine, flooding, fp32 messages, 64-frame groups, MS / OMS / NMS, enable_syndrome = 0, check degrees <= 27
 * in register-resident buckets, and a graph for which qldpc_code_chain_table returns 1.  Everything else -- early exit included -- runs on explicit
 * messages.  Environment: QLDPC_FLOOD_POST=0 keeps the explicit messages, QLDPC_FLOOD_POST_VN=0 keeps the posterior pass between two iterations
 * on the general variable-node kernel instead of its own one-launch kernel (both: A/B measurements and tests). */
int qldpc_decoder_flood_post(const qldpc_decoder *dec);
/* Allocate now the buffers the load calls would otherwise allocate on first use (per-frame erasure ballots). */
int qldpc_decoder_reserve(qldpc_decoder *dec);

/* AFF3CT mirror, host pointers: Y_N[n_frames][N] -> V_K[n_frames][K] (one int per bit). Synchronous. */
int qldpc_decode_siho(qldpc_decoder *dec, const float *Y_N, int *V_K, int n_frames);

/* ---- staged, HBM-resident path.  d_* are device pointers on the decoder's device. ----------- */
/* load: channel LLRs [n_frames][N] float (frame-major, as decode_siho takes them). */
int qldpc_load_llr_dev(qldpc_decoder *dec, const float *d_llr, int n_frames);
/*
 * load: QKD-native frame formation on the device.  d_bits[n_frames][ceil(N/32)] packed MSB-first
 * (helpers.h:65-70): Bob's sifted-key bits at channel VNs, Alice's disclosed bits at pinned VNs.
 * d_llr_mag[n_frames] = |LLR| of a channel bit of that frame, i.e. qldpc_bsc_llr(estimated QBER)
 * (ProcessBlock.localError) computed by the host; d_vn_class[N] (NULL = all QLDPC_VN_CHANNEL) is
 * shared by all frames.
 */
int qldpc_load_bits_dev(qldpc_decoder *dec, const uint32_t *d_bits, const float *d_llr_mag,
                        const uint8_t *d_vn_class, int n_frames);
/* The same with a per-frame count of channel VNs: class-0 VNs at index >= d_n_channel[f] are known (shortened) bits of
 * frame f and are pinned like class 1.  Lets blocks of different length share one code and one launch. */
int qldpc_load_bits_short_dev(qldpc_decoder *dec, const uint32_t *d_bits, const float *d_llr_mag,
                              const uint8_t *d_vn_class, const int *d_n_channel, int n_frames);
/*
 * Syndrome form: instead of pinning disclosed parity VNs, every check c must come out with the
 * parity s_c that Alice computed on her key (s = H x_A).  d_synd_bits[n_frames][ceil(M/32)], MSB-first.  Call after
 * qldpc_load_* (which clears it) and before qldpc_run; the success flag / early exit then test H x = s.  Works with
 * any H (no encoder needed); not an AFF3CT configuration, so it is checked against the oracle's own coset mode.
 */
int qldpc_load_syndrome_dev(qldpc_decoder *dec, const uint32_t *d_synd_bits, int n_frames);
/*
 * Per-frame puncturing (BS/src/main.cpp:359-362, the harness's `LLRs[pattern[i]] = 0` with a pattern of its own for every frame):
 * d_erase_bits[n_frames][ceil(N/32)] packed MSB-first, a set bit makes that VN of that frame an erasure (channel LLR 0) whatever
 * its class in d_vn_class.  Lets blocks punctured to different efficiencies share one code and one launch.  Call after
 * qldpc_load_bits_* / qldpc_load_llr_dev for the frames just loaded; the next load clears it.
 */
int qldpc_load_erasures_dev(qldpc_decoder *dec, const uint32_t *d_erase_bits, int n_frames);
/*
 * Known bits (blind reconciliation, see qldpc_recon_decode_blind): the mirror of qldpc_load_erasures_dev.  d_known_bits / d_value_bits
 * [n_frames][ceil(N/32)] packed MSB-first, a set known bit makes that VN of that frame a known bit: its channel LLR becomes +23.03 for value bit 0
 * and -23.03 for value bit 1 (QLDPC_CONFIRMED_BIT_LLR, what the loads give a pinned VN; msg_dtype 2: what that quantises to) whatever its class.
 * Call after qldpc_load_* for the frames just loaded; the next load clears it.  The order relative to qldpc_load_syndrome_dev and
 * qldpc_load_erasures_dev is free, and where a VN is both erased and known, known wins.  Works wherever qldpc_load_erasures_dev works (both
 * engines, every schedule and message type).  Frames loaded by qldpc_load_bits_* into the coded form (flooding) are written out as the LLR array
 * they stand for and run on it: the results are bit-identical, the run reads 4 N instead of N / 8 channel bytes per frame and pass.
 */
int qldpc_load_known_dev(qldpc_decoder *dec, const uint32_t *d_known_bits, const uint32_t *d_value_bits, int n_frames);
/* s = H x for packed words d_bits[n_frames][ceil(N/32)] -> d_synd_bits[n_frames][ceil(M/32)] (Alice's side). */
int qldpc_syndrome_dev(qldpc_decoder *dec, const uint32_t *d_bits, uint32_t *d_synd_bits, int n_frames);
/* run the BP iterations on what was loaded. */
int qldpc_run(qldpc_decoder *dec);
/* fetch: hard decision of every VN, packed MSB-first, d_out[n_frames][ceil(N/32)]. */
int qldpc_fetch_packed_dev(qldpc_decoder *dec, uint32_t *d_out);
/* fetch: V_K[n_frames][K] ints at info_bits_pos (AFF3CT layout). */
int qldpc_fetch_info_dev(qldpc_decoder *dec, int *d_V_K);
/* fetch: per-frame iterations executed and 1/0 "syndrome of the hard decision is zero". */
int qldpc_fetch_status_dev(qldpc_decoder *dec, int *d_iters, int *d_ok);
/* fetch: a-posteriori LLRs [n_frames][N] (debug / parity tests; costs one extra pass). */
int qldpc_fetch_post_dev(qldpc_decoder *dec, float *d_post);
/*
 * fetch: the least reliable VNs of every frame (blind reconciliation).  Row f of d_weak_bits[n_frames][ceil(N/32)], packed MSB-first, has a bit
 * set for the min(d, candidates) candidates of frame f that come first in ascending (key, v) order, key = the bit pattern of |posterior| as
 * uint32 (bits & 0x7fffffff; -0 equals +0), over exactly the floats qldpc_fetch_post_dev returns for f (msg_dtype 2: the integer posteriors).
 * d_cand_bits[n_frames][ceil(N/32)] = the candidates of each frame (NULL = every VN), d_take[n_frames] non-zero = the frame is wanted (NULL =
 * every frame); rows of frames not taken are zero.  d = 0 gives zero rows, d < 0 is QLDPC_EINVAL.  Preconditions as qldpc_fetch_post_dev:
 * QLDPC_ESTATE without a completed run, QLDPC_EUNSUPPORTED after a run that compacted.  FRAMES engine, every schedule, message type and
 * frames_per_lane; the EDGES engine returns QLDPC_EUNSUPPORTED.  The posterior rows are read where they lie (flooding: after the posterior pass
 * qldpc_fetch_post_dev runs, in the same buffer); beyond that buffer only the output rows are written.
 */
int qldpc_fetch_weakest_dev(qldpc_decoder *dec, const uint32_t *d_cand_bits, const int *d_take, int d, uint32_t *d_weak_bits);
/* Host mirror of the select, no device needed: one frame, post[N], cand_bits[ceil(N/32)] (NULL = every v < N; bits at v >= N are ignored),
 * weak_bits[ceil(N/32)], *n_taken (optional) = bits set.  The kernel's lanes run the same functions (csrc/qldpc_weakest_core.h). */
int qldpc_weakest_host(const float *post, int N, const uint32_t *cand_bits, int d, uint32_t *weak_bits, int *n_taken);
/*
 * fetch: what the give-up rule saw (decoders created with giveup_patience >= 1; QLDPC_EUNSUPPORTED otherwise, QLDPC_ESTATE without a completed run).
 * Each array is [n_frames] ints in the caller's frame order and may be NULL; valid after a run that compacted, as qldpc_fetch_status_dev is.
 *   d_gave         1 if the frame was given up, else 0
 *   d_last_weight  the syndrome weight at the frame's last test: 0 for a converged frame, > 0 for one given up; for a frame that ran out the last test
 *                  of the run -- on the flooding schedule the one after iteration n_ite - 1, NOT the weight of the final hard decision
 *   d_best_weight  the smallest weight the frame showed at a test (-1: the run made no test, n_ite = 1 on the flooding schedule)
 * qldpc_fetch_post_dev / qldpc_fetch_weakest_dev are exact for a frame given up under the condition that makes them exact for a converged frame:
 * freeze_messages = 1 (otherwise its messages ran on after it stopped).
 */
int qldpc_fetch_giveup_dev(qldpc_decoder *dec, int *d_gave, int *d_last_weight, int *d_best_weight);
/* *frames = the frames given up by all runs of this decoder since it was created, counted on the device (0 with giveup_patience = 0): what a loop that
 * runs the decoder many times -- qldpc_mc_run, qldpc_mc_blind, qldpc_sim -g -- reports.  Synchronises the decoder's stream. */
int qldpc_giveup_total(qldpc_decoder *dec, uint64_t *frames);
/* Host mirror of the give-up rule for one frame, no device needed: weights[t] = the syndrome weight at test t + 1 (t < n_tests) of a run that never
 * stops the frame.  *stop_test (optional) = the 1-based test at which it converged or was given up, 0 if it ran out; *outcome (optional) one of
 * QLDPC_GIVEUP_*.  patience = 0: the rule is off.  QLDPC_EINVAL: n_tests < 1, syndrome_depth < 1, patience < 0, a negative weight. */
enum { QLDPC_GIVEUP_CONVERGED = 0, QLDPC_GIVEUP_GAVE_UP = 1, QLDPC_GIVEUP_RAN_OUT = 2 };
int qldpc_giveup_host(const int *weights, int n_tests, int syndrome_depth, int patience, int *stop_test, int *outcome);
/* block until everything queued on the decoder's stream is done. */
int qldpc_sync(qldpc_decoder *dec);

/* ---- measurement hooks ---------------------------------------------------------------------- */
typedef struct qldpc_kernel_stat {
    char name[32];        /* kernel family: "cn_update", "vn_update", ...                         */
    uint64_t launches;
    double total_ms;      /* hipEvent time summed over launches                                   */
    double alg_bytes;     /* algorithmic bytes summed over launches         */
    double moved_bytes;   /* bytes those launches have to move in the data form in use (e.g. with coded LLRs a
                             variable-node pass fetches N/8 bytes of received-bit ballots per frame, not the 4 N bytes of an
                             LLR array that alg_bytes prices): time these for the bandwidth actually sustained */
} qldpc_kernel_stat;
/* When on, every kernel launch is bracketed by hipEvents on the decoder's stream. */
int qldpc_profile_enable(qldpc_decoder *dec, int on);
/* Sync, fold events into stats; writes up to cap entries, returns the count (or a status). */
int qldpc_profile_read(qldpc_decoder *dec, qldpc_kernel_stat *out, int cap);
int qldpc_profile_clear(qldpc_decoder *dec);
/* Launches actually issued by the last qldpc_run (converged groups make later ones no-ops). */
int qldpc_last_run_iterations(const qldpc_decoder *dec);
/* Early-exit bookkeeping of the last qldpc_run (FRAMES engine; zeros otherwise): out[0] = lane-iterations executed (every
 * iteration a group ran counts its whole width, converged lanes included -- divide the sum of the frames' iteration counts by it
 * for the useful-work fraction), out[1] = compactions, out[2] = groups in flight at the end, out[3] = frames per group.
 * Synchronises the decoder's stream. */
int qldpc_last_run_stats(qldpc_decoder *dec, long long out[4]);

/* ------------------------------------------------------------------ decoder gangs ------------ */
/*
 * A gang steps several horizontal-layered decoders ("members") in lockstep: colour step s of a sweep covers every member that has a layer s,
 * and is ONE launch per kernel class present (degree cap 8 / 12 / 20 / 40 / any, rule family, explicit messages or compressed check state;
 * csrc/qldpc_kernels_gang.h) instead of one launch per member and bucket -- the launch granularity of a mixed-rate batch is then that of the
 * whole batch, not of its smallest group.  The kernels run the members' own per-check code, so every result (hard decisions, iteration counts,
 * success flags, posteriors) is bit-identical to qldpc_run on each member.  Ballot, syndrome and status passes stay per member.
 *
 * Members are loaded and read with their own qldpc_load_* / qldpc_fetch_* calls (syndrome form, erasures and shortened loads included) and stay
 * usable on their own: qldpc_run on a member is legal before and after gang runs, and a decoder may belong to several gangs.  Members are not
 * owned and must outlive the gang.  The gang has ONE stream (member 0's at creation, or qldpc_gang_set_stream); a taken member found on another
 * stream when a run starts is moved to the gang's by the stream switch (qldpc_decoder_set_stream): what it has queued there comes first.  Steps are ordered by the stream alone.  The host polls the members'
 * early-exit counters every p sweeps, p = the smallest non-zero polling period of a member (none: every sweep is issued, converged groups
 * return early inside the kernels); a member with no frame left takes no part in later launches.
 *
 * qldpc_gang_create refuses with QLDPC_EUNSUPPORTED a member that is not: FRAMES engine, QLDPC_SCHED_HLAYERED, fp32 messages, 64-frame groups
 * (frames_per_lane 1), compaction not enabled, one-launch sweep (layer_chain) not in use; with QLDPC_EINVAL members on different devices or with
 * different n_ite / enable_syndrome, a NULL or repeated member and n outside 1 .. QLDPC_GANG_MAX_MEMBERS; qldpc_last_error() names the member.
 * Rules, rule parameters, syndrome_depth, freeze_messages, codes and frame counts may differ.  qldpc_gang_run returns QLDPC_ESTATE before anything
 * is queued when a taken member has nothing loaded.  Flooding, vertical-layered, binary16 and 8-bit members are not built.
 *
 * Unmeasured: what a gang gains over decoders side by side on their own streams.  tools/gang_cost.py measures it; until it has run on the
 * device nothing in the library turns a gang on by itself (sessions: QLDPC_RECON_GANG=1).
 */
typedef struct qldpc_gang qldpc_gang;
#define QLDPC_GANG_MAX_MEMBERS 32      /* per gang; launches cover up to 8 members each */
int  qldpc_gang_create(qldpc_decoder *const *members, int n, qldpc_gang **out);
void qldpc_gang_free(qldpc_gang *g);                       /* members are not owned and must outlive the gang */
int  qldpc_gang_set_stream(qldpc_gang *g, void *hip_stream); /* every member's stream, by the stream switch (qldpc_decoder_set_stream): loads, the run and fetches are ordered on it */
/* take[n]: which members take part (NULL = every member); the others are left as they are.  Afterwards each taken member is as after qldpc_run. */
int  qldpc_gang_run(qldpc_gang *g, const unsigned char *take /* n flags, NULL = every member */);
/* of the last qldpc_gang_run: out[0] = sweeps issued, out[1] = layer launches issued, out[2] = layer launches the members would have issued alone
 * for the sweeps each took part in, out[3] = members the host dropped before the last sweep */
int  qldpc_gang_last_run_stats(qldpc_gang *g, long long out[4]);
/* host only, no device needed */
/* The planning a gang uses, as a function of the codes: rule[i] = qldpc_rule of member i, compressed[i] != 0 (NULL = none) = it keeps the compressed
 * check state (min-sum / AMS rules, check degree <= 32: QLDPC_EINVAL otherwise).  *steps = the largest layer count, *launches_per_sweep = the sum
 * over steps of the distinct kernel classes present, *solo_launches_per_sweep = the sum of the members' own launches (outputs may be NULL).
 * A check's cap is the smallest of 8, 12, 20, 40 that holds its degree, else 0. */
int  qldpc_gang_plan(const qldpc_code *const *codes, const int *rule, const int *compressed, int n,
                     int *steps, int *launches_per_sweep, int *solo_launches_per_sweep);
/* Host mirror of the kernels' block -> (member, block within the member's range) mapping of one launch (the same inline function): n in 1 .. 8
 * members, member m owns blocks [prefix[m], prefix[m + 1]); members of zero blocks own none.  A block at or past prefix[n]: QLDPC_EINVAL. */
int  qldpc_gang_locate_host(const int *prefix /* n + 1, non-decreasing, prefix[0] = 0 */, int n, int block, int *member, int *local);

/* ------------------------------------------------------------------ encoder (Alice) ---------- */
/* method: "IRA" (dual-diagonal accumulate), "IDENTITY" / "LU_DEC" (Encoder_LDPC_from_H's two G_methods, VAR/main.cpp (alist-v1.0.1):135-145:
 * GF(2) elimination of any H, parity positions searched from the first / from the last column) or "QC" (Encoder_LDPC_from_QC,
 * VAR/main.cpp (qc):145: info bits first, parity = H2^-1 H1 u; QLDPC_EUNSUPPORTED when H2 is singular). */
int qldpc_encoder_create(const qldpc_code *code, const char *method, int device, qldpc_encoder **out);
void qldpc_encoder_free(qldpc_encoder *enc);
/* Size the encoder's device workspace for calls of up to max_frames frames now (it otherwise grows on first need): a caller that must not
 * allocate later -- the daemon after ldpc_init -- says so here.  One encoder is not re-entrant (neither is an AFF3CT module). */
int qldpc_encoder_reserve(qldpc_encoder *enc, int max_frames);
int qldpc_encoder_k(const qldpc_encoder *enc);
int qldpc_encoder_info_bits_pos(const qldpc_encoder *enc, int *pos /* K */);
/* host mirror of encoder->encode: U_K[n_frames][K] ints -> X_N[n_frames][N] ints. */
int qldpc_encode(qldpc_encoder *enc, const int *U_K, int *X_N, int n_frames);
/* device, packed MSB-first: d_info[n_frames][ceil(K/32)] -> d_cw[n_frames][ceil(N/32)]. */
int qldpc_encode_packed_dev(qldpc_encoder *enc, const uint32_t *d_info, uint32_t *d_cw, int n_frames,
                            void *hip_stream);

/* ------------------------------------------------------------------ reconciliation sessions -- */
/*
 * What an ecd2 LDPC handler does between QBER estimation and privacy amplification, i.e. the
 * replacement of the cascade_biconf exchange (subcomponents/cascade_biconf.c:427-940, ~55 packets
 * each way) by ONE parity message: the two `return 81` arms at subcomponents/qber_estim.c:337-340
 * and :420-423 call into this.  Buffers are the daemon's own: ProcessBlock.mainBufPtr words,
 * MSB-first (helpers.h:65-70), `workbits` valid bits (helpers.c:31-69), QBER = localError.
 *
 * Per block (qldpc_recon_plan): the QBER estimate is clamped to [0.001, 0.25]; target rate R* = min(min_cr(qber, efficiency),
 * capacity - rate_gap (65536/K)^0.4) (BS/src/main.cpp:29); table rate = largest entry <= R* (:235-266); code = IRA MOTHER code with K a multiple of
 * `mother_step` (blocks above `mother_max` bits: K = workbits rounded up to `key_quantum`) and M = round(K (1-R)/R) parity VNs, the
 * information VNs past the block's length are shortened (known 0, pinned per frame); of the M parity bits only
 * d = ceil(workbits (1/R* - 1)) are disclosed and the other M - d are punctured (BS/src/main.cpp:34,305-311,359-362:
 * parity_bits_to_punct, LLR 0), evenly spaced along the accumulator.  Alice sends the d parity bits + CRC-32 of her key; Bob pins
 * them (+-23.03), erases the punctured ones, decodes and verifies.  Leak = d + 32 bits.
 */
typedef struct qldpc_recon qldpc_recon;

typedef struct qldpc_recon_cfg {
    int device;
    float efficiency;      /* f in min_cr(q, f); 1.4                        */
    int n_rates;           /* <= 8                                                               */
    float rates[8];        /* ascending; default {0.5, 0.7, 0.8, 0.9}                            */
    int n_ite;             /* 60                                                                 */
    int rule;              /* QLDPC_RULE_SPA                                                     */
    float rule_param;      /* 0 (SPA takes none)                                                 */
    int key_quantum;       /* 1024 (multiple of 32)                                              */
    int max_blocks;        /* blocks decoded concurrently by qldpc_recon_decode_batch            */
    uint64_t seed;         /* IRA construction seed shared by both sides (7)                     */
    int schedule;          /* schedule of Bob's decoder: QLDPC_RECON_SCHED_AUTO (default) = horizontal layered when the decoders take
                              batches (max_blocks > 8: half the iterations for the same bytes per sweep; config-3 stream 16.1 -> 14.4 ms,
                              0 instead of 0 - 1 first-round failures in 2 048 epochs), flooding for max_blocks <= 8 (the one-block
                              edge-parallel engine is flooding); QLDPC_SCHED_FLOODING / QLDPC_SCHED_HLAYERED force one */
    int mother_step;       /* 8192: blocks of up to mother_max bits use mother codes whose K is a multiple of this (a block
                              is shortened to its length per frame), so a handful of codes serve every block; 0 = a code per size */
    int mother_max;        /* 65536 */
    float rate_gap;        /* the effective rate stays rate_gap (65536 / K)^0.4 below the BSC capacity 1 - h(q); 0 = by rule
                              (0.035 SPA / LSPA, 0.05 min-sum family), times a factor per mother rate and size: gap_profile below */
    int puncture;          /* 1 (default): puncture parity VNs down to the target efficiency; 0 / 2: disclose all M    */
    int preload;           /* 1: build every (mother size, rate) entry in qldpc_recon_create -- no code construction and no
                              device allocation afterwards for blocks of up to mother_max bits                          */
    int peg_depth;         /* 0: the information part of every code is the seeded socket shuffle (qldpc_code_ira); 1..4: grown by
                              progressive edge growth to that depth (qldpc_code_ira_peg; 2 = no 4-cycles), SURVEY.md 8f #3.  Both
                              sides must use the same value: the codes are derived from (size, rate, peg_depth, seed)          */
    int gap_profile;       /* how far below capacity the plan stays, as a multiple c(R, K) of rate_gap (65536 / K)^0.4 per mother rate R:
                              0 = as calibrated for the construction in use (PEG: 0.10 for R <= 0.75 on mothers of K >= 32 768, more on
                              shorter ones, 0.85 for R <= 0.85, 1 above -- leak 0.29 of the key on the config-3 stream; seeded shuffle:
                              0.6 / 0.9 / 1.0); 1 = round 2's 0.6 / 0.9 / 1.0 whatever the construction (fewer iterations, leak 0.305).
                              Both sides must use the same value                                                            */
} qldpc_recon_cfg;

/* Travels in the parity packet (all fields uint32, little-endian like every ecd2 header). */
typedef struct qldpc_recon_msg {
    uint32_t rate_index;   /* index into the rate table                                          */
    uint32_t key_bits;     /* workbits                                                           */
    uint32_t code_k;       /* info VNs of the (mother) code, >= key_bits                         */
    uint32_t code_m;       /* parity VNs of the code                                             */
    uint32_t crc32;        /* CRC-32 (IEEE) of Alice's key words, tail bits masked               */
    uint32_t n_punct;      /* parity VNs punctured: code_m - n_punct bits are disclosed          */
} qldpc_recon_msg;

void qldpc_recon_cfg_default(qldpc_recon_cfg *cfg);
int qldpc_recon_create(const qldpc_recon_cfg *cfg, qldpc_recon **out);
void qldpc_recon_free(qldpc_recon *r);
/* Rate choice, code dimensions and puncturing for a block; fills everything but crc32.  qber in [0, 0.5) (0 is clamped). */
int qldpc_recon_plan(const qldpc_recon *r, int key_bits, float qber, qldpc_recon_msg *msg);
int qldpc_recon_parity_words(const qldpc_recon_msg *msg);    /* words of disclosed parity a message carries: ceil((code_m - n_punct)/32) */
int qldpc_recon_leaked_bits(const qldpc_recon_msg *msg);     /* code_m - n_punct + 32 (CRC)                                             */
int qldpc_recon_check_header(const qldpc_recon *r, const qldpc_recon_msg *msg, int key_bits);      /* QLDPC_OK / QLDPC_ESIZE: as the decode calls check it */
long qldpc_recon_entries_created(const qldpc_recon *r);      /* (code, encoder, decoder) sets built so far: constant after a preload   */
/* qldpc_profile_enable / _read of Bob's decoders, summed over the session's codes by kernel kind */
int qldpc_recon_profile_enable(qldpc_recon *r, int on);
int qldpc_recon_profile_read(qldpc_recon *r, qldpc_kernel_stat *out, int cap);
/* Alice: the disclosed parity bits (qldpc_recon_parity_words(msg_out) words, MSB-first, in position order) + message header. */
int qldpc_recon_encode(qldpc_recon *r, const uint32_t *key_words, int key_bits, float qber,
                       qldpc_recon_msg *msg_out, uint32_t *parity_words, int parity_cap_words);
/* Bob: corrects key_words in place.  QLDPC_OK = decoded and CRC verified; QLDPC_EDECODE = failed,
 * key untouched.  corrected_bits / leaked_bits / iterations may be NULL. */
int qldpc_recon_decode(qldpc_recon *r, uint32_t *key_words, int key_bits, float qber, const qldpc_recon_msg *msg,
                       const uint32_t *parity_words, int *corrected_bits, int *leaked_bits, int *iterations);
/* Alice, second round (incremental redundancy): the parity bits of a plan already made -- `msg` as qldpc_recon_encode left it, with
 * n_punct lowered by the caller (0 = every parity bit of the mother code).  Same codeword, lower effective rate; Bob decodes again with
 * qldpc_recon_decode* and the new header.  The ecd2 handlers use it when a verdict asks for the withheld bits (ldpc_reconcile.c). */
int qldpc_recon_encode_planned(qldpc_recon *r, const uint32_t *key_words, int key_bits, qldpc_recon_msg *msg, uint32_t *parity_words, int cap);
/* Bob, n blocks that share one plan (same key_bits / rate / code dims) in one launch.
 * key_words[n][ceil(key_bits/32)], parity_words[n][ceil(code_m/32)] (row i holds qldpc_recon_parity_words(&msgs[i]) words),
 * status[n] = QLDPC_OK / QLDPC_EDECODE / QLDPC_ESIZE (that block's header does not match it). */
/* Alice's side for many blocks of any mix of lengths / plans in one call: every msgs[i] is planned and filled as by
 * qldpc_recon_encode, blocks are grouped by plan and encoded in launches of up to max_blocks frames. */
int qldpc_recon_encode_blocks(qldpc_recon *r, int n, const uint32_t *const *key_words, const int *key_bits, const float *qber,
                              qldpc_recon_msg *msgs, uint32_t *const *parity_words, const int *parity_cap);
int qldpc_recon_decode_batch(qldpc_recon *r, int n_blocks, uint32_t *key_words, int key_bits, const float *qber,
                             const qldpc_recon_msg *msgs, const uint32_t *parity_words, int *status,
                             int *corrected_bits, int *iterations);
/* Blocks of any mix of lengths and plans, one pointer per block (keys are decoded in place): grouped by plan and decoded in
 * launches of up to max_blocks frames; within a plan the blocks may differ in length.  status[i] = QLDPC_OK | QLDPC_EDECODE. */
int qldpc_recon_decode_blocks(qldpc_recon *r, int n, uint32_t *const *key_words, const int *key_bits, const float *qber,
                              const qldpc_recon_msg *msgs, const uint32_t *const *parity_words, int *status, int *corrected,
                              int *iterations);
/*
 * Blind (interactive) reconciliation: after a failed decode Bob names the few key positions with the smallest |a-posteriori LLR|, Alice answers with
 * her bits there (qldpc_recon_disclose_host), and Bob decodes again with those bits known -- a few bits of leak per failed block instead of the
 * withheld parity or the cascade, so that plans may sit closer to capacity.  One call = one round = qldpc_recon_decode_blocks with the positions of
 * blind[i] pinned to Alice's bits (qldpc_load_known_dev): same grouping, lanes, CRC verification, key untouched on failure; with n_known = 0 for every
 * block status, keys, corrected counts and iterations are those of qldpc_recon_decode_blocks.  The call keeps no state: the caller owns the record of
 * every block, appends the answers to pos / bit and calls again with the same messages and parity words.
 *   For a block that ends QLDPC_EDECODE, ask[0 .. n_ask) = the min(ask_bits, candidates) weakest positions (qldpc_fetch_weakest_dev) among the key
 *   positions below key_bits that are not known yet, ascending, out of that block's failed decode; every other block gets n_ask = 0.
 *   leaked[i] = qldpc_recon_leaked_bits(&msgs[i]) + n_known.  corrected[i] counts the bits that differ from the key handed in, at disclosed positions too.
 *   The key returned is the full corrected key, disclosed positions included: removing them or accounting for them is privacy amplification's business.
 * QLDPC_EINVAL: a known position repeated or not in 0 .. key_bits - 1, ask_bits < 0 (nothing is decoded).  QLDPC_EUNSUPPORTED: a session whose decoders
 * run on the edge-parallel engine (max_blocks <= 8 with the flooding schedule), or a flooding run that compacted its frames.  With QLDPC_RECON_GANG=1
 * these calls decode on the ordinary path, not through a gang.  qldpc_recon_msg and the wire format are unchanged: the request and the answer are two
 * new packets of the binding.
 */
typedef struct qldpc_recon_blind {
    int n_known, cap;      /* in: positions disclosed so far; cap = room in pos / bit (the caller's bookkeeping, not read) */
    int *pos;              /* in: distinct key positions < key_bits */
    uint8_t *bit;          /* in: Alice's bits there */
    int n_ask;             /* out */
    int *ask;              /* out on QLDPC_EDECODE: ascending positions to ask for, room for ask_bits */
} qldpc_recon_blind;
int qldpc_recon_decode_blind(qldpc_recon *r, int n, uint32_t *const *key_words, const int *key_bits, const float *qber,
                             const qldpc_recon_msg *msgs, const uint32_t *const *parity_words, qldpc_recon_blind *blind, int ask_bits,
                             int *status, int *corrected, int *iterations, int *leaked);
/* Alice's answer to a request for key bits (blind reconciliation): bit[i] = bit pos[i] of her key.  Host only.  A position outside
 * 0 .. key_bits - 1: QLDPC_EINVAL. */
int qldpc_recon_disclose_host(const uint32_t *key_words, int key_bits, const int *pos, int n, uint8_t *bit);
/*
 * Guessing rounds in a session (the rule of qldpc_guess_* below, with the session's CRC as the verdict; stated once in csrc/qldpc_recon_guess_core.h).
 * Local to Bob: nothing is disclosed, no packet is needed, qldpc_recon_msg and the wire format are unchanged.  Stateless and opt-in.
 *   first pass  exactly qldpc_recon_decode_blocks: same validation, grouping, lanes, staging and verification.  A block that ends QLDPC_OK there has the
 *               status, key, corrected and iterations of that call and guess[i] = {0, -1, 0, 0, 0, 0}.  With guess_bits = 0 (guess may be NULL), or
 *               with no failed block, the call is qldpc_recon_decode_blocks: nothing more is launched.
 *   source      a block whose first decode ends QLDPC_EDECODE (syndrome or CRC).  Its guess set is what qldpc_fetch_weakest_dev(cand, take, d =
 *               guess_bits) gives out of that failed decode, the candidates being the key positions below key_bits; its hard row is that of the
 *               same run; ranks, trials and the known / value rows are those of qldpc_guess_expand_dev.
 *   trials      the T = 2^guess_bits trial frames of a source are its own frame decoded from scratch -- the same bits, erasures, |LLR|, shortening and
 *               class map as its first decode -- plus qldpc_load_known_dev with the trial's rows.  The failed blocks of a code are pooled across the
 *               call and decoded floor(max_blocks / T) sources a launch, in ascending block index, after the ordinary launches of that code, on its
 *               lane and decoder.
 *   verdict     pass(t) = the trial's syndrome is zero && the CRC-32 of its key bits below key_bits equals msgs[i].crc32 -- what verifies a first
 *               decode.  winner = the lowest passing t; n_ok, n_pass count the zero-syndrome and the passing trials; ambiguous = some passing trial's
 *               key differs from the winner's in a bit below key_bits.  With a winner: status QLDPC_OK, the winner's key written in place, corrected
 *               counted against the key handed in, iterations = the first decode's + the winner's.  Without: QLDPC_EDECODE, the key untouched,
 *               iterations = the first decode's, corrected = 0.
 *   invariance  everything about a block is a function of the block, the session configuration and guess_bits: not of the other blocks of the call,
 *               of max_blocks (while T <= max_blocks) or of how the sources fall into trial launches.
 *   leak        qldpc_recon_leaked_bits(&msgs[i]) is unchanged: nothing is disclosed.  But the CRC now selects among up to n_ok zero-syndrome
 *               candidates, so the chance of accepting a wrong key is at most n_ok 2^-32 per block instead of 2^-32; the keyed tag is the check
 *               for callers who need a bound: qldpc_recon_decode_guess_tagged below computes it in the same call.
 * Refused before anything is decoded: QLDPC_EINVAL for a missing pointer, or guess == NULL with guess_bits > 0; QLDPC_ESIZE for guess_bits outside
 * 0 .. QLDPC_GUESS_MAX_BITS or 2^guess_bits > max_blocks (lower guess_bits or raise max_blocks); QLDPC_EUNSUPPORTED, as qldpc_recon_decode_blind, for a
 * session on the edge-parallel engine (max_blocks <= 8 with the flooding schedule) -- and, from the run, for a flooding run that compacted its frames.
 * A block with a bad header gets QLDPC_ESIZE alone.  With QLDPC_RECON_GANG=1 these calls decode on the ordinary path.  The pool of a code (sources of
 * a call and their trial frames) is device memory of its session entry, allocated by the first guessing call that uses the code and freed with it.
 *
 * qldpc_recon_guess_settle_dev is the verdict alone over device pointers (the two kernels a trial launch ends with), so that synthetic rows can be
 * settled without a decode: d_trial_rows [n_src 2^g][Wn] (qldpc_fetch_packed_dev), d_ok, d_iters [n_src 2^g] (qldpc_fetch_status_dev), d_keys
 * [n_src][Wk] the keys handed in, d_key_bits (1 .. 32 Wk: the caller's business, the kernels clamp), d_crc_want, d_first_iters [n_src] -> d_pass_out,
 * d_crc_out [n_src 2^g] = pass(t) and the CRC of every trial, d_res_keys [n_src][Wk] (words past a key's length are not written), d_res [4][n_src] =
 * status | corrected | iterations | CRC of the winner's key (of trial 0's without a winner), d_guess [n_src][6] = the ints of qldpc_recon_guess.
 * Asynchronous on hip_stream, on the current device.  qldpc_recon_guess_settle_host is its mirror on host pointers, no device needed; it also
 * refuses a key_bits outside 1 .. 32 Wk (QLDPC_ESIZE).  Both: QLDPC_EINVAL for a missing pointer, QLDPC_ESIZE for g outside 0 ..
 * QLDPC_GUESS_MAX_BITS, n_src < 0, n_src 2^g above 2^24, Wk < 1 or Wn < Wk.
 * Not built: the daemon binding (its one-block path is on the edge engine), guessing inside qldpc_recon_decode_blind, giveup_patience on the trial
 * launches, gangs, the edge engine.
 */
typedef struct qldpc_recon_guess {      /* out, per block */
    int tried;              /* 1: the block's first decode failed and its 2^g trials were decoded */
    int winner;             /* the trial kept, or -1 */
    int n_ok;               /* trials that ended with a zero syndrome */
    int n_pass;             /* of those, trials whose key bits match msgs[i].crc32 */
    int ambiguous;          /* some passing trial differs from the winner in a key bit below key_bits */
    int trial_iterations;   /* sum over the block's trials */
} qldpc_recon_guess;
int qldpc_recon_decode_guess(qldpc_recon *r, int n, uint32_t *const *key_words, const int *key_bits, const float *qber, const qldpc_recon_msg *msgs,
                             const uint32_t *const *parity_words, int guess_bits, qldpc_recon_guess *guess, int *status, int *corrected, int *iterations);
int qldpc_recon_guess_settle_dev(int g, int n_src, int Wk, int Wn, const uint32_t *d_trial_rows, const int *d_ok, const int *d_iters, const uint32_t *d_keys,
                                 const int *d_key_bits, const uint32_t *d_crc_want, const int *d_first_iters, int *d_pass_out, uint32_t *d_crc_out,
                                 uint32_t *d_res_keys, int *d_res, int *d_guess, void *hip_stream);
int qldpc_recon_guess_settle_host(int g, int n_src, int Wk, int Wn, const uint32_t *trial_rows, const int *ok, const int *iters, const uint32_t *keys,
                                  const int *key_bits, const uint32_t *crc_want, const int *first_iters, int *pass_out, uint32_t *crc_out, uint32_t *res_keys,
                                  int *res, int *guess);
/*
 * Keyed universal-hash tags inside Bob's verify step.  The CRC-32 that accepts a decoded block has no key and bounds nothing (and a guessing call lets
 * it choose among up to n_ok candidates); the hash that gives a bound is the one of qldpc_polyhash_* below, (W + 2) 2^-61 per key.  These calls
 * compute exactly that tag -- tag = k (k H + n) mod 2^61 - 1 with H the Horner value of the masked words, hi word then lo word, n_keys = r in 1 .. 4
 * values key after key -- over Bob's decoded rows where they lie on the device, in the pass that computes the CRC (csrc/qldpc_recon_tag_core.h,
 * csrc/qldpc_kernels_recon_tag.h).  Equal tags on both sides bound the chance that the keys differ; the CRC stays what it was, a cheap pre-check.
 *
 * THE HASH KEY IS THE CALLER'S AND MUST BE DRAWN AFTER THE PARITY MESSAGE HAS ARRIVED.  The library cannot check that.  Passing the key into the
 * decode call is sound for this reason: Bob holds Alice's message when he calls, so the blocks are fixed before he draws the key; he then sends the
 * key (and his tags, or their comparison) to Alice, who tags her keys with qldpc_recon_tag_blocks.
 *
 *   qldpc_recon_decode_blocks_tagged   qldpc_recon_decode_blocks -- the same validation, grouping, lanes, staging sets and pipeline, on either engine
 *               -- with the verdict kernel also hashing.  hash_keys[i] = block i's 2 n_keys key words (when all n pointers are equal the row is
 *               uploaded once a launch and shared), tag_words[i] = 2 n_keys words out.  status, keys, corrected and iterations are those of
 *               qldpc_recon_decode_blocks.  A block that ends QLDPC_OK gets the tag of the key returned; every other block (failed, or left out with
 *               QLDPC_ESIZE) gets zeros: nothing is disclosed for it.  The hash keys travel with a launch's input block and the tags with its result
 *               block; the staging of a session entry has the room from its creation, so a preloaded session allocates nothing in a call.
 *   qldpc_recon_decode_guess_tagged    qldpc_recon_decode_guess likewise (every field of qldpc_recon_guess as there): a block decoded at once is tagged
 *               by the verdict kernel, a rescued block gets the tag of the winner's key, a block still failed zeros.  guess_bits = 0 is
 *               qldpc_recon_decode_blocks_tagged.  Refusals: those of qldpc_recon_decode_guess, then those below.
 *   qldpc_recon_tag_blocks             the tags of host keys, for either side; only the length of a block matters (1 .. 2^18 bits, QLDPC_ESIZE
 *               outside), there is no plan and no message.  Launches of at most max_blocks rows through a staging block of the session (allocated
 *               with a preloaded session for blocks of up to mother_max bits, else by the first call that needs it, again when a call needs more).
 *   qldpc_recon_verify_tag_dev         the verdict kernel alone over device pointers, so that synthetic rows can be verified without a decode:
 *               d_out_rows [n][Wn] decoded rows, d_keys [n][Wk] the keys handed in, d_key_bits (1 .. 32 Wk: the caller's business, the kernel
 *               clamps), d_crc_want, d_ok, d_iters [n], d_hash_keys rows of 2 n_keys words hash_key_stride words apart (0: every block reads row
 *               0) -> d_res_keys [n][Wk] (words past a key's length are not written), d_res [4][n] = status | corrected | iterations | CRC found,
 *               d_tags [n][2 n_keys].  Asynchronous on hip_stream, on the current device.  qldpc_recon_verify_tag_host is its mirror on host
 *               pointers, no device needed; it also refuses a key_bits outside 1 .. 32 Wk.  Both: QLDPC_ESIZE for n < 0, Wk < 1, Wn < Wk or a
 *               stride in 1 .. 2 n_keys - 1.
 *   qldpc_recon_tag_host               one tag of one block under one key by the kernels' decomposition with `lanes` lanes (a power of two; the
 *               kernels: 256): equal to qldpc_polyhash_host for every such lanes.
 *   qldpc_recon_leaked_bits_tagged     qldpc_recon_leaked_bits(msg) + 61 n_keys: the conservative account, charging both the CRC and the tags;
 *               0 on a bad argument.
 * Argument checks run before anything is queued or written, and qldpc_last_error() names the block: n_keys outside 1 .. 4, a NULL hash_keys[i] or
 * tag_words[i] (or array) are QLDPC_EINVAL.
 * Left out on purpose: tags in qldpc_recon_decode_blind, qldpc_recon_decode_batch and the one-block qldpc_recon_decode; a tag field in qldpc_recon_msg;
 * the daemon packet; a one-time pad of the tag; gangs (with QLDPC_RECON_GANG=1 a tagged call decodes on the ordinary lanes, as the blind and guessing
 * calls do).
 */
int qldpc_recon_decode_blocks_tagged(qldpc_recon *r, int n, uint32_t *const *key_words, const int *key_bits, const float *qber, const qldpc_recon_msg *msgs,
                                     const uint32_t *const *parity_words, int n_keys, const uint32_t *const *hash_keys, uint32_t *const *tag_words,
                                     int *status, int *corrected, int *iterations);
int qldpc_recon_decode_guess_tagged(qldpc_recon *r, int n, uint32_t *const *key_words, const int *key_bits, const float *qber, const qldpc_recon_msg *msgs,
                                    const uint32_t *const *parity_words, int guess_bits, qldpc_recon_guess *guess, int n_keys,
                                    const uint32_t *const *hash_keys, uint32_t *const *tag_words, int *status, int *corrected, int *iterations);
int qldpc_recon_tag_blocks(qldpc_recon *r, int n, const uint32_t *const *key_words, const int *key_bits, int n_keys, const uint32_t *const *hash_keys,
                           uint32_t *const *tag_words);
int qldpc_recon_verify_tag_dev(int n, int n_keys, int Wk, int Wn, const uint32_t *d_out_rows, const uint32_t *d_keys, const int *d_key_bits,
                               const uint32_t *d_crc_want, const int *d_ok, const int *d_iters, const uint32_t *d_hash_keys, size_t hash_key_stride,
                               uint32_t *d_res_keys, int *d_res, uint32_t *d_tags, void *hip_stream);
int qldpc_recon_verify_tag_host(int n, int n_keys, int Wk, int Wn, const uint32_t *out_rows, const uint32_t *keys, const int *key_bits, const uint32_t *crc_want,
                                const int *ok, const int *iters, const uint32_t *hash_keys, size_t hash_key_stride, uint32_t *res_keys, int *res, uint32_t *tags);
int qldpc_recon_tag_host(const uint32_t *key_words, int key_bits, const uint32_t hash_key[2], int lanes, uint32_t tag[2]);
int qldpc_recon_leaked_bits_tagged(const qldpc_recon_msg *msg, int n_keys);
/*
 * Bob's QBER estimate of every block out of its parity message (qldpc_qber_* below), before anything is decoded: the blocks are validated, grouped by
 * code and assembled into frames exactly as qldpc_recon_decode_blocks does it (key VNs channel, shortened past key_bits, disclosed parity pinned,
 * punctured parity erased), and each group goes through the estimator of its session entry (one per entry, created with the entry when the session
 * preloads, else at the first call that needs it) in launches of up to max_blocks frames.  qber_out[i] = the estimate of block i (0 for a block with
 * no informative check, or whose header does not match: those are left out), usable as the `qber` of the decode calls; counts_out (optional) =
 * [n][QLDPC_QBER_MAX_DEGREE + 1][2] uint32, block i's counts by effective degree, rows past its code's largest check degree zero; *pool_qber_out
 * (optional) = the estimate from the counts of all blocks of the call summed, whatever their codes (0 if there is none).  Keys are not touched; the
 * grid is the default one of qldpc_qber_cfg_default.  The call returns when the results are in place.
 */
int qldpc_recon_estimate_blocks(qldpc_recon *r, int n, const uint32_t *const *key_words, const int *key_bits, const qldpc_recon_msg *msgs,
                                const uint32_t *const *parity_words, float *qber_out, uint32_t *counts_out, float *pool_qber_out);
/* The same with runs of checks across punctured parity bits merged into one observation each (qldpc_qber_set_merge below): every session entry keeps a
 * merged estimator beside its plain one.  A block whose plan punctures half of its parity or more gets 0 from the call above (one informative check
 * is left at most) and an estimate from this one.  counts_out rows run to QLDPC_QBER_MAX_DEGREE for every code. */
int qldpc_recon_estimate_blocks_merged(qldpc_recon *r, int n, const uint32_t *const *key_words, const int *key_bits, const qldpc_recon_msg *msgs,
                                       const uint32_t *const *parity_words, float *qber_out, uint32_t *counts_out, float *pool_qber_out);
uint32_t qldpc_crc32_words(const uint32_t *words, int n_bits);
/* The same CRC-32 the way the device verification computes it (rk_verify / rk_crc in qldpc_recon.hip): `lanes` (a power of two) equal
 * chunks, each run through the byte-wise recurrence from a zero register, folded pairwise with x^len multipliers mod the CRC polynomial,
 * start value and final inversion applied at the end.  Host mirror for tests: equals qldpc_crc32_words for every length. */
uint32_t qldpc_crc32_words_chunked(const uint32_t *words, int n_bits, int lanes);

/* ------------------------------------------------------------------ QBER from the syndrome weight ---- */
/*
 * Bob's own estimate of a frame's QBER out of the parity message, at no extra disclosed bit and before the first BP iteration (no reference counterpart:
 * the reference samples disclosed bits, subcomponents/qber_estim.c).  The rule is stated once, in csrc/qldpc_qber_core.h:
 *
 *   A VN of a frame is KNOWN-EXACT (its known bit is set -- value from the value row, known wins over erased --, or class QLDPC_VN_PINNED, or class
 *   QLDPC_VN_CHANNEL at index >= n_channel[f]), ERASED (class QLDPC_VN_PUNCTURED or its erase bit set, and not known) or NOISY (the rest): what
 *   qldpc_load_bits_short_dev, qldpc_load_erasures_dev and qldpc_load_known_dev mean.  A check is INFORMATIVE iff none of its VNs is erased; its
 *   effective degree d = the number of its noisy VNs, its outcome u = s_c ^ XOR of the values of all its VNs (s_c = 0 without a syndrome row).
 *   counts[f][d][0] = informative checks of frame f with effective degree d, counts[f][d][1] = those with u = 1; d = 0 .. D = qldpc_code_max_cn_degree
 *   (row 0: an unsatisfied check without a noisy VN is an inconsistency; the score ignores the row).
 *   With d noisy neighbours of flip probability q a check comes out 1 with p_d(q) = (1 - (1 - 2 q)^d) / 2.  On the grid q_k = q_lo (q_hi / q_lo)^(k / (n_grid - 1))
 *   the score is S_k = SUM_{d >= 1} u_d L1[d][k] + (n_d - u_d) L0[d][k] in int64 with L1 = llround(log p_d(q_k) 2^24), L0 = llround(log(1 - p_d(q_k)) 2^24)
 *   (int32 tables built on the host in double; the device takes no logarithm).  The estimate is the smallest k with maximal S_k, a full scan: integer scores
 *   make host and device agree exactly.  A frame without an informative check of degree >= 1: index -1, QBER 0, |LLR| 0; every check satisfied: k = 0.
 *   The POOLED estimate of a call is the same argmax over the sum of its frames' counts.
 *
 * A check next to an erased VN is left out -- unless MERGING is turned on (qldpc_qber_set_merge; off by default, and then nothing changes).  It needs a
 * code whose parity part is an accumulator chain: K = N - M, VN K + c on exactly checks c and c + 1 for c < M - 1, VN K + M - 1 on check M - 1 only, no
 * other VN >= K in any row (verified edge by edge; QLDPC_EUNSUPPORTED otherwise, the reason in qldpc_last_error()).  VN K + c, c < M - 1, of a frame is a
 * LINK iff it is erased in that frame; a RUN is a maximal set of consecutive checks h .. t joined by links.  A run of one check is counted as above.  A run
 * of two or more is one observation: the checks on the two sides of an erased chain VN add up to a parity equation without it, so u = XOR over the run's
 * checks of s_c and of the values of all their VNs but the links, d = the number of noisy VNs with an odd number of edges into the run (a VN shared by two
 * checks of the run cancels in u and does not count).  A run is left out when it holds an erased VN other than its own links (an erased VN K + M - 1
 * included; an erased VN that occurs twice in the run is not cancelled), when it has more than 16 checks, or when d > QLDPC_QBER_MAX_DEGREE.  With merging
 * on the counts have QLDPC_QBER_MAX_DEGREE + 1 rows whatever D (qldpc_qber_count_rows) and the score tables run to that degree; score, argmax and pool are
 * the same.  With half of the parity punctured at even spacing the unmerged rule is left with one check and the merged one with M / 2 runs of two.
 * Noisy disclosed parity, table / soft channels, non-chain codes and estimates from a decoder's ballots mid-run are not built.
 *
 * qldpc_qber_create: QLDPC_EINVAL for n_grid outside 2 .. 1 024, q_lo < 1e-6, q_lo >= q_hi, q_hi >= 0.5, max_frames outside 1 .. 65 535; QLDPC_EUNSUPPORTED
 * for a check degree above QLDPC_QBER_MAX_DEGREE or max_frames x M >= 2^35 (the pooled score could overflow); QLDPC_ENODEV without a device.
 * checks_per_block: checks a workgroup of the counting kernel covers (256 threads, a thread per check and pass; 0 = chosen per call from the frame count) -- tests
 * force many partial histograms per frame with it.  The counting kernel stages a frame's rows in LDS while 3 ceil(N / 32) words fit (N up to about
 * 390 000) and gathers from memory above; QLDPC_QBER_STAGE=0 in the environment at creation takes the memory path whatever the size (tests, A/B).
 */
#define QLDPC_QBER_MAX_DEGREE 63
typedef struct qldpc_qber qldpc_qber;
typedef struct qldpc_qber_cfg {
    int device;
    int max_frames;        /* capacity of one call */
    int n_grid;            /* 256 */
    float q_lo, q_hi;      /* 0.001, 0.25: the clamp qldpc_recon_plan applies */
    int checks_per_block;  /* 0 = auto */
} qldpc_qber_cfg;
void   qldpc_qber_cfg_default(qldpc_qber_cfg *cfg);
int    qldpc_qber_create(const qldpc_code *code, const qldpc_qber_cfg *cfg, qldpc_qber **out);
void   qldpc_qber_free(qldpc_qber *est);
size_t qldpc_qber_device_bytes(const qldpc_qber *est);
/* NULL = the null stream.  A switch to another stream orders it after everything the estimator has queued on the old one, its own count rows included;
 * the same stream again does nothing (the stream switch, qldpc_decoder_set_stream) */
int    qldpc_qber_set_stream(qldpc_qber *est, void *hip_stream);
/* Merging on (non-zero) or off, between calls.  The first call that turns it on verifies the chain (QLDPC_EUNSUPPORTED for any other code), builds and
 * uploads the repeat table (a byte per edge) and replaces the score tables and the estimator's own count rows by ones of QLDPC_QBER_MAX_DEGREE + 1 rows; it
 * synchronises the device.  qldpc_qber_count_rows = the rows of d_counts / d_pool_counts as the estimator stands: D + 1, with merging on
 * QLDPC_QBER_MAX_DEGREE + 1. */
int    qldpc_qber_set_merge(qldpc_qber *est, int on);
int    qldpc_qber_count_rows(const qldpc_qber *est);
/* q[n_grid] / llr[n_grid] (either may be NULL) = the grid and qldpc_bsc_llr of it; returns n_grid */
int    qldpc_qber_grid(const qldpc_qber *est, float *q, float *llr);
/*
 * Asynchronous on the estimator's stream.  Inputs as the loads take them: d_bits[n_frames][ceil(N/32)], d_vn_class[N] (NULL = all channel), d_n_channel[n_frames]
 * (NULL = N), d_synd_bits[n_frames][ceil(M/32)] (NULL = zero syndrome), d_erase_bits / d_known_bits / d_value_bits [n_frames][ceil(N/32)] (NULL = none; known
 * needs value).  Outputs, each may be NULL: d_counts[n_frames][rows][2] uint32 (cleared on the stream first; rows = qldpc_qber_count_rows: D + 1, merged
 * QLDPC_QBER_MAX_DEGREE + 1), d_index[n_frames] (grid index or -1),
 * d_qber[n_frames] (q_k), d_llr_mag[n_frames] (qldpc_bsc_llr(q_k): can be handed to qldpc_load_bits_dev / _short_dev on the same stream),
 * d_pool_counts[rows][2] uint64, d_pool_index[1].  An estimator is not re-entrant.  QLDPC_EINVAL: n_frames < 1 or > max_frames.
 */
int    qldpc_qber_estimate_dev(qldpc_qber *est, const uint32_t *d_bits, const uint8_t *d_vn_class, const int *d_n_channel, const uint32_t *d_synd_bits,
                               const uint32_t *d_erase_bits, const uint32_t *d_known_bits, const uint32_t *d_value_bits, int n_frames,
                               uint32_t *d_counts, int *d_index, float *d_qber, float *d_llr_mag, uint64_t *d_pool_counts, int *d_pool_index);
/* Host mirrors, no device needed (csrc/qldpc_qber_host.c over the functions the kernels run).  Tables: L1 / L0 [max_degree + 1][n_grid] (row 0 zero),
 * q / llr [n_grid]; each may be NULL.  Counts of ONE frame: rows of that frame, n_channel its count (N = none), counts[D + 1][2].  Argmax: counts as
 * uint64 [max_degree + 1][2], *index = the estimate or -1. */
int    qldpc_qber_table_host(int max_degree, int n_grid, float q_lo, float q_hi, int32_t *L1, int32_t *L0, float *q, float *llr);
int    qldpc_qber_counts_host(const qldpc_code *code, const uint32_t *bits, const uint8_t *vn_class, int n_channel, const uint32_t *synd,
                              const uint32_t *erase, const uint32_t *known, const uint32_t *value, uint32_t *counts);
int    qldpc_qber_argmax_host(const uint64_t *counts, int max_degree, int n_grid, const int32_t *L1, const int32_t *L0, int *index);
/* The merged count of ONE frame, arguments as qldpc_qber_counts_host, counts[QLDPC_QBER_MAX_DEGREE + 1][2]; QLDPC_EUNSUPPORTED for a code that is no chain.
 * qldpc_qber_repeat_table_host: the chain test and the repeat table both sides use, on the transposed check table tab[D][M] (tab[j][c] = VN of slot j of
 * check c, -1 past its degree): rep[D][M] (NULL = test only) = for every edge the distance back to the nearest earlier check within 15 that holds the
 * same VN, or 0. */
int    qldpc_qber_counts_merged_host(const qldpc_code *code, const uint32_t *bits, const uint8_t *vn_class, int n_channel, const uint32_t *synd,
                                     const uint32_t *erase, const uint32_t *known, const uint32_t *value, uint32_t *counts);
int    qldpc_qber_repeat_table_host(const int *tab, int N, int M, int D, uint8_t *rep);

/* ------------------------------------------------------------------ privacy amplification ---- */
/*
 * The hash loop of privAmp_doPrivAmp (subcomponents/priv_amp.c:213-218) with the LFSR word stream of
 * rnd_getPrngValue2_32 (subcomponents/rnd.c:118-127, feedback 0xe0000200): final key bit i =
 * parity(XOR_j key[j] & w[i*numwords + j]).  key = mainBufPtr words (bits past workbits are ignored),
 * seed = EcPktHdr_StartPrivAmp.seed (definitions/packets.h:170-175), out = ceil(final_bits/32) words.
 * Pure integer arithmetic: bit-identical to the reference.
 */
int qldpc_privamp(int device, const uint32_t *key_words, int workbits, uint32_t seed, int final_bits, uint32_t *final_words);
/* device pointers; the key's tail bits past workbits must already be zero */
int qldpc_privamp_dev(const uint32_t *d_key_words, int workbits, uint32_t seed, int final_bits, uint32_t *d_final_words, void *hip_stream);

/*
 * The same hash for a batch of blocks in one launch (csrc/qldpc_privamp_batch.hip).  With A one word step of the LFSR and R = A^numwords,
 * final key bit i = parity(v_key & R^i seed) where v_key = XOR_j (A^T)^(j+1) key[j] is a 32-bit functional of the key: O(numwords +
 * final_bits) work per block, no bound from the LDS and none at 2^17 final bits.  Bit-identical to qldpc_privamp and to the reference.
 *
 * qldpc_privamp_create allocates everything (pinned staging, device buffers for max_blocks blocks of max_key_bits -> max_final_bits bits,
 * descriptor rows, the jump tables, which are built on the device per call, one per distinct key length); no call afterwards allocates.
 * max_key_bits and max_final_bits may each be up to 2^24 and max_blocks up to 65 535 (QLDPC_ESIZE above, and when max_blocks x the two row
 * lengths pass 2^31 words).  The packed key and output areas of the host form (max_blocks rows of max_key_bits / max_final_bits, pinned and
 * on the device) are allocated whichever form is used afterwards: a caller of qldpc_privamp_blocks_dev alone pays for them too.
 * final_bits[i] may exceed workbits[i]; final_bits[i] == 0 leaves block i alone; n == 0 is QLDPC_OK.  A bad argument in any block
 * (NULL row: QLDPC_EINVAL; workbits <= 0, final_bits < 0, a value over the context's sizes, n > max_blocks: QLDPC_ESIZE) refuses the
 * whole call before any work is queued, and qldpc_last_error() names the block.  A context is not re-entrant; a call first waits for the
 * previous call on the same context to have run (its descriptor rows are reused).
 */
typedef struct qldpc_privamp_ctx qldpc_privamp_ctx;
int  qldpc_privamp_create(int device, int max_blocks, int max_key_bits, int max_final_bits, qldpc_privamp_ctx **out);
void qldpc_privamp_free(qldpc_privamp_ctx *pa);
size_t qldpc_privamp_device_bytes(const qldpc_privamp_ctx *pa);
/* host buffers, n <= max_blocks blocks of any mix of lengths; key tail bits past workbits[i] are ignored (priv_amp.c:196-198) */
int qldpc_privamp_blocks(qldpc_privamp_ctx *pa, int n, const uint32_t *const *key_words, const int *workbits,
                         const uint32_t *seeds, const int *final_bits, uint32_t *const *final_words);
/* device-resident keys and outputs, rows key_stride / out_stride words apart; workbits / seeds / final_bits are host arrays;
   asynchronous on hip_stream; writes exactly ceil(final_bits[i]/32) words of row i */
int qldpc_privamp_blocks_dev(qldpc_privamp_ctx *pa, int n, const uint32_t *d_keys, size_t key_stride, const int *workbits,
                             const uint32_t *seeds, const int *final_bits, uint32_t *d_out, size_t out_stride, void *hip_stream);
/* host mirrors of the two halves, for tests: the key fold in `lanes` equal chunks (any lanes >= 1 gives the same value; 0 on a bad
   argument), and the expansion of a functional into the final key words */
uint32_t qldpc_privamp_key_functional(const uint32_t *key_words, int workbits, int lanes);
int qldpc_privamp_expand_host(uint32_t functional, int workbits, uint32_t seed, int final_bits, uint32_t *final_words);

/* ------------------------------------------------------------------ Toeplitz-hash privacy amplification ---- */
/*
 * The hash of qldpc_privamp* keeps the reference's wire behaviour and with it 32 bits of the key.  This is the hash a
 * deployment needs: Toeplitz hashing, whose every output bit reads the whole key and which carries the leftover-hash guarantee.  For a
 * block of key_bits = n >= 1, out_bits = m >= 0 and seed bits t_0 .. t_(n+m-2)
 *
 *     y_i = XOR_{j < n} x_j t_(i+j)        i = 0 .. m-1
 *
 * x_j = bit j of key_words and t_k = bit k of seed_words, both MSB-first (word[j/32] & (1u << (31 - j%32)), helpers.h:65-70); key bits
 * at index >= n and seed bits at index >= n + m - 1 are ignored; y is written MSB-first into ceil(m/32) words, the unused low bits of
 * the last word zero.  This is T reverse(x) with the Toeplitz matrix T[i][j] = t[i - j + n - 1]: the same 2-universal family, indexed so
 * that output bit i reads one contiguous window of t.  m may exceed n; m == 0 leaves the block alone; n and m are at most 2^24.
 *
 * THE SEED IS THE CALLER'S.  The library makes none: the caller supplies n + m - 1 uniformly random bits per block
 * (qldpc_toeplitz_seed_words words).  They may be public and the blocks of a call may share them.  The guarantee of the hash is the
 * quality of that seed and nothing the library can check.
 *
 * An n x m GF(2) matrix-vector product per block, on the device, all blocks of a call in one launch (csrc/qldpc_toeplitz.hip).
 * Conventions as qldpc_privamp_create / _blocks / _blocks_dev: qldpc_toeplitz_create allocates everything (pinned staging and device rows
 * for max_blocks keys, seeds and outputs, descriptor rows), whichever form is used afterwards, and no call afterwards allocates;
 * max_blocks up to 65 535, max_key_bits and max_out_bits up to 2^24 (QLDPC_ESIZE above, for max_blocks <= 0, and when max_blocks x the
 * row lengths pass 2^31 words).  A bad argument in any block (NULL row: QLDPC_EINVAL; key_bits <= 0, out_bits < 0, a value over the
 * context's sizes, n > max_blocks: QLDPC_ESIZE) refuses the whole call before any work is queued, and qldpc_last_error() names the block.
 * n == 0 is QLDPC_OK.  A context is not re-entrant; a call first waits for the previous call on the same context to have run.
 */
typedef struct qldpc_toeplitz_ctx qldpc_toeplitz_ctx;
/* ceil((key_bits + out_bits - 1) / 32); 0 for out_bits <= 0 or key_bits <= 0 */
size_t qldpc_toeplitz_seed_words(int key_bits, int out_bits);
int    qldpc_toeplitz_create(int device, int max_blocks, int max_key_bits, int max_out_bits, qldpc_toeplitz_ctx **out);
void   qldpc_toeplitz_free(qldpc_toeplitz_ctx *tz);
size_t qldpc_toeplitz_device_bytes(const qldpc_toeplitz_ctx *tz);
/* host buffers, n <= max_blocks blocks of any mix of lengths.  When all n seed_words pointers are equal the seed is uploaded once and
   shared (the row then covers the longest key_bits + out_bits - 1 of the call); otherwise once per block */
int    qldpc_toeplitz_blocks(qldpc_toeplitz_ctx *tz, int n, const uint32_t *const *key_words, const int *key_bits,
                             const uint32_t *const *seed_words, const int *out_bits, uint32_t *const *out_words);
/* device-resident rows key_stride / seed_stride / out_stride words apart (seed_stride 0: every block reads row 0); key_bits / out_bits are
   host arrays; asynchronous on hip_stream; writes exactly ceil(out_bits[i]/32) words of row i */
int    qldpc_toeplitz_blocks_dev(qldpc_toeplitz_ctx *tz, int n, const uint32_t *d_keys, size_t key_stride, const int *key_bits,
                                 const uint32_t *d_seeds, size_t seed_stride, const int *out_bits,
                                 uint32_t *d_out, size_t out_stride, void *hip_stream);
/* host mirror, for tests: the kernel's own window / fold functions (csrc/qldpc_toeplitz_core.h), the key consumed in tiles of tile_words
   (0 = the kernel's tile; every tile size gives the same words) */
int    qldpc_toeplitz_host(const uint32_t *key_words, int key_bits, const uint32_t *seed_words, int out_bits, int tile_words, uint32_t *out_words);

/*
 * The sub-quadratic method.  The product above is a correlation: over the integers c_i = SUM_j x_j t_(i+j) <= n <= 2^24 and y_i = c_i mod 2,
 * so a number-theoretic transform over the prime p = 15 * 2^27 + 1 = 2 013 265 921 > 2^24 computes it exactly: three transforms of length
 * L = qldpc_toeplitz_ntt_length(n, m) in place of n m bit-products, and the SAME WORDS as the direct method, bit for bit
 * (csrc/qldpc_toeplitz_ntt.hip, csrc/qldpc_toeplitz_ntt_core.h).  A context is built for one method by qldpc_toeplitz_create_cfg and
 * is then used through qldpc_toeplitz_blocks / _blocks_dev with the checks, refusals and stream semantics stated above; with
 * QLDPC_TOEPLITZ_NTT the blocks of a call are grouped by their L, blocks of equal L share launches, and a seed the call shares (all
 * seed_words pointers equal, or seed_stride == 0) is transformed once per distinct L from the first min(L, 32 x the longest
 * qldpc_toeplitz_seed_words of the call) bits of its row.  The words do not depend on the grouping, on rounds or on pass_log2.
 *
 * There is no automatic choice of method: where the two cross has not been decided in the library (tools/toeplitz_cost.py measures both in
 * one process; README).  qldpc_toeplitz_create builds the direct method.
 */
#define QLDPC_TOEPLITZ_DIRECT 0
#define QLDPC_TOEPLITZ_NTT 1
#define QLDPC_TOEPLITZ_PASS_LOG2 9         /* B of the production pass kernels: a transform of length 2^k runs as ceil(k / B) passes */
#define QLDPC_TOEPLITZ_PASS_LOG2_SMALL 5   /* B of the small instance, which reaches every pass structure at test sizes */
typedef struct {
    int device, max_blocks, max_key_bits, max_out_bits;      /* as qldpc_toeplitz_create takes them */
    int method;                /* QLDPC_TOEPLITZ_DIRECT / QLDPC_TOEPLITZ_NTT; anything else QLDPC_EINVAL */
    int pass_log2;             /* NTT: 0 = the production instance, QLDPC_TOEPLITZ_PASS_LOG2_SMALL = the small one; anything else QLDPC_EINVAL */
    size_t work_bytes;         /* NTT: the work area, two arrays of L 32-bit residues per block in flight (key and seed spectrum).  0 = room for all
                                  max_blocks at L = qldpc_toeplitz_ntt_length(max_key_bits, max_out_bits) where that is <= 1 GiB, else as many
                                  blocks as fit in 1 GiB, and never less than one; a value below one block (8 L bytes) is QLDPC_ESIZE.  A call
                                  with more blocks of one L than fit runs them in rounds */
} qldpc_toeplitz_cfg;
/* max_blocks 64, 2^16 key and output bits, the direct method, device 0 */
void   qldpc_toeplitz_cfg_default(qldpc_toeplitz_cfg *cfg);
/* allocates everything, the work area and the twiddle tables included (qldpc_toeplitz_device_bytes counts them); no call afterwards allocates.
   qldpc_toeplitz_create is this with the defaults and its four arguments */
int    qldpc_toeplitz_create_cfg(const qldpc_toeplitz_cfg *cfg, qldpc_toeplitz_ctx **out);
/* the transform length of a block: the smallest power of two >= key_bits + out_bits - 1, and at least 32 (an output word is stored whole);
   0 where qldpc_toeplitz_seed_words gives 0, and for sizes over 2^24 */
size_t qldpc_toeplitz_ntt_length(int key_bits, int out_bits);
/* the last call of the context: out[0] kernel launches, [1] forward transforms, [2] inverse transforms, [3] rounds, [4] distinct L,
   [5] the largest L, [6..7] 0.  A direct context reports one launch and zeros */
int    qldpc_toeplitz_stats(const qldpc_toeplitz_ctx *tz, uint64_t out[8]);
/* host mirror of the NTT method, for tests: no device; the core header's functions over the same tiles and passes as the kernels, with
   B = pass_log2 (0 = QLDPC_TOEPLITZ_PASS_LOG2; every value 1 .. 25 gives the same words; anything else QLDPC_EINVAL) */
int    qldpc_toeplitz_ntt_host(const uint32_t *key_words, int key_bits, const uint32_t *seed_words, int out_bits, int pass_log2, uint32_t *out_words);
/* the field arithmetic, for tests: a b mod p, and a primitive 2^log2_len-th root of unity (log2_len 0 .. 25, else 0) */
uint32_t qldpc_toeplitz_ntt_mul_host(uint32_t a, uint32_t b);
uint32_t qldpc_toeplitz_ntt_root_host(int log2_len);

/* ------------------------------------------------------------------ error verification by a universal hash ---- */
/*
 * After a decode the two sides must learn whether their keys are equal.  The CRC-32 of the sessions (qldpc_recon_*) is a cheap pre-check with
 * a fixed public polynomial: it has no key and bounds nothing.  This is the hash the correctness term of a security statement needs:
 * polynomial evaluation over the Mersenne prime p = 2^61 - 1 (csrc/qldpc_polyhash_core.h, csrc/qldpc_polyhash.hip).  A block of
 * key_bits = n >= 1 bits in W = ceil(n / 32) words (MSB-first; the bits past n in the last word are ignored) has the coefficients
 * c_0 .. c_(W-1), its words with the tail masked, and c_W = n, and
 *
 *     tag = SUM_{j = 0 .. W} c_j k^(W+1-j) mod p          (as Horner: h = 0; for every c: h = (h + c) k mod p)
 *
 * canonical in [0, p), written as two words: hi (29 bits), then lo.  The length is a coefficient, so zero padding cannot collide.  With
 * n_keys = r in 1 .. 4 independent keys per block the tag is r such values, 2 r words, key after key.
 *
 * THE KEY IS THE CALLER'S.  The library makes none: the caller supplies two words (hi, lo) per key, k = ((hi << 32) | lo) & p with the
 * value p itself taken as 0, so every 64-bit pattern is a valid key.  The guarantee is the quality of those bits and the moment they are
 * chosen (after the adversary can no longer influence the blocks) and nothing the library can check.  Two different (n, message) pairs give
 * equal tags with probability at most (W + 2) 2^-61 per key, W of the longer one (a non-zero polynomial of degree <= W + 1; field value 0
 * has probability 2^-60 and every other 2^-61), to the power r for r keys: qldpc_polyhash_bound_log2.  A tag discloses at most 61 r bits of
 * the block: qldpc_polyhash_leaked_bits.
 *
 * Conventions as qldpc_toeplitz_create_cfg / _blocks / _blocks_dev: creation allocates everything (pinned staging, device rows, descriptor
 * rows and the work area of the blocks that span several tiles) and no call afterwards allocates; max_blocks up to 65 535, max_key_bits up
 * to 2^24 (QLDPC_ESIZE above, for values < 1, and when max_blocks x the row lengths pass 2^31 words); n_keys outside 1 .. 4 and a
 * tile_words other than 0 and the two values below are QLDPC_EINVAL.  A bad argument in any block (NULL row: QLDPC_EINVAL; key_bits <= 0 or
 * over the context's, n > max_blocks, a device row shorter than its block: QLDPC_ESIZE) refuses the whole call before any work is queued,
 * and qldpc_last_error() names the block.  n == 0 is QLDPC_OK.  A context is not re-entrant; a call first waits for the previous call on
 * the same context to have run.  All blocks of a call go in one launch; a block of more than tile_words coefficients is split over
 * several workgroups, and a second launch on the same stream then folds their partials.  The tag does not depend on tile_words.
 *
 * The sessions compute the same tag inside Bob's verify step, over his decoded rows where they lie on the device: qldpc_recon_decode_blocks_tagged,
 * qldpc_recon_decode_guess_tagged and qldpc_recon_tag_blocks above.
 * Not built: qldpc_recon_msg carrying a tag, the daemon packet, a one-time pad of the tag, GF(2^128) families, truncated tags.
 */
#define QLDPC_POLYHASH_PRIME 0x1FFFFFFFFFFFFFFFull
#define QLDPC_POLYHASH_TILE_WORDS 8192         /* coefficients per workgroup of the production instance */
#define QLDPC_POLYHASH_TILE_WORDS_SMALL 1024   /* of the small instance, which reaches every multi-tile structure at test sizes */
typedef struct qldpc_polyhash_ctx qldpc_polyhash_ctx;
typedef struct {
    int device, max_blocks, max_key_bits;
    int n_keys;                /* independent keys per block, 1 .. 4 */
    int tile_words;            /* 0 = QLDPC_POLYHASH_TILE_WORDS; QLDPC_POLYHASH_TILE_WORDS_SMALL = the small instance */
} qldpc_polyhash_cfg;
/* max_blocks 64, 2^16 key bits, one key, the production tile, device 0 */
void   qldpc_polyhash_cfg_default(qldpc_polyhash_cfg *cfg);
int    qldpc_polyhash_create_cfg(const qldpc_polyhash_cfg *cfg, qldpc_polyhash_ctx **out);
void   qldpc_polyhash_free(qldpc_polyhash_ctx *ph);
size_t qldpc_polyhash_device_bytes(const qldpc_polyhash_ctx *ph);
/* host buffers, n <= max_blocks blocks of any mix of lengths; hash_keys[i]: the 2 n_keys words of block i's keys, tag_words[i]: 2 n_keys
   words.  When all n hash_keys pointers are equal the row is uploaded once and shared */
int    qldpc_polyhash_blocks(qldpc_polyhash_ctx *ph, int n, const uint32_t *const *key_words, const int *key_bits,
                             const uint32_t *const *hash_keys, uint32_t *const *tag_words);
/* device-resident rows key_stride / hash_key_stride / tag_stride words apart (hash_key_stride 0: every block reads row 0); key_bits is a
   host array; asynchronous on hip_stream; writes exactly 2 n_keys words of row i */
int    qldpc_polyhash_blocks_dev(qldpc_polyhash_ctx *ph, int n, const uint32_t *d_keys, size_t key_stride, const int *key_bits,
                                 const uint32_t *d_hash_keys, size_t hash_key_stride, uint32_t *d_tags, size_t tag_stride, void *hip_stream);
/* n_keys (log2(W + 2) - 61): log2 of the bound above; 0 on a bad argument */
double qldpc_polyhash_bound_log2(int key_bits, int n_keys);
/* 61 n_keys; 0 on a bad argument */
int    qldpc_polyhash_leaked_bits(int n_keys);
/* host mirror, for tests: no device; the core header's functions over the kernels' own decomposition with `lanes` lanes per workgroup (the
   kernels: 256) and tiles of tile_words (as in the configuration).  Every lanes >= 1 and either tile give the same tag */
int    qldpc_polyhash_host(const uint32_t *key_words, int key_bits, const uint32_t hash_key[2], int lanes, int tile_words, uint32_t tag[2]);
/* the field arithmetic, for tests: a b mod p for any a, b, and the field element of a key's two words */
uint64_t qldpc_polyhash_mul_host(uint64_t a, uint64_t b);
uint64_t qldpc_polyhash_key_host(uint32_t hi, uint32_t lo);

/* ------------------------------------------------------------------ Monte-Carlo FER loop ---- */
/*
 * The loop of the reference harness -- source -> encoder -> BSC -> decoder -> monitor (BS/src/main.cpp:335-393, Monitor_BFER's max_fe stop
 * rule) -- with nothing per bit crossing the host (csrc/qldpc_mc.hip).  Frame number i is a 64-bit GLOBAL index and its content a pure
 * function of (seed, i) (csrc/qldpc_mc_core.h): it does not depend on the batch size, the launch shape or the device, so ranks and batches
 * take disjoint index ranges and a failed frame can be generated again alone.  The channel is the BSC below unless qldpc_mc_set_channel set a
 * table of a quantised soft-output channel (further down).
 *
 *   generator  Philox4x32-10, key = (seed low word, seed high word)
 *   source     info word j of frame i = output word j % 4 at counter (j / 4, 0, i_lo, i_hi), MSB-first, the bits past K cleared
 *   channel    VN v of frame i flips iff u < T[class(v)], u = output word v % 4 at counter (v / 4, 1, i_lo, i_hi), T = floor(p 2^32) in
 *              double on the host with p = qber (QLDPC_VN_CHANNEL), parity_ber (QLDPC_VN_PINNED: dirty disclosed parity, 0 = exact) or
 *              0 (QLDPC_VN_PUNCTURED); rx = cw ^ flips.  A flip probability is exactly T / 2^32.
 *
 * vn_class (a HOST array of N classes) may be NULL: the harness's classes, QLDPC_VN_CHANNEL at info_bits_pos and QLDPC_VN_PINNED elsewhere.
 * Status codes as everywhere: QLDPC_ESIZE for qber outside (0, 0.5) in qldpc_mc_run and outside [0, 1) in the frame calls, for a batch above
 * the decoder's max_frames and for fail_cap < 1; QLDPC_ENODEV without a device.  qldpc_mc_run has no CPU fallback.  Everything is queued on
 * the decoder's stream; one object is not re-entrant.  Not built: a random puncture pattern per frame, sessions / gangs as the decoder under
 * test, a multi-GPU driver (first_frame makes sharding the caller's loop).
 *
 * Puncture patterns and the search over them (BS/src/main.cpp:235-411: shuffle the parity positions, erase the first bits_to_puncture of the
 * shuffle -- LLRs[pattern[i]] = 0 --, simulate, keep the first shuffle that goes through with FER = 0 / n).  Pattern p (a 64-bit GLOBAL
 * index) is a pure function of (seed, p, n_cand, n_punct, key_bits), like the frames independent of batch, launch shape and device:
 *
 *   candidates an ascending list of distinct VNs cand[0 .. n_cand-1]; default: every QLDPC_VN_PINNED VN of the class map, ascending (with the
 *              harness's classes the parity VNs, its `for a = K .. N-1`)
 *   key        u_c = output word c % 4 of the generator at counter (c / 4, 2, p_lo, p_hi), key = (seed low word, seed high word);
 *              u'_c = u_c >> (32 - key_bits)
 *   selection  the n_punct candidates smallest in the lexicographic order (u'_c, c), 0 <= n_punct <= n_cand: equal keys go to the lower
 *              candidate index.  A uniformly random subset, up to 32-bit key collisions broken by index.
 *
 * key_bits is 32 in production and 0 stands for 32; smaller values exist so that TESTS can force equal keys and reach the tie rule (as
 * tile_words of qldpc_toeplitz_host and lanes of qldpc_crc32_words_chunked).  A pattern is an erase row of ceil(N / 32) words, MSB-first; an
 * erasure overrides whatever the frame holds at that VN (qldpc_load_erasures_dev).
 *
 * qldpc_mc_search: frame k of pattern p is Monte-Carlo frame first_frame + p F + k (F = frames_per_pattern), so the counter row of a pattern is
 * a pure function of (seed, p, F, first_frame, n_punct, key_bits, qber, candidates, decoder configuration) and depends neither on the batch
 * nor on first_pattern nor on how a search is split into calls.  A round is floor(batch / F) patterns in one generate / load / erase / run /
 * fetch / monitor sequence with one read-back of its counter rows; the last round may be ragged.  With stop_at_goal the search stops after the
 * first round that holds a pattern without frame errors; `patterns` is therefore round-granular (as `frames` of qldpc_mc_run), goal, best and
 * the rows are not.  Status codes: QLDPC_ESIZE for n_punct outside [0, n_cand], frames_per_pattern outside [1, batch], key_bits outside
 * 0 .. 32, qber outside (0, 0.5); QLDPC_EINVAL for a candidate or puncture list that is not ascending, distinct and inside [0, N) and for
 * non-zero reserved fields.  A refused call queues nothing.  What the pattern calls need on the device is allocated by the first
 * qldpc_mc_search / qldpc_mc_patterns_dev / qldpc_mc_set_puncture (and counted by qldpc_mc_device_bytes); later calls allocate nothing.
 * Not built: patterns per frame rather than per pattern slot, common frames across patterns, shortening patterns, feeding a found pattern
 * into qldpc_recon_*.
 */
typedef struct qldpc_mc qldpc_mc;
typedef struct qldpc_mc_cfg {
    uint64_t seed;
    int batch;             /* frames per decoder launch, <= the decoder's max_frames; 0 = the decoder's max_frames                  */
    int fail_cap;          /* the global indices of the first fail_cap failed frames of a run are kept (>= 1; default 1024)         */
    double parity_ber;     /* flip probability of a pinned VN, in [0, 1)                                                             */
    int reserved[2];       /* must be zero                                                                                           */
} qldpc_mc_cfg;
typedef struct qldpc_mc_result {
    uint64_t frames;        /* frames decoded: a multiple of the batch unless max_frames cut the last batch short                    */
    uint64_t bit_errors;    /* sum of be = popcount((decoded ^ codeword) & mask of info_bits_pos)                                    */
    uint64_t frame_errors;  /* frames with be > 0                                                                                    */
    uint64_t undetected;    /* ... whose hard decision nevertheless has a zero syndrome                                              */
    uint64_t not_converged; /* frames whose hard decision has a non-zero syndrome                                                    */
    uint64_t iter_sum, iter_max;
    uint64_t channel_flips, channel_bits;   /* flips drawn at QLDPC_VN_CHANNEL VNs / such VNs seen: the empirical QBER (with a table: the
                                               hard-decision error rate of those VNs)                                                */
    uint64_t batches;
    uint64_t next_frame;    /* first_frame + frames: where a following run continues                                                 */
    double decode_ms;       /* qldpc_run alone, by hipEvents: what SIM_THR of the harness means                                      */
    double source_ms, encode_ms, channel_ms, load_ms, monitor_ms;   /* the other stages of the batches, by hipEvents: info words, encoder,
                               channel, qldpc_load_bits_dev (with a table: qldpc_load_llr_dev), fetch + monitor                      */
    double total_ms;        /* the whole call on the host's clock                                                                    */
} qldpc_mc_result;

void   qldpc_mc_cfg_default(qldpc_mc_cfg *cfg);
/* host mirrors, no device needed: one generator call, and info words [n][ceil(K/32)] / flip words [n][ceil(N/32)] (either may be NULL)
   of frames [first_frame, first_frame + n_frames); info_bits_pos NULL = 0 .. K-1 */
int    qldpc_mc_philox_host(const uint32_t counter[4], const uint32_t key[2], uint32_t out[4]);
int    qldpc_mc_frames_host(int K, int N, const int *info_bits_pos, const uint8_t *vn_class, uint64_t seed, double qber, double parity_ber,
                            uint64_t first_frame, int n_frames, uint32_t *info_words, uint32_t *flip_words);
/* dec and enc (same code, same K; info_bits_pos are the encoder's) are not owned and must outlive the object */
int    qldpc_mc_create(qldpc_decoder *dec, qldpc_encoder *enc, const uint8_t *vn_class, const qldpc_mc_cfg *cfg, qldpc_mc **out);
void   qldpc_mc_free(qldpc_mc *mc);
size_t qldpc_mc_device_bytes(const qldpc_mc *mc);
/* the source alone, for callers with a loop of their own: device rows d_info[n][ceil(K/32)], d_cw[n][ceil(N/32)] (Alice's codeword) and
   d_rx[n][ceil(N/32)] (what Bob holds); d_rx, or d_cw and d_rx, may be NULL.  Asynchronous on the decoder's stream. */
int    qldpc_mc_frames_dev(qldpc_mc *mc, uint64_t first_frame, int n_frames, double qber, uint32_t *d_info, uint32_t *d_cw, uint32_t *d_rx);
/* Per batch: generate, encode, load, run, fetch, monitor, one read-back of the counters.  Stops at the first batch boundary at which
   frame_errors >= max_frame_errors (0 = never) or max_frames is reached; the last batch may be ragged.  Counters, histogram and failed-frame
   list start from zero in every call. */
int    qldpc_mc_run(qldpc_mc *mc, double qber, uint64_t first_frame, uint64_t max_frames, uint64_t max_frame_errors, qldpc_mc_result *result);
/* of the last run: frames per iteration count, n_ite + 1 bins; writes min(cap, n_ite + 1) and returns n_ite + 1 (or a status) */
int    qldpc_mc_iter_hist(qldpc_mc *mc, uint64_t *hist, int cap);
/* of the last run: the global indices of the failed frames kept (the first fail_cap in batch order, ascending); writes min(cap, kept) and
   returns kept (or a status) */
int    qldpc_mc_failed_frames(qldpc_mc *mc, uint64_t *frames, int cap);

/*
 * Quantised soft-output channels.  Besides the BSC the loop runs any binary-input channel with 2 <= Q <= 256 output levels given by a
 * threshold table (csrc/qldpc_mc_core.h): VN v of frame i draws u = output word v % 4 of the generator at counter (v / 4, 3, i_lo, i_hi) --
 * stream 3, so the BSC's frames do not move -- and, b being its codeword bit,
 *
 *   level = #{k : u >= cum[b][k]}        P(level | b) = (cum[b][level] - cum[b][level - 1]) / 2^32 exactly, cum[b][-1] = 0, cum[b][Q-1] = 2^32
 *
 * cum[b] (Q - 1 entries, uint64_t) is non-decreasing with entries in [0, 2^32]; repeated entries are levels of probability zero, entries equal
 * to 2^32 levels that nothing reaches.  Per class: QLDPC_VN_CHANNEL LLR = value[level]; QLDPC_VN_PINNED LLR = +-QLDPC_CONFIRMED_BIT_LLR by the
 * codeword bit, the sign inverted iff the same u < floor(parity_ber 2^32); QLDPC_VN_PUNCTURED LLR = 0.  The rx bit of a VN is its codeword bit,
 * inverted iff the sign of the LLR contradicts it (b = 0 and LLR < 0, or b = 1 and LLR > 0; 0 contradicts nothing), so channel_flips /
 * channel_bits becomes the hard-decision error rate of the channel VNs.  Frames stay a pure function of (seed, i) and the table; no floating
 * point is computed on the device.
 *
 * With a table set, qldpc_mc_run and qldpc_mc_search generate through the soft kernel and load the decoder with qldpc_load_llr_dev; their
 * qber argument is validated as before and otherwise IGNORED.  The fixed puncture set and the search's erase rows go on top as with the BSC.
 * qldpc_mc_frames_dev stays the BSC's frame call whatever is set.  qldpc_mc_set_channel returns QLDPC_ESIZE for levels outside 2 .. 256 (or a
 * batch whose quads pass 2^31 lanes) and QLDPC_EINVAL for a missing array, a decreasing row, an entry above 2^32 or non-zero reserved words; a
 * refused call leaves the previous table in force.  NULL, or levels = 0, returns the object to the BSC.  The first accepted table allocates
 * the LLR rows [batch][N] (counted by qldpc_mc_device_bytes).  Not built: unquantised float noise, a table per VN class, non-binary input.
 */
typedef struct qldpc_mc_channel {
    int levels;                /* Q, 2 .. 256; 0 = no table (the BSC)                                                                    */
    const uint64_t *cum[2];    /* cum[b][Q - 1], b = the codeword bit                                                                     */
    const float *value;        /* value[Q]: the LLR of a level                                                                            */
    int reserved[2];           /* must be zero                                                                                            */
} qldpc_mc_channel;
enum { QLDPC_MC_SOURCE_RANDOM = 0, QLDPC_MC_SOURCE_ZERO = 1 };
int    qldpc_mc_set_channel(qldpc_mc *mc, const qldpc_mc_channel *table);
/* QLDPC_MC_SOURCE_ZERO: all-zero info words, hence the all-zero codeword, in every call that generates frames (the published fixed-point
   AWGN table of the reference needs it, tests/matlab_fp.py); QLDPC_MC_SOURCE_RANDOM is the default */
int    qldpc_mc_set_source(qldpc_mc *mc, int mode);
/* host only: the table of BPSK over AWGN, r = (1 - 2 b) + sigma n quantised to floor(r / rmax * maxq) clamped to [-maxq - 1, maxq]: Q = 2 maxq
   + 2 levels (1 <= maxq <= 127), boundary k at (k - maxq) rmax / maxq, cum[b][k] = floor(2^32 Phi((boundary_k - (1 - 2 b)) / sigma)) with
   Phi(x) = erfc(-x / sqrt 2) / 2 in double, value[l] = l - maxq - 1.  cum0, cum1: Q - 1 entries; value: Q.  QLDPC_ESIZE for sigma or rmax not
   positive and finite or maxq outside 1 .. 127 */
int    qldpc_mc_awgn_table(double sigma, double rmax, int maxq, uint64_t *cum0, uint64_t *cum1, float *value);
/* host mirror, no device needed: LLR rows llr[n][N] and flip words [n][ceil(N/32)] (either may be NULL) of frames [first_frame, first_frame +
   n_frames) whose codewords are cw_words[n][ceil(N/32)] (NULL = the all-zero codeword); info_bits_pos and vn_class as qldpc_mc_frames_host */
int    qldpc_mc_llr_host(int K, int N, const int *info_bits_pos, const uint8_t *vn_class, uint64_t seed, double parity_ber,
                         const qldpc_mc_channel *table, const uint32_t *cw_words, uint64_t first_frame, int n_frames, float *llr,
                         uint32_t *flip_words);
/* the soft counterpart of qldpc_mc_frames_dev through the table that is set (QLDPC_ESTATE without one): d_info[n][ceil(K/32)],
   d_cw[n][ceil(N/32)], d_rx[n][ceil(N/32)] (may be NULL) and d_llr[n][N] float, frame-major as qldpc_load_llr_dev takes them.  QLDPC_ESIZE
   where n_frames * 8 ceil(N/32) passes 2^31.  Asynchronous on the decoder's stream. */
int    qldpc_mc_llr_dev(qldpc_mc *mc, uint64_t first_frame, int n_frames, uint32_t *d_info, uint32_t *d_cw, uint32_t *d_rx, float *d_llr);

/* host mirror, no device needed: the candidate indices (into the candidate list) of pattern `pattern`, ascending */
int    qldpc_mc_pattern_host(uint64_t seed, uint64_t pattern, int n_cand, int n_punct, int key_bits, int *idx /* n_punct */);
/* the candidate VNs of the object (a HOST array): ascending, distinct, inside [0, N); NULL = every QLDPC_VN_PINNED VN of the class map */
int    qldpc_mc_set_candidates(qldpc_mc *mc, const int *vn, int n);
/* erase rows of patterns [first_pattern, first_pattern + n_patterns): d_erase[n_patterns][ceil(N/32)], MSB-first; asynchronous on the
   decoder's stream */
int    qldpc_mc_patterns_dev(qldpc_mc *mc, uint64_t first_pattern, int n_patterns, int n_punct, int key_bits, uint32_t *d_erase);
/* the VNs of a pattern over the object's candidates, ascending (host side) */
int    qldpc_mc_pattern_vns(qldpc_mc *mc, uint64_t pattern, int n_punct, int key_bits, int *vn /* n_punct */);
/* a fixed puncture set for qldpc_mc_run (a HOST array, ascending, distinct): these VNs are erased in every frame, everything else of the run is
   unchanged, so its counters equal the search's row of that pattern over the same frames.  n = 0 clears it: the run then issues exactly the
   launches it issues without this call. */
int    qldpc_mc_set_puncture(qldpc_mc *mc, const int *vn, int n);

typedef struct qldpc_mc_search_cfg {
    int n_punct;              /* VNs erased per pattern, 0 .. n_cand                                                                  */
    int frames_per_pattern;   /* F, 1 .. batch                                                                                        */
    int key_bits;             /* 0 = 32; below 32 for tests only                                                                      */
    int stop_at_goal;         /* stop after the first round that holds a pattern without frame errors                                 */
    uint64_t first_frame;
    int reserved[2];          /* must be zero                                                                                         */
} qldpc_mc_search_cfg;
typedef struct qldpc_mc_pattern_stat { uint64_t pattern, frames, frame_errors, bit_errors, undetected, not_converged, iter_sum; } qldpc_mc_pattern_stat;
typedef struct qldpc_mc_search_result {
    uint64_t patterns, frames, batches;   /* evaluated: whole rounds                                                                  */
    uint64_t goal;            /* lowest pattern index with 0 frame errors in its F frames; UINT64_MAX = none                          */
    uint64_t best, best_frame_errors, best_bit_errors;   /* fewest frame errors, then fewest bit errors, then lowest index            */
    uint64_t next_pattern;    /* first_pattern + patterns                                                                             */
    double decode_ms;         /* qldpc_run alone, by hipEvents                                                                        */
    double pattern_ms, expand_ms, generate_ms, load_ms, erase_ms, monitor_ms;   /* the other stages of the rounds, by hipEvents: pattern
                                 kernel, rows -> frame rows, source + encoder + BSC, qldpc_load_bits_dev, qldpc_load_erasures_dev,
                                 fetch + per-pattern monitor                                                                          */
    double total_ms;          /* the whole call on the host's clock                                                                   */
} qldpc_mc_search_result;
/* patterns [first_pattern, first_pattern + max_patterns) in rounds, see above */
int    qldpc_mc_search(qldpc_mc *mc, double qber, const qldpc_mc_search_cfg *cfg, uint64_t first_pattern, uint64_t max_patterns,
                       qldpc_mc_search_result *res);
/* of the last search: one row per evaluated pattern, in pattern order; writes min(cap, count) and returns the count (or a status) */
int    qldpc_mc_search_stats(qldpc_mc *mc, qldpc_mc_pattern_stat *rows, int cap);

/*
 * The QBER sweep (the harness's outermost loop, `for (float ber = ber_min; ber <= ber_max; ber += ber_step)`, BS/src/main.cpp:233, with
 * parity_bits_to_punct(K, N, min_cr(ber, target_efficiency)) punctured parity bits per BER, :235,272): operating points side by side in one
 * batch, each with its own monitor row and stop rule, and lanes that pass from closed points to open ones.
 *
 *   point      a sweep has P operating points, 1 <= P <= QLDPC_MC_SWEEP_MAX_POINTS; point q = (qber_q in (0, 0.5), n_punct_q >= 0)
 *   puncture   the sets are nested: the caller gives ONE order punct_order[n_order], a HOST array of distinct VNs inside [0, N) that need
 *              not be ascending (the order is the point of it); point q erases the first n_punct_q VNs of it on top of the fixed set of
 *              qldpc_mc_set_puncture.  n_order = 0: no puncturing, every n_punct_q must be 0
 *   frames     frame k of EVERY point is Monte-Carlo frame first_frame + k: the same info word and the same Philox words, so the flip
 *              sets of two points are nested as their thresholds are.  The row of a point is exactly what the point would get alone: its
 *              counters equal those of qldpc_mc_run(qber_q, first_frame, max_frames = frames_q, max_frame_errors = 0) after
 *              qldpc_mc_set_puncture(fixed set + prefix_q), for any batch, any chunk and any set of neighbouring points
 *   rounds     a chunk is C frames, 1 <= C <= batch (cfg.chunk = 0: min(64, batch)); a round has S = floor(batch / C) chunk slots.
 *              Point q is OPEN iff done_q < max_frames and (max_frame_errors == 0 or fe_q < max_frame_errors);
 *              need_q = ceil((max_frames - done_q) / C) for an open point
 *   deal       cycles over the open points in ascending q and on each visit gives one chunk to a point with give_q < need_q; it stops when
 *              the S slots are used or a whole cycle has given nothing.  The chunks of a point are consecutive in the batch, points in
 *              ascending order, frame slots without holes; the j-th chunk of point q covers k in [done_q + j C, min(done_q + (j + 1) C,
 *              max_frames)), so only the last chunk of a point can be ragged.  The deal is a pure function of (done[], fe[], C, S,
 *              max_frames, max_frame_errors): nothing depends on timing (qldpc_mc_sweep_deal_host is that function)
 *
 * One round is one sequence generate / encode / channel / load / erase / qldpc_run / fetch / monitor that ends with ONE read-back of the P
 * counter rows; the host updates done and fe from those rows and deals the next round.  The sweep ends when no point is open.  frames_q is
 * therefore round-granular (as `frames` of qldpc_mc_run is batch-granular); the rows, given frames_q, are not.  A point that reaches
 * max_frames is closed by QLDPC_MC_CLOSED_MAX_FRAMES, whatever its frame errors; otherwise by QLDPC_MC_CLOSED_MAX_FE.  Rounds count from 0.
 *
 * Status codes: QLDPC_ESIZE for P outside its range, a qber outside (0, 0.5), chunk outside [0, batch], max_frames == 0, an n_punct outside
 * [0, n_order]; QLDPC_EINVAL for a missing array, an order with a repeated or out-of-range VN, non-zero reserved fields; QLDPC_ESTATE while a
 * table of qldpc_mc_set_channel is in force.  A refused call queues nothing and leaves the last sweep's rows readable.  The kernels run at
 * most batch ceil(N / 32) lanes, which qldpc_mc_create has checked against 2^31.  The first sweep allocates what sweeps need on the device
 * (the slot tables, the point rows {threshold, |LLR|}, the erase rows of QLDPC_MC_SWEEP_MAX_POINTS points, the frame erase rows if the search
 * has not made them, the counter and histogram rows and the pinned copies of slot tables and counter rows), counted by
 * qldpc_mc_device_bytes; later sweeps allocate nothing.  A sweep touches neither the counters, histogram and failed-frame list of the last
 * qldpc_mc_run nor the rows of the last search.  Its gain over one qldpc_mc_run per point is not measured yet (tools/mc_sweep_cost.py).
 * Points of a table channel (a table per point) are qldpc_mc_sweep_tables below.  Not built: failed-frame lists per point (a failed frame of a point is regenerated with
 * qldpc_mc_run over its index); a puncture pattern drawn per point (qldpc_mc_search does that at one QBER); one encode shared by the points
 * that sit on the same frame; a multi-GPU driver; the deal on the device.
 */
#define QLDPC_MC_SWEEP_MAX_POINTS 4096
enum { QLDPC_MC_CLOSED_MAX_FE = 1, QLDPC_MC_CLOSED_MAX_FRAMES = 2 };
typedef struct qldpc_mc_point { double qber; int n_punct; int reserved; /* must be zero */ } qldpc_mc_point;
typedef struct qldpc_mc_sweep_cfg {
    const qldpc_mc_point *points; int n_points;
    const int *punct_order; int n_order;
    int chunk;                 /* C; 0 = min(64, batch)                                                                                */
    uint64_t first_frame, max_frames, max_frame_errors;   /* per point; max_frame_errors = 0: no stop rule                            */
    int reserved[2];           /* must be zero                                                                                         */
} qldpc_mc_sweep_cfg;
typedef struct qldpc_mc_point_stat {
    double qber; int n_punct;
    int closed_by;             /* QLDPC_MC_CLOSED_*                                                                                    */
    uint64_t frames, frame_errors, bit_errors, undetected, not_converged, iter_sum, iter_max, channel_flips, channel_bits;   /* as qldpc_mc_result */
    uint64_t last_round;       /* the last round in which the point received frames                                                    */
} qldpc_mc_point_stat;
typedef struct qldpc_mc_sweep_result {
    uint64_t rounds, frames, batches;   /* frames = the sum over the points; one decoder launch per round                              */
    double decode_ms;          /* qldpc_run alone, by hipEvents                                                                        */
    double source_ms, encode_ms, channel_ms, load_ms, erase_ms, monitor_ms;   /* the other stages of the rounds, by hipEvents: slot tables +
                                  info words, encoder, BSC per point, qldpc_load_bits_dev, expansion + qldpc_load_erasures_dev, fetch +
                                  per-point monitor                                                                                    */
    double total_ms;           /* the whole call on the host's clock                                                                   */
} qldpc_mc_sweep_result;
int    qldpc_mc_sweep(qldpc_mc *mc, const qldpc_mc_sweep_cfg *cfg, qldpc_mc_sweep_result *res);
/* of the last sweep: one row per point, in point order; writes min(cap, P) and returns P (or a status) */
int    qldpc_mc_sweep_stats(qldpc_mc *mc, qldpc_mc_point_stat *rows, int cap);
/* of the last sweep: frames per iteration count of one point, n_ite + 1 bins; writes min(cap, n_ite + 1) and returns n_ite + 1 (or a
   status: QLDPC_ESIZE for a point the last sweep did not have, QLDPC_ESTATE after a later qldpc_mc_strata, whose rows then hold the device) */
int    qldpc_mc_sweep_hist(qldpc_mc *mc, int point, uint64_t *hist, int cap);
/* host mirror, no device needed: the deal of one round over n_points points with `slots` chunk slots of `chunk` frames; give[n_points] = the
   chunks of each point; returns the chunks dealt (or a status: QLDPC_ESIZE for n_points outside 1 .. QLDPC_MC_SWEEP_MAX_POINTS, chunk < 1,
   slots < 1 or max_frames == 0, QLDPC_EINVAL for a missing array) */
int    qldpc_mc_sweep_deal_host(int n_points, int chunk, int slots, uint64_t max_frames, uint64_t max_frame_errors, const uint64_t *done,
                                const uint64_t *frame_errors, int *give);

/*
 * The sweep over operating points of a TABLE channel (an Eb/N0 sweep: the four points per matrix of the reference's fixed-point AWGN experiment,
 * ML/sim_results.m, in one call).  Everything of qldpc_mc_sweep above holds -- the points side by side in one batch, frame k of every point = frame
 * first_frame + k, the nested puncture prefixes on top of the fixed set, chunks, the deal, one read-back per round -- with one change: point q draws
 * its frames through its OWN threshold table table_q ("Quantised soft-output channels" above; the tables of one sweep may differ in levels and
 * in everything else) and the decoder is loaded with qldpc_load_llr_dev.  The row of point q is exactly what
 * qldpc_mc_set_channel(table_q) + qldpc_mc_set_puncture(fixed set + prefix_q) + qldpc_mc_run(., first_frame, frames_q, 0) give for that point
 * alone, for any batch, any chunk and any set of neighbouring points.  `label` is the caller's name for the point -- Eb/N0 in dB, say --; it is
 * not interpreted and comes back in the `qber` field of the point's qldpc_mc_point_stat.  Rows and histograms are read with
 * qldpc_mc_sweep_stats / qldpc_mc_sweep_hist: the call is a sweep to them and to qldpc_mc_strata_hist (QLDPC_ESTATE after it).
 *
 * The call neither needs nor changes the table of qldpc_mc_set_channel: with one in force or without, qldpc_mc_run afterwards runs as before
 * (and qldpc_mc_sweep keeps returning QLDPC_ESTATE while one is in force).  Status codes: per table those of qldpc_mc_set_channel (QLDPC_ESIZE for
 * levels outside 2 .. 256, QLDPC_EINVAL for a missing array, a decreasing row, an entry above 2^32, non-zero reserved words), for the rest those
 * of qldpc_mc_sweep, and QLDPC_ESIZE for a batch whose quads pass 2^31 lanes.  A refused call queues nothing and leaves the last rows readable.
 * qldpc_mc_sweep_tables_check_host is every one of these checks without a device; the device call runs it first.  On the device the call adds the P
 * tables (3 076 bytes each, allocated for the call's P and grown when a later call has more) and, where qldpc_mc_set_channel has not made
 * them, the LLR rows [batch][N]; both are counted by qldpc_mc_device_bytes.  Against one qldpc_mc_set_channel + qldpc_mc_run per point it is measured on one
 * configuration only (tools/mc_sweep_cost.py --tables: four points of 20 000 frames on a batch of 20 000, no stop rule: 12.5 ms against 12.3 ms, no gain).  Not built: strata or blind rounds of a table channel, a table per VN class, a frame budget per
 * point.
 */
typedef struct qldpc_mc_table_point {
    qldpc_mc_channel table;    /* levels 2 .. 256 (0 is no point), cum[2], value; HOST arrays, read during the call only                  */
    double label;              /* the caller's; returned in qldpc_mc_point_stat.qber                                                      */
    int n_punct;               /* the first n_punct VNs of punct_order are erased in this point's frames                                  */
    int reserved;              /* must be zero                                                                                            */
} qldpc_mc_table_point;
typedef struct qldpc_mc_sweep_tables_cfg {   /* as qldpc_mc_sweep_cfg, points of tables */
    const qldpc_mc_table_point *points; int n_points;
    const int *punct_order; int n_order;
    int chunk;
    uint64_t first_frame, max_frames, max_frame_errors;
    int reserved[2];
} qldpc_mc_sweep_tables_cfg;
int    qldpc_mc_sweep_tables(qldpc_mc *mc, const qldpc_mc_sweep_tables_cfg *cfg, qldpc_mc_sweep_result *res);
/* every argument check of qldpc_mc_sweep_tables for an object of a code of N VNs and this batch, no device: QLDPC_OK or the status the call returns */
int    qldpc_mc_sweep_tables_check_host(int N, int batch, const qldpc_mc_sweep_tables_cfg *cfg);

/*
 * Fixed-weight error strata: the step that makes a deep FER affordable on the BSC, and there it is exact.  Conditioned on the number W of
 * flipped channel bits the flip set is uniform over the C(n, W) subsets, and with the decoder's |LLR| held fixed the failure probability
 * P_f(w) of weight w does not depend on the QBER, so FER(q) = sum_w Binom(n, q)(w) P_f(w) for every q from ONE set of fixed-weight runs: the
 * binomial tail is known in closed form and only the narrow transition of P_f(w) is simulated.  It also answers how many errors a block may
 * hold and still decode.
 *
 *   frame      the fixed-weight frame (i, w) (csrc/qldpc_mc_core.h): the key of VN v is u_v, output word v % 4 of the generator at counter
 *              (v / 4, 1, i_lo, i_hi) -- exactly the word the BSC frame compares with its threshold -- coarsened to u'_v = u_v >>
 *              (32 - key_bits), key_bits 1 .. 32 (0 stands for 32; smaller values exist so that tests can force ties).  The flip set is the
 *              w VNs of class QLDPC_VN_CHANNEL smallest in the order (u'_v, v): equal keys go to the lower VN; 0 <= w <= channel VNs.
 *              QLDPC_VN_PINNED VNs keep their rule (flip iff u_v < floor(parity_ber 2^32)), QLDPC_VN_PUNCTURED VNs never flip.  The weight
 *              counts channel VNs before any erasure of qldpc_mc_set_puncture: an erased VN may be in the set and then has no effect
 *   identity   at key_bits = 32 the BSC set {v channel : u_v < T} is, for every T, the fixed-weight set of its own size: the frame of
 *              qldpc_mc_frames_host with c channel flips IS the fixed-weight frame of weight c, bit for bit, and the flip sets of two
 *              weights of one frame are nested
 *   strata     qldpc_mc_strata runs 1 <= n_strata <= QLDPC_MC_SWEEP_MAX_POINTS weights (any order, repeats allowed) side by side in one
 *              batch; every slot is decoded with |LLR| = qldpc_bsc_llr((float)design_qber), design_qber in (0, 0.5); frame k of every
 *              stratum is Monte-Carlo frame first_frame + k.  Open / closed, need, chunks, the deal (qldpc_mc_sweep_deal_host), the rounds
 *              and the one read-back per round are those of qldpc_mc_sweep, and the two calls run the same round loop; the fixed set of
 *              qldpc_mc_set_puncture is honoured.  The row of a stratum is what the stratum would get alone, for any batch, chunk and
 *              neighbours; channel_flips is counted by the monitor kernel from rx ^ cw and so comes out as frames x weight
 *   estimate   qldpc_mc_strata_fer_host, from strictly ascending weights w_0 < .. < w_last: p_s = frame_errors_s / frames_s; P^(w) is
 *              piecewise linear in w between neighbouring strata; b(w) = exp(lgamma(n + 1) - lgamma(w + 1) - lgamma(n - w + 1) + w ln q +
 *              (n - w) log1p(-q)) in double.  out[0] = sum_{w_0 <= w <= w_last} b(w) P^(w); out[1] = sum_{w < w_0} b(w); out[2] =
 *              sum_{w > w_last} b(w); out[3] = sqrt(sum_s c_s^2 p_s (1 - p_s) / frames_s), c_s = sum_w b(w) hat_s(w) the binomial mass that
 *              stratum s carries through the interpolation, so that out[0] = sum_s c_s p_s
 *
 * The caller turns out[1] and out[2] into bounds: as far as the interpolation holds, FER(q) lies between out[0] and out[0] + out[1] +
 * out[2]; where the top stratum fails every frame, out[2] counts in full.  Limits: P_f below the lowest stratum that saw a failure is
 * bounded only by the frames spent there (0 of F frames bounds p_s by about 3 / F at 95 %): stratification removes the binomial tail, NOT an
 * error floor.  The linear interpolation is an assumption between strata (contiguous weights need none), out[3] is the sampling error of the
 * p_s alone, and P_f(w) is that of the decoder at the design |LLR|: a decoder fed the |LLR| of each q differs where its rule is not
 * scale-invariant.
 *
 * Status codes: QLDPC_ESIZE for a weight outside [0, channel VNs], n_strata outside its range, design_qber outside (0, 0.5), chunk outside
 * [0, batch], max_frames == 0, key_bits outside 0 .. 32, and in the estimate frames_s == 0 (or frame_errors_s > frames_s) or qber outside
 * (0, 1); QLDPC_EINVAL for a missing array, non-zero reserved fields, or weights not strictly ascending in the estimate; QLDPC_ESTATE while a
 * table of qldpc_mc_set_channel is in force; QLDPC_ENODEV without a device.  A refused call queues nothing and leaves earlier rows readable.
 * The first strata call allocates what it needs (what the first sweep allocates: the two calls share the slot tables and the device rows),
 * counted by qldpc_mc_device_bytes; later calls allocate nothing.  The device rows belong to whichever of qldpc_mc_sweep / qldpc_mc_strata ran
 * last: qldpc_mc_sweep_hist after a strata run and qldpc_mc_strata_hist after a sweep return QLDPC_ESTATE; the stat rows of both are kept on
 * the host, separately, and stay readable.  The fixed-weight channel costs about five times the generator work of the BSC kernel (four digit
 * passes and the final one); measured once at the headline shape it took 0.8 ms per 4 096-frame round beside 81 ms of decode
 * (tools/mc_strata_cost.py, profiles/mc_strata_cost.json).
 * Not built: a matched |LLR| per stratum; strata of a table channel; failed-frame lists per stratum; an adaptive choice of weights; a
 * multi-GPU driver; the deal on the device.
 */
typedef struct qldpc_mc_strata_cfg {
    const int *weights; int n_strata;   /* HOST array                                                                                 */
    double design_qber;        /* every slot is decoded with |LLR| = qldpc_bsc_llr((float)design_qber)                                 */
    int key_bits;              /* 0 = 32                                                                                               */
    int chunk;                 /* C; 0 = min(64, batch)                                                                                */
    uint64_t first_frame, max_frames, max_frame_errors;   /* per stratum; max_frame_errors = 0: no stop rule                          */
    int reserved[2];           /* must be zero                                                                                         */
} qldpc_mc_strata_cfg;
typedef qldpc_mc_sweep_result qldpc_mc_strata_result;     /* rounds, frames, batches, stage times; channel_ms = the fixed-weight channel */
typedef struct qldpc_mc_stratum_stat {
    int weight;
    int closed_by;             /* QLDPC_MC_CLOSED_*                                                                                    */
    uint64_t frames, frame_errors, bit_errors, undetected, not_converged, iter_sum, iter_max, channel_flips, channel_bits;   /* as qldpc_mc_result */
    uint64_t last_round;       /* the last round in which the stratum received frames                                                  */
} qldpc_mc_stratum_stat;
/* host mirror, no device needed: frames [first_frame, first_frame + n_frames), frame f at weight weights[f]: info_words[n][ceil(K/32)] and
   flip_words[n][ceil(N/32)] as qldpc_mc_frames_host gives them (either may be NULL; weights is read for flip_words only); info_bits_pos and
   vn_class as there */
int    qldpc_mc_weight_frames_host(int K, int N, const int *info_bits_pos, const uint8_t *vn_class, uint64_t seed, double parity_ber,
                                   uint64_t first_frame, int n_frames, const int *weights /* n_frames */, int key_bits, uint32_t *info_words,
                                   uint32_t *flip_words);
/* the source alone, one weight for the call: DEVICE buffers d_info[n][ceil(K/32)], d_cw[n][ceil(N/32)], d_rx[n][ceil(N/32)] = cw ^ flips
   (d_cw / d_rx may be NULL from the right); asynchronous on the decoder's stream, like qldpc_mc_frames_dev */
int    qldpc_mc_weight_frames_dev(qldpc_mc *mc, uint64_t first_frame, int n_frames, int weight, int key_bits, uint32_t *d_info, uint32_t *d_cw,
                                  uint32_t *d_rx);
int    qldpc_mc_strata(qldpc_mc *mc, const qldpc_mc_strata_cfg *cfg, qldpc_mc_strata_result *res);
/* of the last strata run: one row per stratum, in the caller's order; writes min(cap, n_strata) and returns n_strata (or a status) */
int    qldpc_mc_strata_stats(qldpc_mc *mc, qldpc_mc_stratum_stat *rows, int cap);
/* of the last strata run: frames per iteration count of one stratum, n_ite + 1 bins; writes min(cap, n_ite + 1) and returns n_ite + 1 (or a
   status: QLDPC_ESIZE for a stratum the last run did not have, QLDPC_ESTATE after a later qldpc_mc_sweep) */
int    qldpc_mc_strata_hist(qldpc_mc *mc, int stratum, uint64_t *hist, int cap);
/* host only: the estimate above over n_channel channel VNs at `qber`; weights strictly ascending */
int    qldpc_mc_strata_fer_host(int n_channel, int n_strata, const int *weights, const uint64_t *frames, const uint64_t *frame_errors, double qber,
                                double out[4]);

/*
 * Blind reconciliation rounds inside the Monte-Carlo loop: what asking for the weakest key bits after a failed decode buys at a code, a rule,
 * a QBER and a puncture set -- the FER that remains, the key bits disclosed and the decodes it costs.  The BSC at `qber`, the loop's classes
 * and the fixed set of qldpc_mc_set_puncture; per frame i:
 *
 *   round 0    the decode qldpc_mc_run does
 *   closing    a frame CLOSES in the first round whose decode ends with a zero syndrome (`ok` of qldpc_fetch_status_dev; Bob sees nothing
 *              else): a frame that closes wrong counts as frame_errors and undetected
 *   asking     a frame still open after round r < R = max_rounds asks for its min(ask_bits, candidates) weakest positions (the select of
 *              qldpc_fetch_weakest_dev: ascending (bits of |posterior|, VN) over the posteriors of that very decode) among the
 *              QLDPC_VN_CHANNEL VNs it does not know yet; known <- known | asked, the values are Alice's codeword bits
 *   round r+1  the same frame -- the same channel word, the same |LLR| -- loaded again with the known bits pinned (qldpc_load_known_dev,
 *              +-QLDPC_CONFIRMED_BIT_LLR) and decoded from scratch
 *   open       a frame still open after round R stays open
 *
 * Everything about a frame -- its round of closure, its ask sets, its verdict -- is a pure function of (seed, i, qber, ask_bits, max_rounds,
 * decoder configuration, class map, puncture set): nothing depends on the batch, on the frames that share a launch with it or on how a run is
 * split into calls.
 *
 *   pools      only the frames still open are decoded again.  Level r = 1 .. R has a pool of {frame index, known row} entries, used as a
 *              stack of capacity 2 batch - 1; a launch decodes n <= batch frames of ONE level: fresh frames (level 0) or the last n entries of
 *              pool r, whose channel words are generated again from their indices.  Its open frames are appended to pool r + 1 in ascending
 *              slot order (a scan over the open flags: the content of a pool is reproducible)
 *   schedule   qldpc_mc_blind_next_host, a pure function of the pool counts: the DEEPEST level with pool >= batch, `batch` of it; else, while
 *              input is left, level 0 with min(batch, input_left); else the LOWEST non-empty level, all of it (the flush).  Deepest-first keeps
 *              every pool below 2 batch (csrc/qldpc_mc_core.h has the argument)
 *   input      ends at max_frames, and at the first launch boundary at which the frame errors tallied so far reach max_frame_errors (0 =
 *              never).  The pools are then FLUSHED, never dropped: the frames in flight are the hard ones, and abandoning them would bias
 *              every figure.  `frames` of the result is therefore exactly the frames drawn
 *   rows       row r <= R: the frames that closed in round r; row R + 1: the frames still open after round R.  The counters are those of
 *              qldpc_mc_result over the frame's LAST decode; disclosed = the key bits those frames asked for, in total
 *
 * One launch is generate / encode / channel / load (+ the fixed set, + the known bits) / qldpc_run / fetch + select / advance and ends with ONE
 * read-back of the R + 2 counter rows and the pool counts.  Status codes: QLDPC_ESIZE for qber outside (0, 0.5), ask_bits < 1, max_rounds outside
 * 0 .. QLDPC_MC_BLIND_MAX_ROUNDS; QLDPC_EINVAL for non-zero reserved words; QLDPC_EUNSUPPORTED while a table of qldpc_mc_set_channel is in
 * force (clear it with qldpc_mc_set_channel(mc, NULL)), for a decoder on the EDGES engine (create it with engine = FRAMES) and for a decoder
 * whose configuration can compact its active frames (flooding with compact = 0 and >= 4 groups does; create it with compact = 2), after which
 * qldpc_fetch_weakest_dev is refused.  A refused call queues nothing and leaves the rows of the last call readable.  The first call allocates
 * what the rounds need -- the pools, the candidate and ask rows, the list of open frames (fail_cap entries with their known rows), the counter
 * rows -- counted by qldpc_mc_device_bytes; later calls with the same or a smaller max_rounds allocate nothing.  A call touches neither the
 * counters of the last qldpc_mc_run nor the rows of a search, a sweep or a strata run.  Measured once at the headline shape at the foot of
 * the waterfall (tools/mc_blind_cost.py, profiles/mc_blind_cost.json: 124 of 16 384 first decodes fail): 1.0078 decodes per frame and 1.14 x the wall
 * time of qldpc_mc_run over the same frames, most of the difference in the select stage; deeper in the waterfall: not measured yet.
 * Not built: continuing BP from the failed run's messages; asking among punctured parity VNs; table channels; blind rounds inside sweep /
 * strata points; sessions or gangs as the decoder; the schedule on the device.
 */
#define QLDPC_MC_BLIND_MAX_ROUNDS 64
typedef struct qldpc_mc_blind_cfg {
    double qber;
    int ask_bits;              /* >= 1                                                                                                 */
    int max_rounds;            /* R, 0 .. QLDPC_MC_BLIND_MAX_ROUNDS; 0: qldpc_mc_run's decode with its frames split by the syndrome verdict */
    uint64_t first_frame, max_frames, max_frame_errors;   /* max_frame_errors = 0: no stop rule                                        */
    int reserved[2];           /* must be zero                                                                                         */
} qldpc_mc_blind_cfg;
typedef struct qldpc_mc_blind_round_stat {   /* row r <= R: the frames that closed in round r; row R + 1: still open after round R    */
    uint64_t frames, bit_errors, frame_errors, undetected, not_converged, iter_sum, iter_max, channel_flips, channel_bits;   /* of the frame's LAST decode */
    uint64_t disclosed;        /* key bits those frames asked for, in total                                                            */
} qldpc_mc_blind_round_stat;
typedef struct qldpc_mc_blind_result {
    uint64_t frames, frame_errors, undetected, open, disclosed;   /* sums over the rows; open = the frames of row R + 1                */
    uint64_t decodes;          /* frame-decodes run: the sum over the launches of n                                                    */
    uint64_t launches, next_frame;
    double source_ms, encode_ms, channel_ms, load_ms, decode_ms, select_ms, advance_ms;   /* the stages of the launches, by hipEvents: info
                                  words, encoder, BSC, load + fixed set + known bits, qldpc_run, fetch + candidate rows + select, verdicts +
                                  pool append                                                                                          */
    double total_ms;           /* the whole call on the host's clock                                                                   */
} qldpc_mc_blind_result;
int    qldpc_mc_blind(qldpc_mc *mc, const qldpc_mc_blind_cfg *cfg, qldpc_mc_blind_result *res);
/* of the last call: its max_rounds + 2 rows; writes min(cap, their number) and returns their number (or a status) */
int    qldpc_mc_blind_stats(qldpc_mc *mc, qldpc_mc_blind_round_stat *rows, int cap);
/* of the last call: the frames that ended open (the first fail_cap of them, ascending index) with everything they disclosed,
   known_words[cap][ceil(N/32)] packed MSB-first or NULL; writes min(cap, their number) and returns their number (or a status) */
int    qldpc_mc_blind_open(qldpc_mc *mc, uint64_t *frames, uint32_t *known_words, int cap);
/* host mirror, no device needed: the next launch by the schedule above from pool[max_rounds + 1] (pool[0] is not read) and the input that is
   left; returns 0 when nothing is left, 1 with *level and *n written (or a status: QLDPC_ESIZE for max_rounds outside its range or batch < 1,
   QLDPC_EINVAL for a missing pointer) */
int    qldpc_mc_blind_next_host(int max_rounds, int batch, const uint64_t *pool, uint64_t input_left, int *level, int *n);
/* host only: the efficiency a stream ends at, f = (n_disclosed_parity + disclosed / frames) / (n_channel h2(qber)) in double; QLDPC_ESIZE
   for n_channel < 1, n_disclosed_parity < 0, frames == 0 or qber outside (0, 0.5) */
int    qldpc_mc_blind_efficiency_host(int n_channel, int n_disclosed_parity, uint64_t frames, uint64_t disclosed, double qber, double *f);

/*
 * Guessing rounds: a third remedy for a failed decode, and the only one that discloses nothing.  Bob pins the g least reliable VNs of the failed
 * frame to each of the T = 2^g possible values himself, decodes the T trial frames side by side and keeps a trial whose syndrome comes out zero
 * ("BP with bit guessing", a Chase-style list step).  The rule is stated once in csrc/qldpc_guess_core.h, which the kernels and the host mirrors share:
 *
 *   guess set  the row qldpc_fetch_weakest_dev(cand, take, d = g) gives for the frame, a packed set of at most g VNs, ceil(N/32) words MSB-first;
 *              `hard` is the frame's packed hard-decision row (qldpc_fetch_packed_dev) of the same run
 *   trial t    0 <= t < T pins the VN of rank j to hard[v] ^ ((t >> j) & 1); the rank counts the set bits of the guess row in ascending VN order, so
 *              only the set matters; ranks >= popcount(row) do not exist and the bits of t above them are ignored; trial 0 pins the frame's own decisions
 *   winner     the lowest t whose decode ends with ok = 1, or -1; n_ok = the number of such trials; the frame is `ambiguous` when some ok trial's
 *              hard row differs from the winner's in any of the N valid bits: the only sign of a risky rescue that Bob can see
 *
 * qldpc_guess_expand_dev: d_weak, d_hard [n_src][ceil(N/32)] -> the known and value rows of the n_src T trial slots, slot s T + t, as
 *   qldpc_load_known_dev reads them: known row = the guess row, value row = the pinned values on the set bits and 0 elsewhere.
 * qldpc_guess_pick_dev: d_ok [n_src T] and d_trial_hard [n_src T][ceil(N/32)] of the trials' decode (qldpc_fetch_status_dev, qldpc_fetch_packed_dev)
 *   -> d_winner, d_n_ok, d_ambiguous [n_src] and the winner's row in d_out_hard [n_src][ceil(N/32)]; the row of a source without a winner is not
 *   touched.  d_out_hard must not overlap d_trial_hard.
 * Both take no decoder: device pointers of the current device and a stream (NULL = the default stream), and return once the kernel is queued.
 * QLDPC_EINVAL for a missing pointer; QLDPC_ESIZE for g outside 0 .. QLDPC_GUESS_MAX_BITS, N < 1, n_src < 0 or n_src T above 2^24.  With g = 0
 * there is one trial per source and it pins nothing; n_src = 0 queues nothing.  The host mirrors need no device and work on ONE trial and ONE source:
 * known_out, value_out [ceil(N/32)]; ok [T], trial_hard [T][ceil(N/32)] (and QLDPC_ESIZE for a trial outside 0 .. T - 1).
 */
#define QLDPC_GUESS_MAX_BITS 10
int    qldpc_guess_expand_dev(int N, int g, int n_src, const uint32_t *d_weak, const uint32_t *d_hard, uint32_t *d_known_out, uint32_t *d_value_out,
                              void *hip_stream);
int    qldpc_guess_pick_dev(int N, int g, int n_src, const int *d_ok, const uint32_t *d_trial_hard, int *d_winner, int *d_n_ok, int *d_ambiguous,
                            uint32_t *d_out_hard, void *hip_stream);
int    qldpc_guess_trial_host(int N, int g, int t, const uint32_t *weak, const uint32_t *hard, uint32_t *known_out, uint32_t *value_out);
int    qldpc_guess_pick_host(int N, int g, const int *ok, const uint32_t *trial_hard, int *winner, int *n_ok, int *ambiguous);

/*
 * Guessing rounds inside the Monte-Carlo loop: what they buy at a code, a rule, a QBER and a puncture set -- the FER that remains and the decodes it
 * costs -- at no leak.  The BSC at `qber`, the loop's classes and the fixed set of qldpc_mc_set_puncture; per frame i:
 *
 *   round 0    the decode qldpc_mc_run does; a frame with ok = 1 closes in row 0
 *   guess set  a failed frame takes its min(g, channel VNs) weakest positions among the QLDPC_VN_CHANNEL VNs (the select of qldpc_fetch_weakest_dev
 *              over the posteriors of that decode)
 *   trials     its T = 2^g trials are the same channel word, generated again from the index, each loaded with the trial's known and value rows
 *              (qldpc_guess_expand_dev, qldpc_load_known_dev) and decoded from scratch
 *   rescued    (row 1) iff a trial ends with a zero syndrome: the counters of row 1 are those of qldpc_mc_result over the WINNER's decode against
 *              Alice's codeword, so a winner that is wrong counts as frame_errors and undetected
 *   open       (row 2) otherwise, the counters over its FIRST decode
 *
 * Everything about a frame is a pure function of (seed, i, qber, g, decoder configuration, classes, puncture set): nothing depends on the batch, on
 * the neighbours in a launch or on how a run is split into calls.
 *
 *   pool       ONE pool of {frame index, guess row, hard row, the verdict of the first decode} entries; the failed frames of a fresh launch are
 *              appended in ascending slot order (the scan of the blind rounds).  A trial launch takes the LAST S = floor(batch / T) entries and
 *              runs S T trial frames
 *   schedule   qldpc_mc_guess_next_host, a pure function of the counts: a trial launch of S sources while pool >= S; else a fresh launch of
 *              min(batch, input_left) frames; else the flush, all remaining sources.  The pool stays below S + batch (csrc/qldpc_mc_core.h has
 *              the argument)
 *   input      ends at max_frames, and at the first launch boundary at which the errors tallied so far reach max_frame_errors (0 = never): the
 *              frame_errors of rows 0 and 1 (closed or rescued wrong) plus the frames of row 2 (open).  Failed first decodes that are still pooled
 *              do not count until they are resolved.  The pool is FLUSHED, never dropped
 *   rows       three qldpc_mc_blind_round_stat rows with disclosed = 0 (nothing is disclosed): closed at once, rescued, open
 *
 * Every launch ends with ONE read-back: the three counter rows, the pool and open counts and the sums.  guess_bits = 0 is qldpc_mc_run split by the
 * syndrome verdict: no trial launch, row 1 empty.  Status codes: QLDPC_ESIZE for guess_bits outside 0 .. QLDPC_GUESS_MAX_BITS, T above the batch,
 * guess_bits above the number of channel VNs, qber outside (0, 0.5); QLDPC_EINVAL for non-zero reserved words; QLDPC_EUNSUPPORTED, as
 * qldpc_mc_blind, while a table of qldpc_mc_set_channel is in force (clear it with qldpc_mc_set_channel(mc, NULL)), for a decoder on the EDGES
 * engine (create it with engine = FRAMES), for a decoder that may compact its active frames (create it with compact = 2) and for giveup_patience
 * without freeze_messages = 1.  A refused call queues nothing and leaves the rows of the last call readable.  The first call allocates the pool, the
 * trial rows and the list of open frames (fail_cap entries with their guess rows), sized for every g and counted by qldpc_mc_device_bytes; later
 * calls allocate nothing.  A call touches neither the counters of the last qldpc_mc_run nor the rows of a search, a sweep, a strata run or a blind
 * call (the launch scratch of the blind rounds -- candidate rows, selected rows, flags -- is shared, the result rows are not).
 * Measured once at the headline shape at the foot of the waterfall (tools/mc_guess_cost.py, profiles/mc_guess_cost.json: 124 of 16 384 first decodes
 * fail): g = 4 rescues 34 of them for 1.23 x the wall time of qldpc_mc_run over the same frames, g = 8 rescues 60 for 3.30 x (2.94 decodes per frame: the
 * trials are hopeless ones that run to n_ite); no rescue wrong, none ambiguous; deeper in the waterfall: not measured.
 * The sessions have them as qldpc_recon_decode_guess (above), with the CRC in the verdict.  Not built: the daemon binding; guesses among punctured parity VNs; pattern subsets (weight <= w); a
 * minimum-distance winner rule; guessing after or inside blind rounds; sweep / strata points; the schedule on the device.
 */
typedef struct qldpc_mc_guess_cfg {
    double qber;
    int guess_bits;            /* g, 0 .. QLDPC_GUESS_MAX_BITS, 2^g <= batch                                                            */
    uint64_t first_frame, max_frames, max_frame_errors;   /* max_frame_errors = 0: no stop rule                                        */
    int reserved[2];           /* must be zero                                                                                         */
} qldpc_mc_guess_cfg;
typedef struct qldpc_mc_guess_result {
    uint64_t frames, frame_errors, undetected;   /* sums over the rows                                                                 */
    uint64_t rescued, open;    /* the frames of rows 1 and 2                                                                           */
    uint64_t trials;           /* frame-decodes in trial launches                                                                      */
    uint64_t trial_iter_sum;   /* their iterations, each clamped to n_ite                                                              */
    uint64_t n_ok_sum;         /* trials that ended with a zero syndrome, over all sources                                             */
    uint64_t ambiguous;        /* rescued frames with two ok trials that differ                                                        */
    uint64_t decodes;          /* frame-decodes run: fresh frames + trials                                                             */
    uint64_t launches, next_frame;
    double source_ms, encode_ms, channel_ms, load_ms, decode_ms, select_ms, advance_ms;   /* as qldpc_mc_blind_result; of a trial launch the
                                  load includes the known bits and `advance` is the resolve + the append to the open list             */
    double expand_ms, pick_ms; /* trial launches: slot table + qldpc_guess_expand_dev; fetch + qldpc_guess_pick_dev                   */
    double total_ms;           /* the whole call on the host's clock                                                                   */
} qldpc_mc_guess_result;
int    qldpc_mc_guess(qldpc_mc *mc, const qldpc_mc_guess_cfg *cfg, qldpc_mc_guess_result *res);
/* of the last call: its 3 rows (disclosed = 0); writes min(cap, 3) and returns 3, or 0 before the first call (or a status) */
int    qldpc_mc_guess_stats(qldpc_mc *mc, qldpc_mc_blind_round_stat *rows, int cap);
/* of the last call: the frames that ended open (the first fail_cap of them, ascending index) with their guess rows, weak_words[cap][ceil(N/32)]
   packed MSB-first or NULL; writes min(cap, their number) and returns their number (or a status) */
int    qldpc_mc_guess_open(qldpc_mc *mc, uint64_t *frames, uint32_t *weak_words, int cap);
/* host mirror, no device needed: the next launch by the schedule above; returns 0 when nothing is left, 1 with *kind = QLDPC_MC_GUESS_FRESH and
   *n frames or QLDPC_MC_GUESS_TRIALS and *n SOURCES (n 2^g trial frames) (or a status: QLDPC_ESIZE for guess_bits outside its range, batch < 1 or
   2^guess_bits above the batch, QLDPC_EINVAL for a missing pointer) */
#define QLDPC_MC_GUESS_FRESH 1
#define QLDPC_MC_GUESS_TRIALS 2
int    qldpc_mc_guess_next_host(int guess_bits, int batch, uint64_t pool, uint64_t input_left, int *kind, int *n);

/* ------------------------------------------------------------------------------------------------------------------------------------------
 * Polar codes: a batched encoder and successive-cancellation (SC) decoder (qldpc_polar_*).  The definition is csrc/qldpc_polar_core.h, shared by
 * the kernels (csrc/qldpc_kernels_polar.h) and the host mirrors (csrc/qldpc_polar_host.c), which agree bit for bit in both message types.
 *
 *   size      N = 2^log2_n, 1 <= log2_n <= 20 (QLDPC_ESIZE).  Index i is natural order, no bit reversal.  Rows are packed MSB-first,
 *             ceil(N / 32) words; bits past N are ignored on input and zero on output.
 *   code      info_pos[n_info]: the positions that carry information, distinct (QLDPC_EINVAL) and below N (QLDPC_ESIZE), 0 <= n_info <= N
 *             (QLDPC_ESIZE); every other position is frozen.  The library ships no reliability table; qldpc_polar_tally_* and
 *             qldpc_polar_construct_* below fit an information set to a channel.
 *   encode    for m = 1, 2, .., N/2: in every block of 2m bits the first half becomes first ^ second.  An involution.
 *   decode    at a node with beliefs [a, b]: the left child gets f(a, b) = sgn(a) sgn(b) min(|a|, |b|) (sgn(v) = -1 iff v < 0), the right child
 *             g(a, b, c) = sat(b + (1 - 2c) a) with c the RE-ENCODED decisions of the left child; the node returns [c_left ^ c_right, c_right].
 *             Leaf: frozen -> its frozen value (0 without one), else bit = (L < 0).
 *   messages  QLDPC_POLAR_I8: int8 levels, clamped into [-(maxq + 1), maxq] on load; sat clamps to the same range and f is NOT saturated
 *             (f(-32, -32) = +32 at maxq = 31), so beliefs reach maxq + 1 and maxq is 1 .. 126 (QLDPC_ESIZE: 127 + 1 does not fit an int8).
 *             QLDPC_POLAR_F32: floats, sat is the identity, g one add or subtract; inputs must be finite (pin a bit with
 *             +-QLDPC_CONFIRMED_BIT_LLR, not with an infinity).  maxq is ignored.
 *   outputs   each may be NULL: u[n_frames][ceil(N/32)] all N decisions; info[n_frames][ceil(n_info/32)] bit m = u[info_pos[m]], the caller's
 *             order; x[n_frames][ceil(N/32)] the root's re-encoded word (= encode(u): Bob's corrected key when the frozen values are Alice's
 *             encode(key) on the frozen positions); leaf[n_frames][N] the leaf beliefs, int8 or float as the messages.
 *   inputs    llr[n_frames][N] frame-major, int8 or float by `messages`; frozen_u[n_frames][ceil(N/32)] the frozen values (bits at other
 *             positions are ignored), NULL = zeros.
 *
 * A context owns its scratch (qldpc_polar_device_bytes: about (2N - 64) x 64 beliefs and 16N bytes of rows per group of 64 frames); a call allocates
 * nothing, is asynchronous on the context's stream (qldpc_polar_set_stream, NULL = the null stream) and a context is not re-entrant.
 * QLDPC_ESIZE: n_frames > max_frames; QLDPC_EINVAL: n_frames < 0, a missing pointer, max_frames outside 1 .. 2^24, messages neither value.
 * n_frames = 0 is a no-op.  Every argument check runs before the first HIP call.  qldpc_polar_encode_dev may run in place (d_x = d_u).
 *
 * The decoder has two forms, the same function bit for bit in all four outputs; the library does not choose, `form` is the caller's.
 *   QLDPC_POLAR_LANES  a frame is one lane, a wave decodes 64 frames: for batches (N = 1 024 x 20 000 frames).  qldpc_polar_create means this.
 *   QLDPC_POLAR_WIDE   a workgroup per frame, lanes over the beliefs of a node, the levels up to 2^12 beliefs in LDS, a 32-leaf block on 32 lanes
 *                      (csrc/qldpc_kernels_polar_wide.h; the memory plan is csrc/qldpc_polar_wide_core.h, which qldpc_polar_decode_wide_host
 *                      walks one element at a time on the host, with the arguments and results of qldpc_polar_decode_host): for few long frames.
 *                      Such a context owns less than N beliefs and 8N / 32 bytes of rows per frame of max_frames, and every call above serves it
 *                      with the same contract.
 * qldpc_polar_create_form: a form that is neither is QLDPC_EINVAL; every other refusal is qldpc_polar_create's.
 *
 * The decoder has two RULES, and the library does not choose between them either (qldpc_polar_create_rule; csrc/qldpc_polar_ssc_core.h):
 *   QLDPC_POLAR_SC     the decoder above: every node of the tree is visited whatever the code is.  qldpc_polar_create and _create_form mean this.
 *   QLDPC_POLAR_SSC    the simplified SC decoder of Alamdar-Yazdi and Kschischang.  A node whose leaves are all frozen (rate 0) returns the
 *                      encoding of its frozen values and its beliefs are not looked at: exact.  A node with no frozen leaf (rate 1) returns
 *                      c[k] = (L[k] < 0) and decides u = encode(c).  Every other node takes the SC step.  Where no belief of a rate-1 node of a
 *                      frame is 0, this is SC bit for bit in u, info and x; where one is, SSC decides 0 for that bit and SC may not: a decoder
 *                      of its own, with a frame error rate inside SC's statistical band.  Outputs u, info and x; there is no leaf output (a
 *                      pruned node never forms its leaf beliefs).  Lanes form only.
 * qldpc_polar_create_rule: with QLDPC_POLAR_SC it is qldpc_polar_create_form; a rule that is neither is QLDPC_EINVAL; QLDPC_POLAR_SSC with
 * QLDPC_POLAR_WIDE and log2_n > 5 is QLDPC_EUNSUPPORTED (create a QLDPC_POLAR_LANES context).  An SSC context also owns the plan of its code on
 * the device (at most 12 bytes per 32 positions).  qldpc_polar_decode_dev serves it under the same contract, but a non-NULL d_leaf is
 * QLDPC_EUNSUPPORTED (create a QLDPC_POLAR_SC context for the leaf beliefs); _encode_dev, _set_stream, _device_bytes and _free are unchanged, and
 * qldpc_polar_tally_dev runs the tally it always ran: every position is frozen there, so the rule has no say.
 * qldpc_polar_decode_ssc_host: the mirror, qldpc_polar_decode_host's arguments and refusals without leaf.
 * qldpc_polar_ssc_plan_host: the plan the kernel and the mirror walk: steps[n_steps][3] = (first 32-leaf block, log2 of the leaves, kind: 0 rate
 * 0, 1 rate 1, 2 a mixed block decoded by the same rule inside it) in leaf order; the steps with kind < 2 are the maximal rate-0 and rate-1
 * nodes of 32 leaves or more; for N < 32 one mixed step holds the frame.  steps must hold max(N / 32, 1) x 3 ints.
 *
 * The ROWS form of the decode gives every frame a frozen set of its own (csrc/qldpc_kernels_polar_rows.h): what incremental freezing needs, where
 * a block that failed is decoded again with more positions frozen, and the blocks of one call sit at different rates.
 * qldpc_polar_decode_rows_dev: qldpc_polar_decode_dev with one more input, d_frozen_rows[n_frames][ceil(N/32)] packed MSB-first like every row,
 * required (QLDPC_EINVAL).  Position i of frame f is frozen iff the code's mask has it OR bit i of row f is set: a row only adds frozen
 * positions.  A frozen position takes its value from d_frozen_u, 0 where that is NULL.  d_info still reads u at the context's info_pos, so an
 * added position returns its frozen value there.  All-zero rows are qldpc_polar_decode_dev bit for bit.  Lanes form and SC rule only: a wide
 * context (log2_n > 5) and an SSC context are QLDPC_EUNSUPPORTED (the SSC plan belongs to the code, not to a frame).  Every other rule is
 * qldpc_polar_decode_dev's: outputs optional, the n_frames checks, asynchronous on the context's stream, all checks before the first HIP call.
 * The cost is one more word load and one OR per lane and 32 leaves; the flags never steer control flow, so a wave of 64 rates does not diverge.
 * qldpc_polar_decode_rows_host: the mirror, qldpc_polar_decode_host's arguments and refusals plus frozen_rows.
 */
typedef struct qldpc_polar qldpc_polar;
enum { QLDPC_POLAR_I8 = 0, QLDPC_POLAR_F32 = 1 };
enum { QLDPC_POLAR_LANES = 0, QLDPC_POLAR_WIDE = 1 };
enum { QLDPC_POLAR_SC = 0, QLDPC_POLAR_SSC = 1 };
int    qldpc_polar_create(int log2_n, int n_info, const int *info_pos, int messages, int maxq, int max_frames, int device, qldpc_polar **out);
int    qldpc_polar_create_form(int log2_n, int n_info, const int *info_pos, int messages, int maxq, int max_frames, int form, int device,
                               qldpc_polar **out);
int    qldpc_polar_create_rule(int log2_n, int n_info, const int *info_pos, int messages, int maxq, int max_frames, int form, int rule, int device,
                               qldpc_polar **out);
void   qldpc_polar_free(qldpc_polar *p);
size_t qldpc_polar_device_bytes(const qldpc_polar *p);
/* NULL = the null stream.  A switch to another stream orders it after everything the context has queued on the old one, so two calls of one context on
 * two streams still share its scratch one after the other; the same stream again does nothing (the stream switch, qldpc_decoder_set_stream).  The same
 * holds for qldpc_polar_list_set_stream */
int    qldpc_polar_set_stream(qldpc_polar *p, void *hip_stream);
int    qldpc_polar_encode_dev(qldpc_polar *p, int n_frames, const uint32_t *d_u, uint32_t *d_x);
int    qldpc_polar_decode_dev(qldpc_polar *p, int n_frames, const void *d_llr, const uint32_t *d_frozen_u,
                              uint32_t *d_u, uint32_t *d_info, uint32_t *d_x, void *d_leaf);
int    qldpc_polar_decode_rows_dev(qldpc_polar *p, int n_frames, const void *d_llr, const uint32_t *d_frozen_u, const uint32_t *d_frozen_rows,
                                   uint32_t *d_u, uint32_t *d_info, uint32_t *d_x, void *d_leaf);
/* host mirrors, no device needed */
int    qldpc_polar_encode_host(int log2_n, int n_frames, const uint32_t *u, uint32_t *x);
int    qldpc_polar_decode_host(int log2_n, int n_info, const int *info_pos, int messages, int maxq, int n_frames, const void *llr,
                               const uint32_t *frozen_u, uint32_t *u, uint32_t *info, uint32_t *x, void *leaf);
int    qldpc_polar_decode_rows_host(int log2_n, int n_info, const int *info_pos, int messages, int maxq, int n_frames, const void *llr,
                                    const uint32_t *frozen_u, const uint32_t *frozen_rows, uint32_t *u, uint32_t *info, uint32_t *x, void *leaf);
int    qldpc_polar_decode_wide_host(int log2_n, int n_info, const int *info_pos, int messages, int maxq, int n_frames, const void *llr,
                                    const uint32_t *frozen_u, uint32_t *u, uint32_t *info, uint32_t *x, void *leaf);
int    qldpc_polar_decode_ssc_host(int log2_n, int n_info, const int *info_pos, int messages, int maxq, int n_frames, const void *llr,
                                   const uint32_t *frozen_u, uint32_t *u, uint32_t *info, uint32_t *x);
int    qldpc_polar_ssc_plan_host(int log2_n, int n_info, const int *info_pos, int *steps /* [N/32 or 1][3] */, int *n_steps);

/* ------------------------------------------------------------------------------------------------------------------------------------------
 * Polar codes: the CRC-aided successive-cancellation LIST decoder (qldpc_polar_list_*), beside the SC decoder above and with its sizes, rows,
 * code, messages and inputs.  The definition is csrc/qldpc_polar_list_core.h, shared by the kernels (csrc/qldpc_kernels_polar_list.h) and the
 * host mirror (csrc/qldpc_polar_list_host.c), which agree bit for bit in both message types.  This is the reference's
 * nrpolar_sclistdecode_FP.m (list 4, CRC 11) without its paths of infinite metric, which never change a result.
 *
 *   size      1 <= log2_n <= 16 (QLDPC_ESIZE: the scratch grows with list_size x N); list_size 1, 2, 4 or 8 (QLDPC_ESIZE).
 *   paths     a list holds up to list_size paths, each with a metric >= 0: an exact uint32 with QLDPC_POLAR_I8, a float with QLDPC_POLAR_F32.
 *             One path of metric 0 at the start; leaves in natural order, every path's leaf belief D computed as the SC decoder computes it.
 *   frozen    bit = the frozen value; metric += |D| if (D < 0) != bit.  Nothing is reordered.
 *   info      P live paths give 2P candidates: c < P is path c with bit (D_c < 0) and metric m_c, P + c is path c with the other bit and metric
 *             m_c + |D_c| (one float add).  The new list is the min(list_size, 2P) smallest in the order (metric, candidate index), new path k
 *             the k-th of them, so the list is sorted at every information leaf and only there.
 *   CRC       crc_len 0 .. 32, at most n_info; crc_poly holds the low crc_len coefficients, x^crc_len is implied (QLDPC_ESIZE otherwise).
 *             Register form, zero start, MSB first, no reflection, no final XOR: top = msb(r) ^ bit; r = (r << 1) & mask; if top: r ^= poly.
 *             It runs over a path's n_info information bits in the caller's order (bit m = u[info_pos[m]]).  The reference's CRC11 is
 *             crc_len = 11, crc_poly = 0x621; a word with its CRC appended has remainder 0.
 *   pick      the first path in list order whose remainder is crc[frame] (0 where crc is NULL), or path 0 where none matches; pick[frame] is its
 *             index, or -1.  crc_len = 0: every path matches, pick = 0, and a crc row is refused (QLDPC_EINVAL).  list_size = 1 with
 *             crc_len = 0 is qldpc_polar_decode_* bit for bit in u, info and x.
 *   outputs   each may be NULL: u, info and x of the picked path, shaped and packed as the SC calls'; pick[n_frames]; metric[n_frames][list_size]
 *             the final metrics in list order, uint32 or float, 0xffffffff or +inf past the live paths (2^n_info of them where that is below
 *             list_size); list_x[n_frames][list_size][ceil(N/32)] every path's re-encoded word, zeros past the live paths.
 *
 * A context owns its scratch (qldpc_polar_list_device_bytes: per frame about list_size x (N beliefs + N/4 bytes of bit levels) + N beliefs, and
 * 2 list_size rows); QLDPC_ENOMEM where it does not fit.  A call allocates nothing, is asynchronous on the context's stream and a context is not
 * re-entrant; n_frames = 0 is a no-op; every argument check runs before the first HIP call.  Other refusals as the SC calls'.
 * qldpc_polar_crc_host: Alice's remainder of packed rows of n_bits bits each, rows[n_frames][ceil(n_bits/32)] -> crc[n_frames].
 */
typedef struct qldpc_polar_list qldpc_polar_list;
int    qldpc_polar_list_create(int log2_n, int n_info, const int *info_pos, int messages, int maxq, int list_size,
                               int crc_len, uint32_t crc_poly, int max_frames, int device, qldpc_polar_list **out);
void   qldpc_polar_list_free(qldpc_polar_list *p);
size_t qldpc_polar_list_device_bytes(const qldpc_polar_list *p);
int    qldpc_polar_list_set_stream(qldpc_polar_list *p, void *hip_stream);
int    qldpc_polar_list_decode_dev(qldpc_polar_list *p, int n_frames, const void *d_llr, const uint32_t *d_frozen_u, const uint32_t *d_crc,
                                   uint32_t *d_u, uint32_t *d_info, uint32_t *d_x, int32_t *d_pick, void *d_metric, uint32_t *d_list_x);
/* host mirrors, no device needed */
int    qldpc_polar_list_decode_host(int log2_n, int n_info, const int *info_pos, int messages, int maxq, int list_size, int crc_len,
                                    uint32_t crc_poly, int n_frames, const void *llr, const uint32_t *frozen_u, const uint32_t *crc,
                                    uint32_t *u, uint32_t *info, uint32_t *x, int32_t *pick, void *metric, uint32_t *list_x);
int    qldpc_polar_crc_host(int crc_len, uint32_t crc_poly, int n_bits, int n_frames, const uint32_t *rows, uint32_t *crc);

/*
 * Polar codes: a device-resident Monte-Carlo FER loop (qldpc_polar_mc_*) around an existing qldpc_polar context (either form) or an existing
 * qldpc_polar_list context: source -> (CRC) -> u -> encode -> table channel -> SC or list decode -> monitor, everything queued on the context's
 * stream, ONE small counter read-back per batch.  The definition is csrc/qldpc_polar_mc_core.h, shared by the kernels
 * (csrc/qldpc_kernels_polar_mc.h) and the host mirror (qldpc_polar_mc_frames_host), which agree bit for bit.
 *
 * Frame i (a 64-bit global index) is a pure function of (seed, i, code, CRC, frozen mode, table), whatever the batch, the launch shape or the
 * split of a run into calls:
 *   message   A = n_info - crc_len bits, word j = the LDPC loop's info word (stream 0) of (seed, i, j, A); QLDPC_MC_SOURCE_ZERO: zeros
 *   info row  n_info bits: the message, then its CRC remainder (the list decoder's register form) MSB first, so the row's remainder is 0 and the
 *             list decoder gets no crc row.  An SC context has crc_len = 0.
 *   u         u[info_pos[m]] = info bit m.  QLDPC_POLAR_MC_FROZEN_ZERO: frozen positions 0, no frozen row for the decoder.
 *             QLDPC_POLAR_MC_FROZEN_RANDOM: frozen word w = Philox output word w % 4 at counter (w / 4, 4, i_lo, i_hi), masked to the frozen
 *             positions, and the u row is the decoder's frozen row: the reconciliation form (x is a uniformly random key, the frozen values Alice's).
 *   x         encode(u)
 *   channel   ONE threshold table of 2 .. 256 levels with the semantics of qldpc_mc_set_channel (cum0, cum1 [levels - 1], value [levels]):
 *             position v draws output word v % 4 at counter (v / 4, 3, i_lo, i_hi), level = #{k : u >= cum[x_v][k]}, LLR = value[level].  A
 *             QLDPC_POLAR_I8 context stores (int8)value[level]: every value must be an integer in [-128, 127] (QLDPC_EINVAL otherwise).  A BSC is
 *             the 2-level table {+mag, -mag}.  flips of a frame = positions whose LLR's sign contradicts x_v (an LLR of 0 contradicts nothing).
 *   verdict   be = the wrong bits among the A message bits of the decoder's info row; frame error iff be > 0; crc_fail iff the list decoder's pick
 *             is -1 (never with SC or crc_len = 0); undetected iff a frame error that is no crc_fail.
 *
 * qldpc_polar_mc_create: exactly one of sc and list (not owned: it must outlive the object); batch = 0 means the context's max_frames, more than
 * that is QLDPC_ESIZE; the object allocates everything here, no later call allocates.  qldpc_polar_mc_set_channel: QLDPC_ESIZE for levels outside
 * 2 .. 256, QLDPC_EINVAL for a missing array, a decreasing row, an entry above 2^32 or a value an int8 context cannot store; a refused call leaves
 * the previous table in force.  qldpc_polar_mc_run and _frames_dev without a table: QLDPC_ESTATE.
 * qldpc_polar_mc_frames_dev: frames first_frame .. + n_frames - 1 into d_info [n][ceil(n_info/32)], d_u, d_x [n][ceil(N/32)], d_llr [n][N] int8 or
 * float (16-byte aligned), d_flips [n]; each may be NULL; asynchronous.
 * qldpc_polar_mc_run: batches of `batch` frames (the last ragged) from first_frame until max_frames are done or, checked at a batch boundary,
 * max_frame_errors (0: no such rule) are reached.  counters[QLDPC_POLAR_MC_COUNTERS] by the enum below; ms (optional) [8] by QLDPC_POLAR_MC_MS_*:
 * hipEvent times of the stages summed over the batches, and the wall time of the call.
 * qldpc_polar_mc_failed_frames: the first fail_cap failed global indices of the last run, ascending; copies min(cap, their number), returns their
 * number.  Every argument check runs before the first HIP call; the object is not re-entrant; there is no CPU fallback.
 *
 * qldpc_polar_mc_awgn_table (host only) -> the level count, or a status: BPSK over AWGN of deviation sigma, received value r quantised with
 * rounding = 0: floor(r / rmax maxq) clamped to [-maxq - 1, maxq], 2 maxq + 2 levels, qldpc_mc_awgn_table bit for bit (the SC scripts);
 * rounding = 1: round(clip(r, -rmax, rmax) / rmax maxq), 2 maxq + 1 levels, boundaries (k - maxq + 1/2) rmax / maxq, value[l] = l - maxq (the list
 * script).  cum0, cum1 hold levels - 1 entries, value levels.
 * qldpc_polar_mc_frames_host: the mirror; every output optional; levels = 0 (no table) allows neither llr nor flips (QLDPC_ESTATE).
 */
typedef struct qldpc_polar_mc qldpc_polar_mc;
enum { QLDPC_POLAR_MC_FROZEN_ZERO = 0, QLDPC_POLAR_MC_FROZEN_RANDOM = 1 };
enum { QLDPC_POLAR_MC_FRAMES = 0, QLDPC_POLAR_MC_BIT_ERRORS, QLDPC_POLAR_MC_FRAME_ERRORS, QLDPC_POLAR_MC_UNDETECTED, QLDPC_POLAR_MC_CRC_FAILS,
       QLDPC_POLAR_MC_CHANNEL_FLIPS, QLDPC_POLAR_MC_CHANNEL_BITS, QLDPC_POLAR_MC_BATCHES, QLDPC_POLAR_MC_NEXT_FRAME, QLDPC_POLAR_MC_COUNTERS = 16 };
enum { QLDPC_POLAR_MC_MS_SOURCE = 0, QLDPC_POLAR_MC_MS_ENCODE, QLDPC_POLAR_MC_MS_CHANNEL, QLDPC_POLAR_MC_MS_DECODE, QLDPC_POLAR_MC_MS_MONITOR,
       QLDPC_POLAR_MC_MS_TOTAL };
int    qldpc_polar_mc_create(qldpc_polar *sc, qldpc_polar_list *list, uint64_t seed, int batch, int fail_cap, int frozen_mode, qldpc_polar_mc **out);
void   qldpc_polar_mc_free(qldpc_polar_mc *mc);
size_t qldpc_polar_mc_device_bytes(const qldpc_polar_mc *mc);
int    qldpc_polar_mc_set_source(qldpc_polar_mc *mc, int mode);
int    qldpc_polar_mc_set_channel(qldpc_polar_mc *mc, int levels, const uint64_t *cum0, const uint64_t *cum1, const float *value);
int    qldpc_polar_mc_frames_dev(qldpc_polar_mc *mc, uint64_t first_frame, int n_frames, uint32_t *d_info, uint32_t *d_u, uint32_t *d_x, void *d_llr,
                                 uint32_t *d_flips);
int    qldpc_polar_mc_run(qldpc_polar_mc *mc, uint64_t first_frame, uint64_t max_frames, uint64_t max_frame_errors, uint64_t *counters, double *ms);
int    qldpc_polar_mc_failed_frames(qldpc_polar_mc *mc, uint64_t *frames, int cap);
/* host only, no device needed */
int    qldpc_polar_mc_awgn_table(double sigma, double rmax, int maxq, int rounding, uint64_t *cum0, uint64_t *cum1, float *value);
int    qldpc_polar_mc_frames_host(int log2_n, int n_info, const int *info_pos, int messages, int crc_len, uint32_t crc_poly, int frozen_mode,
                                  int source_mode, uint64_t seed, int levels, const uint64_t *cum0, const uint64_t *cum1, const float *value,
                                  uint64_t first_frame, int n_frames, uint32_t *info, uint32_t *u, uint32_t *x, void *llr, uint32_t *flips);

/*
 * Polar codes: genie-aided code construction (qldpc_polar_tally_*, qldpc_polar_mc_construct, qldpc_polar_construct_*): which positions should
 * carry information on a given channel, by Arikan's Monte-Carlo method.  The rule is csrc/qldpc_polar_tally_core.h, shared by the kernel
 * (csrc/qldpc_kernels_polar_tally.h), the mirror and the helpers (csrc/qldpc_polar_tally_host.c), which agree count for count.
 *
 *   genie     for a frame with true row u_true, L_p is the leaf belief of the SC decoder above with EVERY position frozen to u_true.
 *   tally     position p of the frame is a TIE iff L_p == 0 (a float -0.0 too) and WRONG iff L_p != 0 and (L_p < 0) != u_p.
 *             tally[0][p] counts the wrong frames, tally[1][p] the ties: a row of [2][N] uint64.  Integers only: any order of addition agrees.
 *   score     score[p] = 2 wrong + ties; score / (2 frames) estimates the error probability of position p under a uniformly random bit (a tie
 *             decides 0 and is wrong half the time; counting it as 1/2 takes that coin's variance out).  u_true must be uniformly random.
 *
 * qldpc_polar_tally_dev: d_llr and d_u_true as qldpc_polar_decode_dev's d_llr and d_frozen_u; the counts of the n_frames frames are ADDED to
 * d_tally [2][N] on the device, which is the caller's (zero it first).  Any QLDPC_POLAR_LANES context of the size and the messages; its own
 * information set is ignored.  Asynchronous on the context's stream, allocates nothing, one or two launches, no u, x or leaf row is written.
 * n_frames = 0 is a no-op; a QLDPC_POLAR_WIDE context (n > 5) is QLDPC_EUNSUPPORTED: create a lanes context for the tally; a missing pointer is
 * QLDPC_EINVAL; the other refusals are qldpc_polar_decode_dev's.  Every check runs before the first HIP call.
 * qldpc_polar_tally_host: the mirror, tally ADDED to as well; refusals as qldpc_polar_decode_host's.
 * qldpc_polar_mc_construct: frames first_frame .. + n_frames - 1 of a Monte-Carlo object (the frames qldpc_polar_mc_frames_host mirrors), per
 * batch source -> encode -> channel -> tally against the sent u row, into a [2][N] row the object owns (allocated by create, zeroed here), and
 * ONE read-back at the end of the call into tally (host, overwritten).  Ranges add up and the batch size does not matter.  It needs an SC
 * context of the lanes' form and QLDPC_POLAR_MC_FROZEN_RANDOM (QLDPC_EUNSUPPORTED otherwise), and the random source and a channel table
 * (QLDPC_ESTATE otherwise), so that u is uniformly random at every position.  ms (optional) [8] by QLDPC_POLAR_MC_MS_*: the tally in the
 * decode slot, 0 in the monitor's.
 * qldpc_polar_construct_order_host: order[N] = the positions in ascending reliability (a code of K bits takes the LAST K): the key is (score
 * descending, rank in `prior` ascending); prior[N] is an order of ascending reliability itself, NULL = 0, 1, .., N - 1; QLDPC_EINVAL where it is
 * no permutation.
 * qldpc_polar_construct_k_host: *k = the largest K whose last K positions of `order` (a permutation, QLDPC_EINVAL otherwise) have a score sum
 * <= max_score_sum; for a union bound eps on the frame error rate over `frames` tallied frames that is floor(2 frames eps).
 * Both helpers refuse a count above 2^40 (QLDPC_ESIZE) instead of overflowing.
 */
int    qldpc_polar_tally_dev(qldpc_polar *p, int n_frames, const void *d_llr, const uint32_t *d_u_true, uint64_t *d_tally);
int    qldpc_polar_mc_construct(qldpc_polar_mc *mc, uint64_t first_frame, uint64_t n_frames, uint64_t *tally, double *ms);
/* host only, no device needed */
int    qldpc_polar_tally_host(int log2_n, int messages, int maxq, int n_frames, const void *llr, const uint32_t *u_true, uint64_t *tally);
int    qldpc_polar_construct_order_host(int log2_n, const uint64_t *tally, const int *prior, int *order);
int    qldpc_polar_construct_k_host(int log2_n, const uint64_t *tally, const int *order, uint64_t max_score_sum, int *k);

/*
 * Polar codes: reconciliation sessions (qldpc_polar_recon_*) around an existing qldpc_polar context (any form, any rule) or an existing
 * qldpc_polar_list context with a CRC: Alice's message (syndrome and crc), Bob's prior, decode and verdict, a status per block, the leak.  The rule
 * is csrc/qldpc_polar_recon_core.h, shared by the kernels (csrc/qldpc_kernels_polar_recon.h), the host mirrors (csrc/qldpc_polar_recon_host.c) and
 * the session (csrc/qldpc_polar_recon.hip), which agree bit for bit.
 *
 * A session belongs to one code (the context's log2_n and info_pos[K]) and one CRC (crc_len 1 .. 32, crc_poly; the list decoder's register form,
 * above).  A block is a key of key_bits bits, 1 <= key_bits <= N, packed MSB-first in a row of W = ceil(N / 32) words.
 *   padding   positions key_bits .. N - 1 are 0 for both parties; Alice's side ignores what the caller left there.  (Last-bits shortening with an
 *             unchanged information set.)  On Alice's side a key_bits outside 1 .. N leaves no bit: the message of the all-zero key.
 *   Alice     u = encode(x).  syndrome = the bits of u at the frozen positions in ascending position order, packed MSB-first into
 *             Wf = ceil((N - K) / 32) words, the tail zero.  crc = the remainder over the K bits u[info_pos[m]], m = 0 .. K - 1, the caller's order:
 *             qldpc_polar_crc_host on the decoder's info row.  Leak: N - K + crc_len bits a block.
 *   prior     Bob's LLR of position i < key_bits is +prior where y_i = 0 and -prior where y_i = 1; of i >= key_bits it is +pin.  prior and pin are
 *             the session's, fixed at create: integers 1 <= prior <= pin <= maxq with QLDPC_POLAR_I8, finite 0 < prior <= pin <= 1e30 with
 *             QLDPC_POLAR_F32 (QLDPC_EINVAL otherwise).  No QBER enters: on a BSC every unknown position has one magnitude, and min-sum f and the
 *             additive g do not depend on its scale; magnitude 1 leaves an int8 context the most room before sat.  Nothing is computed.
 *   frozen    Bob's frozen row: the syndrome scattered back to the frozen positions; bits at other positions are 0.
 *   decode    the context's own qldpc_polar_decode_dev, or qldpc_polar_list_decode_dev with Alice's crc row.
 *   verdict   status = QLDPC_OK iff the remainder of the decoded info row equals Alice's crc (SC contexts) or pick >= 0 (list contexts), and every
 *             bit of x^ at positions >= key_bits is 0; QLDPC_EDECODE otherwise.  corrected = popcount((x^ ^ y) over the first key_bits bits) where
 *             OK, else -1.  Bob's key row becomes x^ where OK and is untouched otherwise.  The picked path is the only one looked at.
 *             A block whose key_bits is outside 1 .. N: status QLDPC_ESIZE, corrected -1, the key untouched, its LLR row all +pin.
 *
 * qldpc_polar_recon_create: exactly one of sc and list (QLDPC_EINVAL; not owned: it must outlive the session).  With list the CRC is the context's:
 * crc_len and crc_poly must be 0 and a list context without a CRC is refused (QLDPC_EINVAL).  With sc: crc_len outside 1 .. min(32, K) or
 * polynomial bits above crc_len are QLDPC_ESIZE.  max_blocks = 0 means the context's max_frames; more than that is QLDPC_ESIZE, negative
 * QLDPC_EINVAL.  The session allocates everything here (LLR rows [max_blocks][N], frozen, x, info and pick rows, two position tables): no later
 * call allocates.  _syndrome_words: Wf.  _leaked_bits: N - K + crc_len.
 * qldpc_polar_recon_encode_dev: d_keys [n_blocks][W], d_key_bits [n_blocks] or NULL (every block is N bits) -> d_syndrome [n_blocks][Wf] (may be
 * NULL when K = N), d_crc [n_blocks].  qldpc_polar_recon_decode_dev: d_keys corrected in place, d_status [n_blocks], d_corrected optional, d_pick
 * optional and list only (QLDPC_EINVAL with an SC context).  Both are asynchronous on the wrapped context's stream: nothing crosses the host and
 * the call waits for nothing.  The session is not re-entrant and shares its context's scratch.
 * n_blocks above max_blocks: QLDPC_ESIZE; negative: QLDPC_EINVAL; a missing pointer: QLDPC_EINVAL; n_blocks = 0 is a no-op.  Every argument check of
 * every call runs before the first HIP call.
 *
 * The building blocks on their own; the _dev forms take a hip_stream (NULL = the null stream) on the current device and no session, the code
 * arrives as device tables (qldpc_polar_recon_tables_host: frozen_mask [W] 1 = frozen, frozen_prefix [W] the frozen positions before each word,
 * frozen_pos [N - K] ascending; each may be NULL):
 *   _prior_dev / _prior_host      keys, key_bits, syndrome -> llr [n_blocks][N] int8 or float (16-byte aligned on the device), frozen [n_blocks][W]
 *   _verdict_dev / _verdict_host  info [n_blocks][ceil(K/32)], x [n_blocks][W], pick or NULL (then crc_len, crc_poly and crc decide), keys,
 *                                 key_bits, crc -> status, corrected (optional), keys
 * qldpc_polar_recon_encode_host and _decode_host: the mirrors of the two session calls, no device; _decode_host runs the host decoder that
 * (form, rule, list_size) name between the prior mirror and the verdict mirror: list_size = 0 is qldpc_polar_decode_host, _decode_wide_host or
 * _decode_ssc_host, 1, 2, 4, 8 qldpc_polar_list_decode_host (form = rule = 0); pick is optional and list only.
 */
typedef struct qldpc_polar_recon qldpc_polar_recon;
int    qldpc_polar_recon_create(qldpc_polar *sc, qldpc_polar_list *list, int crc_len, uint32_t crc_poly, double prior, double pin, int max_blocks,
                                qldpc_polar_recon **out);
void   qldpc_polar_recon_free(qldpc_polar_recon *r);
size_t qldpc_polar_recon_device_bytes(const qldpc_polar_recon *r);
int    qldpc_polar_recon_syndrome_words(const qldpc_polar_recon *r);
int    qldpc_polar_recon_leaked_bits(const qldpc_polar_recon *r);
int    qldpc_polar_recon_encode_dev(qldpc_polar_recon *r, int n_blocks, const uint32_t *d_keys, const int *d_key_bits, uint32_t *d_syndrome, uint32_t *d_crc);
int    qldpc_polar_recon_decode_dev(qldpc_polar_recon *r, int n_blocks, uint32_t *d_keys, const int *d_key_bits, const uint32_t *d_syndrome,
                                    const uint32_t *d_crc, int *d_status, int *d_corrected, int32_t *d_pick);
int    qldpc_polar_recon_prior_dev(void *hip_stream, int log2_n, int n_frozen, const uint32_t *d_frozen_mask, const int *d_frozen_prefix, int messages, int maxq,
                                   double prior, double pin, int n_blocks, const uint32_t *d_keys, const int *d_key_bits, const uint32_t *d_syndrome, void *d_llr,
                                   uint32_t *d_frozen);
int    qldpc_polar_recon_verdict_dev(void *hip_stream, int log2_n, int n_info, int crc_len, uint32_t crc_poly, int n_blocks, const uint32_t *d_info,
                                     const uint32_t *d_x, const int32_t *d_pick, uint32_t *d_keys, const int *d_key_bits, const uint32_t *d_crc, int *d_status,
                                     int *d_corrected);
/* host mirrors, no device needed */
int    qldpc_polar_recon_tables_host(int log2_n, int n_info, const int *info_pos, uint32_t *frozen_mask, int *frozen_prefix, int *frozen_pos);
int    qldpc_polar_recon_encode_host(int log2_n, int n_info, const int *info_pos, int crc_len, uint32_t crc_poly, int n_blocks, const uint32_t *keys,
                                     const int *key_bits, uint32_t *syndrome, uint32_t *crc);
int    qldpc_polar_recon_decode_host(int log2_n, int n_info, const int *info_pos, int messages, int maxq, int form, int rule, int list_size, int crc_len,
                                     uint32_t crc_poly, double prior, double pin, int n_blocks, uint32_t *keys, const int *key_bits, const uint32_t *syndrome,
                                     const uint32_t *crc, int *status, int *corrected, int32_t *pick);
int    qldpc_polar_recon_prior_host(int log2_n, int n_info, const int *info_pos, int messages, int maxq, double prior, double pin, int n_blocks,
                                    const uint32_t *keys, const int *key_bits, const uint32_t *syndrome, void *llr, uint32_t *frozen);
int    qldpc_polar_recon_verdict_host(int log2_n, int n_info, int crc_len, uint32_t crc_poly, int n_blocks, const uint32_t *info, const uint32_t *x,
                                      const int32_t *pick, uint32_t *keys, const int *key_bits, const uint32_t *crc, int *status, int *corrected);

/* ------------------------------------------------------------------------------------------------------------------------------------------
 * Polar reconciliation sessions: INCREMENTAL FREEZING.  A block that failed is decoded again with more positions of the same code frozen, to
 * bits of u that Alice discloses in a fixed public order; only the blocks that failed need it, and the blocks of one call may sit at different
 * rates.  The rule is csrc/qldpc_polar_ladder_core.h on top of the session's, shared by the kernels (csrc/qldpc_kernels_polar_ladder.h), the
 * host mirrors (csrc/qldpc_polar_ladder_host.c) and the session, which agree bit for bit.  The CRC still holds: a frozen information position
 * decodes to Alice's bit.
 *
 *   ladder    extra_pos[E], 0 <= E <= K: distinct information positions of the session's code in the order in which they are given up (the caller
 *             would pass the least reliable first, e.g. the head of qldpc_polar_construct_order_host's order restricted to info_pos).  Per block an
 *             integer extra in 0 .. E: its first `extra` entries are frozen for that block.  The sets are nested.
 *   Alice     besides syndrome and crc: extra_bits [n_blocks][We], We = ceil(E / 32), the bits of u at extra_pos[0 .. E), MSB-first, the tail zero.
 *             She sends a prefix of that row per round; slicing it is the caller's business.
 *   Bob       a round decodes the OPEN blocks: their LLR rows, frozen values (the syndrome scattered back plus the first extra[b] bits of the
 *             block's extra_bits row at their positions) and added frozen flags go to slots 0 .. n_open - 1, qldpc_polar_decode_rows_dev runs on
 *             n_open frames, and slot i's verdict (the session's, unchanged) goes to block open[i].  After a failed decode at extra = e: if e < E
 *             and another round is allowed, extra <- min(E, e + step) and the block stays open; otherwise it is closed as QLDPC_EDECODE.  No bit of
 *             an extra_bits row at or beyond the block's extra is looked at: in a real exchange Bob does not have them yet.
 *   leak      of a block: qldpc_polar_recon_leaked_bits(r) + d_extra[b] as the call returns it.
 *
 * qldpc_polar_recon_create_ladder: qldpc_polar_recon_create around an SC context of the lanes form and the SC rule (a wide or an SSC context:
 * QLDPC_EUNSUPPORTED; there is no list argument, the list decoder has no rows form), plus the ladder.  n_extra outside 0 .. K: QLDPC_ESIZE; an
 * entry that comes twice or is no information position: QLDPC_EINVAL.  Everything the new calls need is allocated here, in the session's ledger
 * (the positions, their rank table [N], the flag rows [max_blocks][W], two open lists and their counters); no later call allocates.  The
 * existing calls work on such a session exactly as on a plain one.  n_extra = 0 is allowed: every call below then behaves as its plain
 * counterpart.  _extra_words: We (0 for a session without a ladder).
 * qldpc_polar_recon_encode_ladder_dev: _encode_dev plus d_extra_bits [n_blocks][We] (may be NULL when E = 0).  Asynchronous as _encode_dev.
 * qldpc_polar_recon_decode_rounds: up to max_rounds rounds.  d_extra [n_blocks] is read and written: with resume = 0 every block with a valid
 * key_bits is open in round 0 at the d_extra given; with resume = 1 d_status is read on entry and only the blocks whose status is QLDPC_EDECODE
 * are open, at the d_extra given, and every other block's status, corrected, key and extra are left alone.  A candidate whose key_bits is outside
 * 1 .. N or whose d_extra is outside 0 .. E gets QLDPC_ESIZE (corrected -1), is never open and is otherwise untouched.  On return d_extra[b] is the
 * count the block's last decode ran with, d_decodes[b] (optional) its decodes in this call, open_per_round[t] (host, optional, [max_rounds]) the
 * blocks decoded in round t, 0 from the round in which nothing was open.  With max_rounds = 1 and resume = 1 the call is the protocol's single
 * round after Alice's next answer: the caller raises d_extra himself.  R rounds in one call are R such calls.
 * THIS CALL WAITS (of a session's calls only this one and qldpc_polar_recon_decode_flip do): the grid of a round needs the open count on the host, one 4-byte read-back per round,
 * queued on the context's stream and waited for on that stream only, never the device.  The loop ends at the first round with nothing open.
 * step < 1, max_rounds < 1, resume outside 0 / 1: QLDPC_EINVAL; a session without a ladder: QLDPC_ESTATE; a missing required pointer
 * (d_keys, d_crc, d_status, d_extra; d_syndrome where K < N; d_extra_bits where E > 0): QLDPC_EINVAL; all before the first HIP call.
 *
 * The mirrors, no device: _encode_ladder_host and _decode_rounds_host take the code and the ladder explicitly and run qldpc_polar_decode_rows_host.
 * qldpc_polar_recon_ladder_extra_host -> a starting count for a block of key_bits bits at a given QBER, or a negative status: the count at which
 * the block has leaked f times the Slepian-Wolf bound, clamp(ceil(f h2(qber) key_bits) - (N - K), 0, n_extra).  A pure function; the session
 * never calls it and nothing gets a default.  QLDPC_ESIZE: the sizes; QLDPC_EINVAL: qber outside 0 .. 0.5, f outside 0 .. 1e6.
 */
int    qldpc_polar_recon_create_ladder(qldpc_polar *sc, int crc_len, uint32_t crc_poly, double prior, double pin, int max_blocks, int n_extra,
                                       const int *extra_pos, qldpc_polar_recon **out);
int    qldpc_polar_recon_extra_words(const qldpc_polar_recon *r);
int    qldpc_polar_recon_encode_ladder_dev(qldpc_polar_recon *r, int n_blocks, const uint32_t *d_keys, const int *d_key_bits, uint32_t *d_syndrome,
                                           uint32_t *d_crc, uint32_t *d_extra_bits);
int    qldpc_polar_recon_decode_rounds(qldpc_polar_recon *r, int n_blocks, uint32_t *d_keys, const int *d_key_bits, const uint32_t *d_syndrome,
                                       const uint32_t *d_crc, const uint32_t *d_extra_bits, int *d_extra, int step, int max_rounds, int resume,
                                       int *d_status, int *d_corrected, int *d_decodes, int *open_per_round);
/* host mirrors, no device needed */
int    qldpc_polar_recon_encode_ladder_host(int log2_n, int n_info, const int *info_pos, int crc_len, uint32_t crc_poly, int n_extra, const int *extra_pos,
                                            int n_blocks, const uint32_t *keys, const int *key_bits, uint32_t *syndrome, uint32_t *crc, uint32_t *extra_bits);
int    qldpc_polar_recon_decode_rounds_host(int log2_n, int n_info, const int *info_pos, int messages, int maxq, int crc_len, uint32_t crc_poly, double prior,
                                            double pin, int n_extra, const int *extra_pos, int n_blocks, uint32_t *keys, const int *key_bits,
                                            const uint32_t *syndrome, const uint32_t *crc, const uint32_t *extra_bits, int *extra, int step, int max_rounds,
                                            int resume, int *status, int *corrected, int *decodes, int *open_per_round);
int    qldpc_polar_recon_ladder_extra_host(int log2_n, int n_info, int n_extra, int key_bits, double qber, double f);

/* ------------------------------------------------------------------------------------------------------------------------------------------
 * Polar reconciliation sessions: SC-FLIP TRIALS (Afisiadis, Balatsoukas-Stimming, Burg 2014).  A block whose decode failed the verdict is
 * decoded again with the decision at one of its T least reliable information leaves inverted; the first trial that passes the verdict is kept.
 * Local to Bob: no packet, and the leak of a block is what it was.  Successive cancellation is causal, so "decode with the decision at p
 * inverted" is "decode with p frozen to the inverse of SC's decision": a trial is one more frame of qldpc_polar_decode_rows_dev.  The rule is
 * csrc/qldpc_polar_flip_core.h on top of the ladder's and the session's, shared by the kernels (csrc/qldpc_kernels_polar_flip.h), the host
 * mirrors (csrc/qldpc_polar_flip_host.c) and the session, which agree bit for bit.
 *
 *   candidate  position i of a block: the code does not freeze it and the block's ladder count does not add it.
 *   key        (mag << 32) | i.  int8 leaves: mag = |leaf| (0 .. 127).  float leaves: mag = the bit pattern of fabsf(leaf); -0.0 and +0.0 give 0.
 *   flips      the T smallest keys of the block, ascending: ties in magnitude go to the lower position (with a BSC prior ties are the normal
 *              case; the order is part of the contract).  With fewer than T candidates the remaining entries are -1: void.
 *   trial t    the block's inputs plus position p_t frozen to (leaf[p_t] >= 0), the inverse of SC's decision (leaf < 0).  A void trial is never
 *              accepted.
 *   settle     the winner is the lowest t whose trial passes the session's verdict test (CRC match and clean pad).  The block then is QLDPC_OK,
 *              its key row that trial's x^, corrected the flips against Bob's row, flip_pos = p_t.  Without a winner: QLDPC_EDECODE, the key
 *              untouched, corrected -1, flip_pos -1.  Either way the block's decode count goes up by 1 + T (a probe and T trials).
 *   THE PRICE  a block now meets up to 1 + T CRC tests, so the chance that a wrong key passes is bounded by (1 + T) 2^-crc_len instead of
 *              2^-crc_len.  Use a CRC-32, or verify with a keyed tag afterwards (qldpc_polyhash_*).
 *
 * qldpc_polar_recon_create_flip: qldpc_polar_recon_create_ladder (its arguments, its refusals; n_extra = 0 is allowed and the common case) plus
 * the scratch of the trials.  max_flips not a power of two in 1 .. 32: QLDPC_EINVAL; above max_blocks (0: the context's max_frames): QLDPC_ESIZE.
 * The trials of a call live in the rows its blocks live in (LLR, frozen, flags, info and x rows [max_blocks][..]), so a call with n_flips = T
 * takes the open blocks in chunks of C = max_blocks / T.  Besides those the session owns, in its ledger, the leaf rows of one chunk's probe and
 * the flips of its trials.  The leaf buffer is sized for the worst case a call can meet, n_flips = 1 where a chunk is max_blocks blocks:
 * [max_blocks][N] leaves; the flips are C T <= max_blocks entries.  No later call allocates.  Every existing call works on such a session as on
 * a ladder session.  _max_flips: the session's max_flips, 0 for any other session.
 * qldpc_polar_recon_decode_flip: with resume = 0 every block with a valid key_bits and count is decoded once at its d_extra, exactly
 * qldpc_polar_recon_decode_rounds with max_rounds = 1, and the blocks that fail form the open list; with resume = 1 d_status is read and the open
 * list is the blocks whose status is QLDPC_EDECODE; every other block is left alone but for its decode count (0) and flip_pos (-1), so the call
 * composes after _decode_dev or _decode_rounds.  A candidate with a key_bits outside 1 .. N or a count outside 0 .. n_extra gets QLDPC_ESIZE as
 * there.  The open blocks then go chunk by chunk through: slot prior, a probe (the failed decode again, for its leaf beliefs: the first pass
 * stays the existing call's and no leaf row is kept for the blocks that pass), select, trial prior on C T slots, rows decode, settle.  d_extra
 * [n_blocks] is only read, NULL = all 0.  d_flip_pos [n_blocks] is required: -1 for every block not rescued by a flip, the blocks that were OK
 * at once included.  d_corrected and d_decodes are optional; n_tried (host, optional) = the open count.  THIS CALL WAITS ONCE: one 4-byte
 * read-back of the open count on the context's stream; after it everything is queued and the call returns.  Chunking shows in no output.
 * n_flips not a power of two or resume outside 0 / 1: QLDPC_EINVAL; n_flips above the session's max_flips: QLDPC_ESIZE; a session not made by
 * _create_flip: QLDPC_ESTATE; a missing required pointer (d_keys, d_crc, d_status, d_flip_pos; d_syndrome where K < N; d_extra_bits where
 * n_extra > 0): QLDPC_EINVAL; all before the first HIP call.
 *
 * The select on its own: qldpc_polar_flip_select_dev (hip_stream, NULL = the null stream, on the current device) and _host: d_leaf
 * [n_frames][N] int8 or float as qldpc_polar_decode_dev's d_leaf gives them (16-byte aligned on the device), d_frozen_mask [W] (1 = frozen),
 * d_rank [N] a ladder's rank table or NULL (no ladder), d_extra [n_frames] or NULL (all 0; not looked at without d_rank) -> d_pos
 * [n_frames][n_flips]; n_flips a power of two (QLDPC_EINVAL) up to 32 (QLDPC_ESIZE).  T successive minima of the key, not a radix select: T is small and the output is an ordered list.
 * qldpc_polar_recon_decode_flip_host: the mirror, _decode_rounds_host's code and ladder arguments plus n_flips, resume and flip_pos; it runs
 * qldpc_polar_decode_rows_host, a block at a time, with no device and no chunking.
 */
int    qldpc_polar_recon_create_flip(qldpc_polar *sc, int crc_len, uint32_t crc_poly, double prior, double pin, int max_blocks, int n_extra,
                                     const int *extra_pos, int max_flips, qldpc_polar_recon **out);
int    qldpc_polar_recon_max_flips(const qldpc_polar_recon *r);
int    qldpc_polar_recon_decode_flip(qldpc_polar_recon *r, int n_blocks, uint32_t *d_keys, const int *d_key_bits, const uint32_t *d_syndrome,
                                     const uint32_t *d_crc, const uint32_t *d_extra_bits, const int *d_extra, int n_flips, int resume, int *d_status,
                                     int *d_corrected, int32_t *d_flip_pos, int *d_decodes, int *n_tried);
int    qldpc_polar_flip_select_dev(void *hip_stream, int log2_n, int messages, int n_frames, const void *d_leaf, const uint32_t *d_frozen_mask,
                                   const int *d_rank, const int *d_extra, int n_flips, int *d_pos);
/* host mirrors, no device needed */
int    qldpc_polar_flip_select_host(int log2_n, int messages, int n_frames, const void *leaf, const uint32_t *frozen_mask, const int *rank,
                                    const int *extra, int n_flips, int *pos);
int    qldpc_polar_recon_decode_flip_host(int log2_n, int n_info, const int *info_pos, int messages, int maxq, int crc_len, uint32_t crc_poly, double prior,
                                          double pin, int n_extra, const int *extra_pos, int n_blocks, uint32_t *keys, const int *key_bits,
                                          const uint32_t *syndrome, const uint32_t *crc, const uint32_t *extra_bits, const int *extra, int n_flips, int resume,
                                          int *status, int *corrected, int32_t *flip_pos, int *decodes, int *n_tried);

#ifdef __cplusplus
}
#endif
#endif /* QLDPC_H */
