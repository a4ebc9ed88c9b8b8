/*
 * qldpc_engine_int.h -- internals shared by the translation units of the decoder (not part of the C ABI): the decoder object (its memory
 * is in one ledger, qldpc_devmem.h), the per-generation state of the early-exit run, the state and the entry points of the edge-parallel engine
 * (qldpc_engine_edge.hip), and the kernel-launch dispatchers.  The dispatchers instantiate every
 * (frames per lane, degree cap, rule family, message type) variant of the hot kernels; they are compiled once per frames-per-lane
 * value (qldpc_launch.hip with -DQL_V=1|2|4) so that the build runs in parallel.
 */
#ifndef QLDPC_ENGINE_INT_H
#define QLDPC_ENGINE_INT_H

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <vector>

#include "qldpc_hip.h"
#include "qldpc_devmem.h"
#include "qldpc_kernels.h"
#include "qldpc_kernels_i8.h"
#include "qldpc_kernels_gang.h"
#include "qldpc_kernels_giveup.h"

enum { KS_CN = 0, KS_VN, KS_LAYER, KS_SYND, KS_STATUS, KS_LOAD, KS_FETCH, KS_VLAYER, KS_LAYER_REMAP, KS_COMPACT_ROWS, KS_LAYER_GANG, KS_COUNT };
static const char *const ks_names[KS_COUNT] = {"cn_update", "vn_update", "layer_update", "syndrome", "status", "load", "fetch", "vn_vlayer", "layer_update_remap", "compact_rows", "layer_update_gang"};

struct prof_rec { int kind; double bytes, moved; hipEvent_t a, b; };

struct bucket { int cap; int n; int *d_list; int *d_rec; };   /* cap = register-resident degree bound, 0 = any degree */
/* d_rec (layer buckets with cap > 0, else NULL): entry i of the list as ONE aligned record {check, first edge, degree, 0, vn[0 .. cap)} --
 * a wave of a layer kernel learns everything it needs to ask for its rows in one scalar round trip instead of three dependent ones
 * (list -> cn_ptr -> cn_var); the launches of a layered sweep are small and bound by the latency of that chain (DESIGN section 8 #6h);
 * QK_REC_HDR (qldpc_kernels.h) = 4 header words */

/* The information VNs of ONE degree (<= QK_FPV_DMAX) as qk_vn_fpost reads them (qldpc_kernels_fpost.h): entry i is the aligned record
 * {v, row[0 .. deg)}, row[k] = vn_tr[vn_ptr[v] + k], QK_FPV_STRIDE(deg) ints.  Classes by exact degree, not by bucket: the cap-4 bucket of
 * an IRA code holds its degree-3 VNs and, where the edge count does not divide, one of degree 4 */
struct fp_vn_class { int deg; int n; int *d_rec; };

/*
 * Per-frame state of one generation of the early-exit run (qldpc_kernels_compact.h).  Generation 0 is the batch as loaded (its
 * pointers alias the decoder's base arrays); every compaction opens the next one with fewer groups.  A retired generation
 * keeps the results of the frames that converged in it.
 */
struct gen_state {
    int G, cap;                          /* groups in use / allocated */
    u64 *sgn, *hard, *unsat, *done, *ybits, *synd, *ebits;
    int *depth, *iters, *origin, *src;   /* origin[slot] = frame index in the caller's batch (-1: padding); src[slot] = slot in the previous generation */
    float *fmag; int *fnch;
    float *llr; uint32_t *llr8;          /* channel LLR rows in this generation's layout (NULL with coded LLRs, and in a layered run: not read after var_nodes = Y_N) */
    int *gu_last, *gu_best, *gu_since; u64 *gu_gave;   /* give-up state of this generation's frames (NULL with giveup_patience = 0) */
    float *post, *msg;                   /* layered schedule: posteriors and messages / check state of this generation (flooding: NULL past generation 0, its arrays are re-used in place) */
};
#define QLDPC_MAX_GENS 6

/* What the edge-parallel engine (one block at a time, lanes over edges: qldpc_engine_edge.hip) keeps beside the decoder's shared fields.  It reads the
 * graph arrays and d_llr [F][N], d_a = v2c / d_b = c2v [F][E] (the frames engine lays the same three names out as [G][..][FG]) */
struct edge_state {
    int eW, eS, e_stride;
    size_t e_lds;
    uint32_t *e_sgn, *e_hard;
    float *e_c2v1;                   /* odd-iteration chk_to_var buffer (d_b is the even one) */
    int *e_unsat, *e_done_at;
    uint32_t *e_synd;                /* packed target syndromes [F][Wm], NULL until used */
    int *h_done;
    hipEvent_t e_ev[2];
    int use_graphs, graph_frames;
    int persist, persist_blocks;     /* one cooperative launch per decode (qe_persist): enabled / co-resident workgroups (0 = not probed yet) */
    int *e_ctl;                      /* control words of the one-launch decode (qe_xcd): claim / rank / barrier / fault words and its iteration count */
    hipStream_t cap_stream;
    std::vector<hipGraphExec_t> e_graphs;   /* one per chunk of poll_every iterations */
};

struct qldpc_decoder {
    qldpc_decoder_cfg cfg;
    int N, M, E, K;
    int V, FG, G;
    int device;
    hipStream_t stream;
    /* graph on device */
    int *d_cn_ptr, *d_cn_tr, *d_cn_var, *d_vn_ptr, *d_info_pos;
    int *d_vn_tr;                    /* VN-major slot -> CN-major edge (inverse of cn_tr, padded): where chk_to_var of a slot lives */
    int *d_cn_var_t, max_dc;         /* cn_var transposed to [edge position][check], -1 padded (syndrome pass) */
    std::vector<bucket> cn_buckets, vn_buckets;
    std::vector<std::vector<bucket>> layer_buckets;   /* per layer */
    int n_layers;
    /* vertical-layered schedule (qldpc_kernels_vl.h): one list per class of check-disjoint VNs, the check of every VN-major slot, and the rows a
     * sweep moves per frame (it recomputes a check's fold for each of its VNs: 2 sum dc^2 - E + N read, E + N written) */
    std::vector<bucket> vlayer_classes;
    int *d_vn_chk;
    double vl_rows;
    /* one launch per sweep for small batches (qldpc_kernels_chain.h): execution order, per-edge {dv, rank}, per-VN version counters, ticket / fault words */
    int layer_cst;      /* layered min-sum keeps {cst1, cst2} per check and two ballot words per edge instead of dc messages (qldpc_kernels_cst.h) */
    int chain, chain_blocks, chain_lds; int *d_chain_order, *d_chain_dep, *d_chain_ver, *d_chain_ctl;
    /* decoder gangs (qldpc_kernels_gang.h): what a solo layer launch passes as arguments, once per (layer, bucket), written when the decoder first
     * joins a gang; the entry of layer_buckets[l][k] is d_gang[gang_off[l] + k] */
    qk_gang_entry *d_gang; std::vector<int> gang_off;
    /* the posterior form of a fixed-iteration flooding min-sum run (qldpc_kernels_fpost.h), decided once at creation: the VN passes write one
     * posterior row per information VN, the checks keep three state rows each (two buffers, ping-pong by iteration parity) and fold the IRA chain in */
    int fpost, ira_K;
    std::vector<bucket> fp_vn_buckets;   /* the information VNs 0 .. ira_K - 1 */
    std::vector<fp_vn_class> fp_vn_classes;   /* the same VNs by degree, for the in-between pass (empty with QLDPC_FLOOD_POST_VN=0) */
    uint32_t *d_fp_chain;            /* [M] chain table (qldpc_code_chain_table) */
    float *fp_post, *fp_st[2];       /* [G][N][64] posteriors, 2 x [G][M][3][64] check state: carved out of d_a (var_to_chk is not used) where they fit, else d_fp_mem */
    float *d_fp_mem;
    int fp_last;                     /* the state buffer the last check pass of the run wrote */
    int fp_between;                  /* set around the in-between posterior passes: nobody reads their ballots */
    int fp_vn;                       /* the in-between posterior passes run on qk_vn_fpost (QLDPC_FLOOD_POST_VN=0: on qk_vn_flood, a launch per bucket) */
    int layer_first;                 /* layered fp32 run, sweep 0, messages not frozen: the layer kernels treat the messages as zero instead of reading a cleared array */
    /* state */
    float *d_llr, *d_a, *d_b;        /* flooding: a = v2c, b = c2v ; layered: a = post, b = msg */
    float *d_post;                   /* lazily allocated by fetch_post */
    u64 *d_sgn, *d_hard, *d_unsat, *d_done;
    int *d_depth, *d_iters, *d_active;   /* d_active[0] = groups, [1] = frames still unconverged after the last status pass */
    int *h_active, *h_active_dev;    /* mapped pinned memory {groups, frames, sequence number} and its device address: qk_status reports, the host spins */
    int poll_seq;
    unsigned long long *d_work;      /* group-iterations executed in the current run (qk_status) */
    /* cfg.giveup_patience > 0 (qldpc_kernels_giveup.h): the current generation's give-up state; gu.weight [G0][FG] serves every generation.  All NULL with
     * the option off, and the run launches qk_syndrome / qk_status / qk_status_init as ever */
    qk_giveup gu;
    /* active-frame compaction: generations of the per-frame state; the d_* pointers above and G are the CURRENT generation's */
    int G0;
    std::vector<gen_state> gens;     /* [0] aliases the base arrays */
    int cur_gen, compact_mode, compactions;
    int live_lanes;                  /* lanes of the groups still active at the last poll (byte accounting of the profile; 0 = not polled yet) */
    float compact_ratio;             /* compact when the active frames fit into <= ratio * G groups */
    const int *remap_src;            /* != NULL: the next check pass reads var_to_chk (layered: the next sweep reads the messages) through this map (set by a compaction) */
    const float *remap_msg;          /* layered: the previous generation's message / check-state array that sweep reads */
    int *d_gcount, *d_goff;          /* [G0], [G0 + 1] */
    int llr_alt_cap[2]; float *d_llr_alt[2]; uint32_t *d_llr8_alt[2];   /* side buffers for compacted LLR rows (generations ping-pong between them; capacity in groups) */
    int lay_alt_cap[2]; float *d_post_alt[2], *d_msg_alt[2];            /* layered: side buffers of the posteriors and messages of generations >= 1 (ping-pong by generation parity: the
                                                                         * layer kernels update in place, so a generation cannot be written over the one it is read from) */
    dm_ledger mem;                   /* every live allocation of the decoder and of its edge engine (qldpc_devmem.h); a second name of a block (d_hard with 8-bit messages) is not in it */
    int n_frames;                    /* loaded */
    int loaded, ran;
    int last_iters;
    int poll_every;
    u64 *d_synd;                     /* [G][M][V] target-syndrome ballots (syndrome form), NULL until used */
    int has_synd;
    float *h_in; int *h_out;         /* device staging of qldpc_decode_siho's host vectors */
    int msg_half;                    /* 1: v2c / c2v stored as binary16 (flooding, frames engine) */
    /* coded channel LLRs (flooding, fp32 / binary16 messages, after qldpc_load_bits_*): no LLR array is read, see qk_coded_llr */
    u64 *d_ybits; float *d_fmag; int *d_fnch; uint8_t *d_vcls; int llr_coded;
    u64 *d_ebits; int has_erase;     /* [G][N][V] per-frame erasure ballots of the coded form (allocated on first use), set by qldpc_load_erasures_dev */
    uint32_t *d_known; int has_known; /* [2][max_frames][ceil(N/32)] known / value masks of qldpc_load_known_dev (allocated on first use): kept so that erasures loaded later leave them standing */
    int post_closes_run;             /* set around the _compute_post that ends an early-exit run (not for posterior read-back) */
    int packed_h16;                  /* binary16 variant: use the packed check-node kernel when V == 2 (QLDPC_PACKED_H16=0 turns it off) */
    int msg_i8;                      /* 1: 8-bit fixed-point messages and integer arithmetic (flooding min-sum family, frames engine, V = 4) */
    uint32_t *d_llr8;                /* [G][N][256] quantised channel LLRs, four frames of a lane per dword */
    float quant_scale;
    int freeze;                      /* 1: lane-masked stores keep converged frames' messages bit-frozen (exact posteriors, slower) */
    int engine;
    edge_state edge;
    /* profiling */
    int prof_on;
    std::vector<prof_rec> prof_pending;
    qldpc_kernel_stat stats[KS_COUNT];
};

static inline int words32(int n) { return (n + 31) / 32; }

/* a batch is in place (qldpc_load_llr_dev, qldpc_load_bits_*; begin_load in qldpc_engine.hip opens the call) */
static inline void end_load(qldpc_decoder *d) { d->loaded = 1; d->ran = 0; }

/* the plain environment overrides of a decoder: *y = the variable's value where it is set, as it stands or as a flag */
static inline void env_int(const char *name, int *y) { if (const char *e = getenv(name)) *y = atoi(e); }
static inline void env_flag(const char *name, int *y) { if (const char *e = getenv(name)) *y = atoi(e) ? 1 : 0; }

static inline int grid_x(int n_items, int per_wave)
{
    const int per_block = QK_WAVES * per_wave;
    return std::max(1, (n_items + per_block - 1) / per_block);
}

static inline int family_of(int rule)
{
    switch (rule) {
    case QLDPC_RULE_MS: case QLDPC_RULE_OMS: case QLDPC_RULE_NMS: return QK_FAM_MS;
    case QLDPC_RULE_SPA: return QK_FAM_SPA;
    case QLDPC_RULE_LSPA: return QK_FAM_LSPA;
    default: return QK_FAM_AMS;
    }
}

/* the rule in quantiser units (qldpc.h: quant_scale) */
static inline qi_rule qi_rule_of(const qldpc_decoder *d)
{
    qi_rule qr{d->cfg.rule, 0};
    if (d->cfg.rule == QLDPC_RULE_OMS) qr.param = (int)lrintf(d->cfg.rule_param * d->quant_scale);
    if (d->cfg.rule == QLDPC_RULE_NMS) qr.param = (int)lrintf(d->cfg.rule_param * 128.0f);
    qr.param = std::min(128, std::max(0, qr.param));
    return qr;
}

/* what the launchers hand to the kernels again and again: the target syndromes of the syndrome form (NULL: H x = 0), the rule, the coded channel LLRs */
static inline const u64 *target_synd(const qldpc_decoder *d) { return d->has_synd ? d->d_synd : nullptr; }
static inline qk_rule rule_of(const qldpc_decoder *d) { return qk_rule{d->cfg.rule, d->cfg.rule_param}; }
static inline qk_coded_llr coded_llr_of(const qldpc_decoder *d) { return qk_coded_llr{d->d_ybits, d->d_fmag, d->d_fnch, d->d_vcls, d->has_erase ? d->d_ebits : nullptr}; }

/* the in-between variable-node passes only need to leave ballots when the syndrome test reads them; _compute_post always does */
static inline int want_ballots(const qldpc_decoder *d, int mode)
{
    if (mode == QK_VN_POST && d->fp_between) return 0;
    if (mode == QK_VN_POST) return 1 | (d->post_closes_run ? 2 : 0);      /* bit 1: skip groups that converged as a whole (their ballots are final) */
    return d->cfg.enable_syndrome ? 1 : 0;
}

/* one profile record around the launches of a scope (qldpc_profile_read folds them) */
struct prof_scope {
    qldpc_decoder *d; int kind; double bytes, moved; hipEvent_t a, b; bool on;
    prof_scope(qldpc_decoder *d_, int kind_, double bytes_, double moved_ = -1.0) : d(d_), kind(kind_), bytes(bytes_), moved(moved_ < 0.0 ? bytes_ : moved_), a(nullptr), b(nullptr), on(d_->prof_on != 0)
    {
        if (on) { (void)hipEventCreate(&a); (void)hipEventCreate(&b); (void)hipEventRecord(a, d->stream); }
    }
    ~prof_scope()
    {
        if (on) { (void)hipEventRecord(b, d->stream); d->prof_pending.push_back({kind, bytes, moved, a, b}); }
    }
};

/* algorithmic bytes: only live (non-padding) frames are counted */
static inline double msg_b(const qldpc_decoder *d) { return d->msg_i8 ? 1.0 : (d->msg_half ? 2.0 : 4.0); }
static inline double llr_b(const qldpc_decoder *d) { return d->msg_i8 ? 1.0 : 4.0; }
/* frames the next launches work on: all loaded frames, or -- once the early-exit loop has polled -- the lanes of the groups still active */
static inline double live_frames(const qldpc_decoder *d) { return (double)(d->live_lanes > 0 && d->live_lanes < d->n_frames ? d->live_lanes : d->n_frames); }
static inline double bytes_cn(const qldpc_decoder *d) { return 2.0 * d->E * msg_b(d) * live_frames(d); }
static inline double bytes_vn(const qldpc_decoder *d, int mode)
{
    if (mode != QK_VN_NORMAL) return ((double)d->E * msg_b(d) + d->N * llr_b(d)) * live_frames(d);      /* FIRST writes the messages only, POST reads them only */
    return (2.0 * d->E * msg_b(d) + d->N * llr_b(d)) * live_frames(d);
}

/*
 * The edge-parallel engine (qldpc_engine_edge.hip): its half of the entry points of the C ABI.  Each entry point of qldpc_engine.hip checks its
 * arguments and the call sequence, then hands a decoder with engine == QLDPC_ENGINE_EDGES over.  edge_create allocates the engine's arrays,
 * edge_destroy releases what is not memory (events, capture stream, graph execs); the loads take the packed rows of
 * d->n_frames frames; edge_erase and edge_known rewrite rows of d_llr in place.  Hidden: calls between two units of one library, no dynamic symbols.
 */
#pragma GCC visibility push(hidden)
bool edge_supports(const qldpc_decoder_cfg *cfg, const qldpc_code *code);      /* flooding, MS / OMS / NMS / SPA, degrees its kernels hold */
int edge_max_dv(void);                                                         /* the largest VN degree among them (the refusal names it) */
int edge_create(qldpc_decoder *d, const qldpc_code *code);
void edge_destroy(qldpc_decoder *d);
int edge_load_llr(qldpc_decoder *d, const float *d_llr);
int edge_load_bits(qldpc_decoder *d, const uint32_t *d_bits, const float *d_llr_mag, const uint8_t *d_vn_class, const int *d_n_channel);
int edge_load_syndrome(qldpc_decoder *d, const uint32_t *d_synd_bits);
int edge_erase(qldpc_decoder *d, const uint32_t *d_erase_bits);
int edge_known(qldpc_decoder *d);
int edge_run(qldpc_decoder *d);
int edge_fetch_packed(qldpc_decoder *d, uint32_t *d_out);
int edge_fetch_info(qldpc_decoder *d, int *d_V_K);
int edge_fetch_status(qldpc_decoder *d, int *d_iters, int *d_ok);
int edge_fetch_post(qldpc_decoder *d, float *d_post_out);
#pragma GCC visibility pop

/*
 * A gang of horizontal-layered decoders (qldpc.h "decoder gangs").  steps[s] = the kernel classes of colour step s, each with the members'
 * buckets that fall into it (in member order): one launch per class and QK_GANG_SLOTS live members.  Built once by qldpc_gang_create with the
 * planner qldpc_gang_plan uses (gang_plan_add); a run only filters by the members still taking part.
 */
struct gang_slot { int member, entry, n; };      /* entry: index into the member's d_gang */
struct gang_class { int cap, fam, cst; std::vector<gang_slot> slots; };
typedef std::vector<std::vector<gang_class>> gang_steps;
static inline void gang_plan_add(gang_steps &steps, int step, int cap, int fam, int cst, gang_slot s)
{
    if ((int)steps.size() <= step) steps.resize((size_t)step + 1);
    for (auto &c : steps[(size_t)step])
        if (c.cap == cap && c.fam == fam && c.cst == cst) { c.slots.push_back(s); return; }
    steps[(size_t)step].push_back(gang_class{cap, fam, cst, {s}});
}
struct qldpc_gang {
    std::vector<qldpc_decoder *> m;
    gang_steps steps;
    std::vector<int> buckets;        /* per member: layer launches of a sweep on its own */
    int device;
    hipStream_t stream;
    long long stats[4];
};
/* one class of one colour step for up to QK_GANG_SLOTS members (qldpc_launch_gang.hip) */
int qldpc_launch_layer_gang(hipStream_t stream, int cap, int fam, int cst, const qk_gang_args &a, unsigned grid);

/* kernel-launch dispatchers (qldpc_launch.hip); `first`: the check pass of iteration 0 in coded-LLR mode */
template <int V> void qldpc_launch_cn(qldpc_decoder *d, const bucket &b, bool first);
template <int V> void qldpc_launch_layer(qldpc_decoder *d, const bucket &b);
template <int V> void qldpc_launch_vlayer(qldpc_decoder *d, const bucket &b);
void qldpc_launch_layer_chain(qldpc_decoder *d, int sweep);      /* V = 1 only */
/* posterior form of the flooding run (V = 1 only): the check pass of iteration `ite` over one bucket, and the closing pass over the chain VNs */
void qldpc_launch_cn_fpost(qldpc_decoder *d, const bucket &b, int ite);
void qldpc_launch_fpost_close(qldpc_decoder *d, float *post_out);
/* the posterior pass between two iterations over fp_vn_classes (qk_vn_fpost: QK_FPV_CLASSES degree classes per launch) */
void qldpc_launch_vn_fpost(qldpc_decoder *d);
int qldpc_chain_resident_blocks(qldpc_decoder *d);
template <int V, int MODE> void qldpc_launch_vn(qldpc_decoder *d, const bucket &b, float *post_out);
#define QLDPC_DECLARE_LAUNCH(V)                                                                   \
    extern template void qldpc_launch_cn<V>(qldpc_decoder *, const bucket &, bool);                \
    extern template void qldpc_launch_layer<V>(qldpc_decoder *, const bucket &);                   \
    extern template void qldpc_launch_vlayer<V>(qldpc_decoder *, const bucket &);                  \
    extern template void qldpc_launch_vn<V, QK_VN_FIRST>(qldpc_decoder *, const bucket &, float *); \
    extern template void qldpc_launch_vn<V, QK_VN_NORMAL>(qldpc_decoder *, const bucket &, float *); \
    extern template void qldpc_launch_vn<V, QK_VN_POST>(qldpc_decoder *, const bucket &, float *);

#endif /* QLDPC_ENGINE_INT_H */
