/*
 * qldpc_recon.hip -- reconciliation sessions: the engine behind an ecd2 LDPC packet handler.
 *
 * Fills what the reference left as `return 81` (subcomponents/qber_estim.c:337-340,420-423): between
 * QBER estimation and privAmp_sendPrivAmpMsgAndPrivAmp (subcomponents/priv_amp.c:38) one parity
 * message replaces the cascade_biconf exchange (subcomponents/cascade_biconf.c:427-940).  Rate choice
 * follows the harness (BS/src/main.cpp:29,235-266: highest rate <= min_cr(QBER, f)); frame formation
 * follows BS/src/main.cpp:348-362 (channel bits +-ln((1-p)/p), disclosed bits +-23.03).
 * Host logic only; the arithmetic is the batched HIP decoder / encoder behind the same C ABI.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <list>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "../../include/qldpc.h"
#include "qldpc_graph.h"
#include "qldpc_hip.h"
#include "qldpc_devmem.h"
#include "qldpc_recon_core.h"

/*
 * One of the two staging sets of an entry: while batch i decodes, batch i + 1 is copied into the other set's pinned block, sent to
 * the device and assembled into frames on the lane's copy stream, and batch i - 1's results travel back.
 */
struct stage_set {
    uint32_t *h_in, *d_in;     /* the input block, pinned and on the device: recon_in_layout (qldpc_recon_core.h) */
    uint32_t *h_res, *d_res;   /* the result block: recon_bob_layout / recon_alice_layout */
    uint32_t *d_bits;          /* [max_blocks][Wn]  assembled frames */
    uint32_t *d_erase;         /* [max_blocks][Wn]  per-frame puncturing masks */
    hipEvent_t ev_in, ev_out, ev_done;
};

struct recon_entry {
    int K, M;
    qldpc_code *code;
    qldpc_encoder *enc;
    qldpc_decoder *dec;
    uint8_t *d_cls;       /* [N]: key VNs channel, parity VNs pinned */
    uint32_t *d_out;      /* [max_blocks][Wn] decoded words / Alice's codewords */
    int *d_iters, *d_ok;  /* [max_blocks] */
    stage_set set[2];
    int next_set;
    uint32_t *d_blind;    /* blind rounds (allocated by the first one): known | value | candidate | weakest rows, [4][max_blocks][Wn] */
    qldpc_qber *qest;     /* qldpc_recon_estimate_blocks: the entry's estimator (with the entry when the session preloads, else at the first such call) */
    qldpc_qber *qest_m;   /* qldpc_recon_estimate_blocks_merged: a second one with merging on (qldpc_qber_set_merge) */
    uint32_t *d_gpool;    /* guessing rounds (allocated by the first guessing call): the sources of a call, gpool_cap of them (recon_guess_pool_layout), then their results (recon_bob_layout | guess ints) */
    int gpool_cap;
    uint32_t *d_gtrial;   /* ... and the frames of a trial launch: known | value | bits | erase rows [4][max_blocks][Wn], then |LLR| | key_bits | pass | CRC [4][max_blocks] */
    uint32_t *d_est;      /* their outputs: counts [max_blocks][rows][2] | QBER [max_blocks], sized for the merged rows */
    dm_ledger mem;        /* the entry's own arrays, its staging sets and the lazy blind, guess and estimator buffers (qldpc_devmem.h): touched by the lane that runs the entry */
};

/* a lane = one host worker with a compute stream and a copy stream: the rate groups of a call run side by side, one lane each */
#define RECON_LANES 4
struct recon_lane {
    hipStream_t stream, copy;
};

struct qldpc_recon {
    qldpc_recon_cfg cfg;
    float gap;
    std::list<recon_entry> cache;   /* most recently used first */
    size_t keep;                    /* entries the cache may hold (all mother codes when they are preloaded) */
    long created;                   /* entries built so far (tests: nothing is built after a preload) */
    recon_lane lane[RECON_LANES];
    int profiling;
    uint32_t *h_tag, *d_tag;        /* qldpc_recon_tag_blocks: the staging block of a launch (recon_tag_layout), pinned and on the device: with the session when it preloads, else at the first such call */
    size_t tag_words;               /* ... and the words each holds */
    dm_ledger tag_mem;              /* ... and their ledger (qldpc_devmem.h): the calling thread's, never a lane's */
    int gang;                       /* QLDPC_RECON_GANG=1 when the session was made: Bob-side calls with several layered rate groups decode in rounds, one gang run each (run_call_gang) */
};

static const uint32_t *crc_table()
{
    /* built once behind the compiler's guard of a function-local static: the lanes' host workers may get here together */
    struct table {
        uint32_t t[256];
        table() { for (uint32_t i = 0; i < 256; i++) t[i] = crc_table_entry(i); }
    };
    static const table tab;
    return tab.t;
}

/* CRC-32 (IEEE 802.3) over the key bits, fed MSB-first word by word, bits past n_bits masked to 0 */
extern "C" uint32_t qldpc_crc32_words(const uint32_t *w, int n_bits) { return crc_serial(w, n_bits, crc_table()); }

/* host mirror of the device verification (rk_verify / rk_crc): `lanes` chunks folded in a tree; equals qldpc_crc32_words */
extern "C" uint32_t qldpc_crc32_words_chunked(const uint32_t *w, int n_bits, int lanes)
{
    if (!w || n_bits <= 0 || lanes < 1 || (lanes & (lanes - 1))) return 0;
    std::vector<uint32_t> reg((size_t)lanes);
    return crc_chunked(w, n_bits, lanes, crc_table(), reg.data());
}

/* one workgroup of 256 lanes per block: CRC-32 of words[0 .. ceil(n_bits / 32)) (tail bits masked) by the chunked fold; with `old` also
 * the number of key bits in which words differs from old, and with `copy_to` the masked words are written out.  Every lane returns the CRC. */
#define RK_LANES 256
__device__ static uint32_t rk_block_crc(const uint32_t *__restrict__ words, int n_bits, const uint32_t *__restrict__ old, uint32_t *__restrict__ copy_to,
                                        int *flips_out, uint32_t *s_tab, uint32_t *s_reg, int *s_cnt)
{
    const int t = (int)threadIdx.x;
    s_tab[t] = crc_table_entry((uint32_t)t);
    __syncthreads();
    const int nw = (n_bits + 31) / 32;
    int pad;
    const int c = crc_chunk_words(nw, RK_LANES, &pad);
    uint32_t reg = 0;
    int flips = 0;
    for (int v = t * c; v < (t + 1) * c; v++) {
        const int i = v - pad;
        if (i < 0) continue;
        const uint32_t m = tail_mask(i, nw, n_bits);
        const uint32_t x = words[i] & m;
        reg = crc_word_step(reg, x, s_tab);
        if (old) flips += __popc((old[i] & m) ^ x);
        if (copy_to) copy_to[i] = x;
    }
    s_reg[t] = reg;
    s_cnt[t] = flips;
    __syncthreads();
    uint32_t X = gf_xpow(32ull * (unsigned long long)c);
    for (int s = 1; s < RK_LANES; s <<= 1) {
        if ((t & (2 * s - 1)) == 0) {
            s_reg[t] = gf_mulmod(s_reg[t], X) ^ s_reg[t + s];
            s_cnt[t] += s_cnt[t + s];
        }
        X = gf_mulmod(X, X);
        __syncthreads();
    }
    if (flips_out) *flips_out = s_cnt[0];
    return crc_close(s_reg[0], nw);
}

/*
 * Bob, after the decode: verification on the device.  Per block: CRC-32 of the decoded key bits against Alice's, the number of bits the
 * decode flipped, and the verified key words (tail masked) in a compact [n][Wk] array -- the host receives {status, flips,
 * iterations, crc} and the words, and touches nothing per bit.  A block that failed gets its ORIGINAL words back (key untouched).
 */
__global__ __launch_bounds__(RK_LANES) void rk_verify(const uint32_t *__restrict__ out, const uint32_t *__restrict__ key, const int *__restrict__ key_bits,
                                                      const uint32_t *__restrict__ crc_want, const int *__restrict__ ok, const int *__restrict__ iters,
                                                      uint32_t *__restrict__ res_keys, int *__restrict__ res, int n, int Wk, int Wn)
{
    __shared__ uint32_t s_tab[256], s_reg[RK_LANES];
    __shared__ int s_cnt[RK_LANES];
    const int b = (int)blockIdx.x;
    const int kb = key_bits[b], nw = (kb + 31) / 32;
    int flips = 0;
    const uint32_t crc = rk_block_crc(out + (size_t)b * Wn, kb, key + (size_t)b * Wk, res_keys + (size_t)b * Wk, &flips, s_tab, s_reg, s_cnt);
    const bool good = ok[b] && crc == crc_want[b];
    if (!good)      /* uniform per workgroup */
        for (int i = (int)threadIdx.x; i < nw; i += RK_LANES) res_keys[(size_t)b * Wk + i] = key[(size_t)b * Wk + i];
    if (threadIdx.x == 0) {
        res[b] = good ? QLDPC_OK : QLDPC_EDECODE;
        res[n + b] = good ? flips : 0;
        res[2 * n + b] = iters[b];
        res[3 * n + b] = (int)crc;
    }
}

/* Alice: CRC-32 of every key as it lies on the device (information words [n][Wk]) */
__global__ __launch_bounds__(RK_LANES) void rk_crc(const uint32_t *__restrict__ key, const int *__restrict__ key_bits, uint32_t *__restrict__ crc_out, int Wk)
{
    __shared__ uint32_t s_tab[256], s_reg[RK_LANES];
    __shared__ int s_cnt[RK_LANES];
    const int b = (int)blockIdx.x;
    const uint32_t crc = rk_block_crc(key + (size_t)b * Wk, key_bits[b], nullptr, nullptr, nullptr, s_tab, s_reg, s_cnt);
    if (threadIdx.x == 0) crc_out[b] = crc;
}

#include "qldpc_kernels_recon_guess.h"
#include "qldpc_kernels_recon_tag.h"

extern "C" void qldpc_recon_cfg_default(qldpc_recon_cfg *c)
{
    if (!c) return;
    memset(c, 0, sizeof(*c));
    c->device = 0;
    c->efficiency = 1.4f;
    c->n_rates = 4;
    c->rates[0] = 0.5f; c->rates[1] = 0.7f; c->rates[2] = 0.8f; c->rates[3] = 0.9f;
    c->n_ite = 60;
    c->rule = QLDPC_RULE_SPA;       /* the harness default (BS/src/main.cpp:193); punctured VNs need it: measured FER 0 where NMS fails */
    c->rule_param = 0.0f;
    c->key_quantum = 1024;
    c->max_blocks = 1;
    c->seed = 7;
    c->schedule = QLDPC_RECON_SCHED_AUTO;
    c->mother_step = 8192;
    c->mother_max = 65536;
    c->rate_gap = 0.0f;             /* 0 = by rule: 0.035 for SPA / LSPA, 0.05 for the min-sum family (qldpc_recon_create) */
    c->puncture = 1;
    c->preload = 0;
    c->gap_profile = 0;
    c->peg_depth = 2;               /* mother codes by progressive edge growth, no 4-cycles */
}

/* Bob: frame words + puncturing mask of every block from its key words and the disclosed parity bits */
__global__ __launch_bounds__(256) void rk_assemble(const uint32_t *__restrict__ key, const uint32_t *__restrict__ disc, const int *__restrict__ key_bits,
                                                   const int *__restrict__ n_punct, uint32_t *__restrict__ bits, uint32_t *__restrict__ erase,
                                                   int Wk, int Wn, int Wm, int M)
{
    const int b = blockIdx.y;
    const int kb = key_bits[b], p = n_punct[b];
    for (int w = blockIdx.x * blockDim.x + threadIdx.x; w < Wn; w += gridDim.x * blockDim.x) {
        uint32_t word = 0, er = 0;
        if (w < Wk) {
            const int lo = w * 32;
            if (lo < kb) {
                word = key[(size_t)b * Wk + w];
                if (kb - lo < 32) word &= 0xFFFFFFFFu << (32 - (kb - lo));      /* shortened positions are known zeros */
            }
        } else {
            const uint32_t *dw = disc + (size_t)b * Wm;
            for (int t = 0; t < 32; t++) {
                const int j = (w - Wk) * 32 + t;
                if (j >= M) break;
                if (punct_at(j, p, M)) er |= 1u << (31 - t);
                else {
                    const int r = punct_rank(j, p, M);
                    word |= ((dw[r >> 5] >> (31 - (r & 31))) & 1u) << (31 - t);
                }
            }
        }
        bits[(size_t)b * Wn + w] = word;
        erase[(size_t)b * Wn + w] = er;
    }
}

/* Alice: the disclosed (non-punctured) parity bits of every codeword, packed in position order */
__global__ __launch_bounds__(256) void rk_disclose(const uint32_t *__restrict__ cw, const int *__restrict__ n_punct, uint32_t *__restrict__ disc,
                                                   int Wk, int Wn, int Wm, int M)
{
    const int b = blockIdx.y;
    const int p = n_punct[b], d = M - p;
    const uint32_t *par = cw + (size_t)b * Wn + Wk;
    for (int w = blockIdx.x * blockDim.x + threadIdx.x; w < Wm; w += gridDim.x * blockDim.x) {
        uint32_t word = 0;
        for (int t = 0; t < 32; t++) {
            const int r = w * 32 + t;
            if (r >= d) break;
            const int j = punct_position(r, p, M);
            word |= ((par[j >> 5] >> (31 - (j & 31))) & 1u) << (31 - t);
        }
        disc[(size_t)b * Wm + w] = word;
    }
}

static void entry_free(recon_entry &e)
{
    qldpc_qber_free(e.qest);
    qldpc_qber_free(e.qest_m);
    qldpc_decoder_free(e.dec);
    qldpc_encoder_free(e.enc);
    qldpc_code_free(e.code);
    dm_free_all(&e.mem);
    for (auto &st : e.set) {
        if (st.ev_in) (void)hipEventDestroy(st.ev_in);
        if (st.ev_out) (void)hipEventDestroy(st.ev_out);
        if (st.ev_done) (void)hipEventDestroy(st.ev_done);
    }
}

extern "C" void qldpc_recon_free(qldpc_recon *r)
{
    if (!r) return;
    (void)hipSetDevice(r->cfg.device);
    for (auto &e : r->cache) entry_free(e);
    dm_free_all(&r->tag_mem);
    for (auto &l : r->lane) {
        if (l.stream) (void)hipStreamDestroy(l.stream);
        if (l.copy) (void)hipStreamDestroy(l.copy);
    }
    delete r;
}

/* code dimensions of a block of key_bits on table rate R: a mother code (K a multiple of mother_step, the block is shortened) up to
 * mother_max bits, otherwise a code of its own size (K = key_bits rounded up to key_quantum) */
static void code_dims(const qldpc_recon_cfg &c, int key_bits, double R, int *K, int *M)
{
    int k;
    if (c.mother_step > 0 && key_bits <= c.mother_max) k = (key_bits + c.mother_step - 1) / c.mother_step * c.mother_step;
    else k = (key_bits + c.key_quantum - 1) / c.key_quantum * c.key_quantum;
    int m = (int)llround((double)k * (1.0 - R) / R);
    if (m < 2) m = 2;
    *K = k; *M = m;
}

static int get_entry(qldpc_recon *r, int K, int M, recon_entry **out, qldpc_code *prebuilt = nullptr);
static int build_code(const qldpc_recon_cfg &cfg, int K, int M, qldpc_code **out);
static int tag_stage_reserve(qldpc_recon *r, size_t words);
static void cache_trim(qldpc_recon *r)
{
    if (r->cache.size() <= r->keep) return;
    (void)hipDeviceSynchronize();
    while (r->cache.size() > r->keep) { entry_free(r->cache.back()); r->cache.pop_back(); }
}
/* is this a session whose decoders run the horizontal-layered schedule?  Batches do unless told otherwise: half the iterations for the same bytes per
 * sweep (config-3 stream 16.1 -> 14.4 ms, 0 instead of 0 - 1 first-round failures per 2 048 epochs); a decoder for <= 8 blocks is the edge-parallel
 * engine, which is flooding */
static bool cfg_layered(const qldpc_recon_cfg &c) { return c.schedule == QLDPC_SCHED_HLAYERED || (c.schedule == QLDPC_RECON_SCHED_AUTO && c.max_blocks > 8); }

extern "C" int qldpc_recon_create(const qldpc_recon_cfg *cfg, qldpc_recon **out)
{
    if (!out) return QLDPC_EINVAL;
    *out = nullptr;
    if (!cfg) return QLDPC_EINVAL;
    if (cfg->n_rates < 1 || cfg->n_rates > 8 || cfg->key_quantum < 32 || (cfg->key_quantum & 31) || cfg->max_blocks < 1 || cfg->n_ite < 1 ||
        !(cfg->efficiency > 0.0f) || cfg->mother_step < 0 || (cfg->mother_step & 31) || (cfg->mother_step > 0 && cfg->mother_max < cfg->mother_step) ||
        !(cfg->rate_gap >= 0.0f && cfg->rate_gap < 0.5f) || cfg->peg_depth < 0 || cfg->peg_depth > 4 || cfg->gap_profile < 0 || cfg->gap_profile > 1 || cfg->schedule < 0 || cfg->schedule > QLDPC_RECON_SCHED_AUTO) {
        qldpc_set_error("recon_create: bad configuration");
        return QLDPC_EINVAL;
    }
    for (int i = 0; i < cfg->n_rates; i++)
        if (!(cfg->rates[i] > 0.0f && cfg->rates[i] < 1.0f) || (i && cfg->rates[i] <= cfg->rates[i - 1])) { qldpc_set_error("recon_create: rate table must be ascending in (0,1)"); return QLDPC_EINVAL; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { qldpc_set_error("no HIP device visible: libqldpc has no CPU fallback"); return QLDPC_ENODEV; }
    if (cfg->device < 0 || cfg->device >= ndev) { qldpc_set_error("device %d out of range", cfg->device); return QLDPC_ENODEV; }
    qldpc_recon *r = new (std::nothrow) qldpc_recon();
    if (!r) return QLDPC_ENOMEM;
    r->cfg = *cfg;
    r->gap = cfg->rate_gap > 0.0f ? cfg->rate_gap : (cfg->rule == QLDPC_RULE_SPA || cfg->rule == QLDPC_RULE_LSPA ? 0.035f : 0.05f);
    const size_t mothers = cfg->mother_step > 0 ? (size_t)(cfg->mother_max / cfg->mother_step) * (size_t)cfg->n_rates : 0;
    r->keep = mothers + 6;
    r->created = 0;
    r->profiling = 0;
    r->gang = 0;
    r->h_tag = r->d_tag = nullptr; r->tag_words = 0;
    if (const char *env = getenv("QLDPC_RECON_GANG")) r->gang = atoi(env) == 1;
    memset(r->lane, 0, sizeof(r->lane));
    if (hipSetDevice(cfg->device) != hipSuccess) { delete r; return QLDPC_EHIP; }
    /* the session's own streams: nothing of it runs on the null stream, so a second session or other work on the device does not
     * serialise behind it */
    /* the runtime binds a stream to one of its few hardware queues when the stream is created, round robin: the compute streams are
     * created back to back so that the lanes land on different queues (interleaved with the copy streams, four lanes shared two queues
     * and at most two kernels ever ran side by side: rocprofv3 kernel trace, profiles/r03_config3_*) */
    bool ok = true;
    for (auto &l : r->lane) ok = ok && hipStreamCreateWithFlags(&l.stream, hipStreamNonBlocking) == hipSuccess;
    for (auto &l : r->lane) ok = ok && hipStreamCreateWithFlags(&l.copy, hipStreamNonBlocking) == hipSuccess;
    if (!ok) {
        qldpc_set_error("recon_create: hipStreamCreate failed");
        qldpc_recon_free(r);
        return QLDPC_EHIP;
    }
    if (cfg->preload && mothers) {
        /* every (mother size, table rate) pair now: code, encoder, decoder and staging buffers, so that no block of up to mother_max
         * bits builds a code or allocates device memory later (the daemon calls this from ldpc_init) */
        struct todo { int K, M; qldpc_code *code; int rc; std::string err; };
        std::vector<todo> list;
        for (int k = cfg->mother_step; k <= cfg->mother_max; k += cfg->mother_step)
            for (int i = 0; i < cfg->n_rates; i++) {
                todo t;
                code_dims(r->cfg, k, cfg->rates[i], &t.K, &t.M);
                t.code = nullptr; t.rc = QLDPC_OK;
                list.push_back(t);
            }
        /* the codes are host work (progressive edge growth: 0.1 - 10 s each unless QLDPC_CODE_CACHE holds them): built side by side on
         * the host's cores, largest first; the device objects follow one by one */
        std::vector<size_t> order(list.size());
        for (size_t i = 0; i < order.size(); i++) order[i] = i;
        std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return (double)list[a].K / list[a].M * list[a].K > (double)list[b].K / list[b].M * list[b].K; });
        std::atomic<size_t> next(0);
        auto worker = [&]() {
            for (size_t at = next++; at < order.size(); at = next++) {
                todo &t = list[order[at]];
                t.rc = build_code(r->cfg, t.K, t.M, &t.code);
                if (t.rc) t.err = qldpc_last_error();
            }
        };
        unsigned nthreads = std::thread::hardware_concurrency();
        if (const char *env = getenv("QLDPC_BUILD_THREADS")) nthreads = (unsigned)atoi(env);
        nthreads = std::max(1u, std::min(nthreads, std::min(16u, (unsigned)list.size())));
        if (cfg->peg_depth <= 0) nthreads = 1;      /* the seeded shuffle takes milliseconds */
        std::vector<std::thread> th;
        for (unsigned t = 1; t < nthreads; t++) th.emplace_back(worker);
        worker();
        for (auto &t : th) t.join();
        int rc = QLDPC_OK;
        for (auto &t : list) if (t.rc && !rc) { rc = t.rc; qldpc_set_error("%s", t.err.c_str()); }
        for (auto &t : list) {
            if (rc) { qldpc_code_free(t.code); continue; }
            recon_entry *e;
            rc = get_entry(r, t.K, t.M, &e, t.code);      /* takes the code over (also on failure: entry_free) */
        }
        /* ... and the staging of qldpc_recon_tag_blocks for launches of max_blocks keys of up to mother_max bits under RT_MAX_KEYS keys */
        if (!rc) rc = tag_stage_reserve(r, recon_tag_layout(nullptr, cfg->max_blocks, cfg->mother_max / 32, RT_MAX_KEYS).words);
        if (rc) { qldpc_recon_free(r); return rc; }
    }
    *out = r;
    return QLDPC_OK;
}

extern "C" long qldpc_recon_entries_created(const qldpc_recon *r) { return r ? r->created : -1; }

/* per-kernel profile of Bob's decoders (qldpc_profile_*), summed over the codes of the session */
extern "C" int qldpc_recon_profile_enable(qldpc_recon *r, int on)
{
    if (!r) return QLDPC_EINVAL;
    r->profiling = on;
    for (auto &e : r->cache) { qldpc_profile_enable(e.dec, on); if (on) qldpc_profile_clear(e.dec); }
    return QLDPC_OK;
}
extern "C" int qldpc_recon_profile_read(qldpc_recon *r, qldpc_kernel_stat *out, int cap)
{
    if (!r || (!out && cap > 0)) return QLDPC_EINVAL;
    int n = 0;
    for (auto &e : r->cache) {
        qldpc_kernel_stat st[16];
        const int m = qldpc_profile_read(e.dec, st, 16);
        if (m < 0) return m;
        for (int i = 0; i < m; i++) {
            int k = 0;
            while (k < n && strcmp(out[k].name, st[i].name)) k++;
            if (k == n) { if (n >= cap) continue; out[n] = st[i]; n++; continue; }
            out[k].launches += st[i].launches; out[k].total_ms += st[i].total_ms; out[k].alg_bytes += st[i].alg_bytes; out[k].moved_bytes += st[i].moved_bytes;
        }
    }
    return n;
}

/*
 * Rate choice, code dimensions and puncturing of a block (BS/src/main.cpp:29-34,235-311).  The QBER estimate is clamped to
 * [0.001, 0.25] first: the daemon's localError is exactly 0 when the test sample held no error (qber_estim.c:26).
 *   target rate  R* = min( 1 / (1 + f h(q)),  1 - h(q) - rate_gap (65536 / K)^0.4 c(R) )   the harness's min_cr, kept away from capacity;
 *                c(R) = 0.6 for mother rates <= 0.75, 0.9 up to 0.85, 1 above
 *   table rate   R  = largest entry <= R*                                  (BS/src/main.cpp:241-266)
 *   code         K >= key_bits information VNs (mother code, shortened), M = round(K (1 - R) / R) parity VNs
 *   disclosed    d = ceil(key_bits (1 / R* - 1)) parity bits, the other p = M - d are punctured (parity_bits_to_punct with the block's
 *                own length for the information bits), at most 65 % of M
 * leak = d + 32 (CRC).
 */
#define RECON_PUNCT_CAP 0.65
static float clamp_qber(float q) { return !(q > 0.001f) ? 0.001f : (q > 0.25f ? 0.25f : q); }

/*
 * c(R): how much of rate_gap a mother code of rate R needs.  Calibrated on streams of 2 048 epochs x 52 429 bits, QBER ~ U[0.5 %, 6 %], two
 * seeds each (qldpc_stream -e 2048 -P <depth>, QLDPC_RECON_GAP_SCALE; logs: profiles/r03_gap_calibration.txt):
 *   PEG-built mothers (peg_depth > 0)   0.10 (mothers of K >= 32 768; more below) / 0.85 / 1.0   for R <= 0.75 / <= 0.85 / above: 0 - 1 first-round failures in 2 048 epochs, leak 0.2896 of
 *                                       the key (the configured efficiency f = 1.4 alone gives 0.288); the low-rate mothers decode to within
 *                                       0.004 of capacity, the rate-0.8 / 0.9 mothers need their 0.03 (0.025: 2 - 4 % failures)
 *   seeded-shuffle mothers (round 2)    0.60 / 0.90 / 1.0   (0.85 for the middle value: 39 failures of 918 on one seed where PEG has none)
 * QLDPC_RECON_GAP_SCALE="lo,mid,hi" overrides the three values for calibration runs -- both sides must then use the same.
 */
static double gap_scale(const qldpc_recon_cfg &cfg, double R, int K)
{
    struct from_env {      /* read once, behind the guard of a function-local static (sessions may plan on several threads) */
        double v[3] = {-1.0, -1.0, -1.0};
        from_env() { if (const char *e = getenv("QLDPC_RECON_GAP_SCALE")) (void)sscanf(e, "%lf,%lf,%lf", &v[0], &v[1], &v[2]); }
    };
    static const from_env env_scale;
    const double *env = env_scale.v;
    const int k = R <= 0.75 ? 0 : (R <= 0.85 ? 1 : 2);
    if (env[0] >= 0.0 && env[k] >= 0.0) return env[k];
    static const double peg[3] = {0.10, 0.85, 1.0}, shuffle[3] = {0.60, 0.90, 1.0};
    if (cfg.peg_depth <= 0 || cfg.gap_profile == 1) return shuffle[k];
    /* short low-rate mothers need more room: 0.1 from K = 32 768 upwards, 0.25 at 16 384, 0.6 at 8 192 (7 000-bit blocks: 24 failures of
     * 1 203 at rate 0.7 with 0.1 - 0.3, 1 with 0.6; 15 000-bit blocks: 1 - 2 of 1 100 at any value) */
    if (k == 0) return std::min(0.6, std::max(0.10, 0.10 * pow(32768.0 / (double)K, 1.3)));
    return peg[k];
}

extern "C" int qldpc_recon_plan(const qldpc_recon *r, int key_bits, float qber, qldpc_recon_msg *msg)
{
    if (!r || !msg) return QLDPC_EINVAL;
    if (key_bits < 32) { qldpc_set_error("recon_plan: key_bits=%d", key_bits); return QLDPC_ESIZE; }
    if (!(qber >= 0.0f && qber < 0.5f)) { qldpc_set_error("recon_plan: qber=%g not in [0, 0.5)", (double)qber); return QLDPC_EINVAL; }
    const float q = clamp_qber(qber);
    const double h = qldpc_binary_entropy(q);
    /* the distance a code needs from capacity grows as it gets shorter: measured clean (FER 0 / 128 per point, QBER 0.3 .. 8 %, SPA) at
     * 0.035 for K = 65 536, 0.042 for 32 768, 0.06 for 16 384 and 8 192 (tools/punct_probe.py) -- rate_gap (65536 / K)^0.4 covers them */
    int K0, M0;
    code_dims(r->cfg, key_bits, 0.5, &K0, &M0);
    const double gap_len = (double)r->gap * pow(65536.0 / (double)K0, 0.4);
    /* ... and with the rate of the mother code: the low-rate mothers decode punctured to within 0.02 of capacity (FER 0 / 128 at 0.015 -
     * 0.02 for rates 0.5 and 0.7), rate 0.8 needs 0.03 and rate 0.9 0.035 (tools/punct_probe.py, gpurun logs punct_c / punct_e): the
     * table entry is the highest rate that fits under ITS OWN target */
    int idx = -1;
    double need = 0.0;
    for (int i = 0; i < r->cfg.n_rates; i++) {
        const double R = r->cfg.rates[i];
        const double gap = gap_len * gap_scale(r->cfg, R, K0);
        double t = qldpc_min_code_rate(q, r->cfg.efficiency);
        if (1.0 - h - gap < t) t = 1.0 - h - gap;
        if (R <= t) { idx = i; need = t; }
    }
    if (idx < 0) { qldpc_set_error("recon_plan: QBER %.4f is above what the rate table covers", (double)qber); return QLDPC_EUNSUPPORTED; }
    int K, M;
    code_dims(r->cfg, key_bits, r->cfg.rates[idx], &K, &M);
    int p = 0;
    if (r->cfg.puncture == 1) {
        const int d = (int)ceil((double)key_bits * (1.0 / need - 1.0));
        p = M - d;
        if (p > (int)(RECON_PUNCT_CAP * M)) p = (int)(RECON_PUNCT_CAP * M);
        if (p < 0) p = 0;
    }
    memset(msg, 0, sizeof(*msg));
    msg->rate_index = (uint32_t)idx;
    msg->key_bits = (uint32_t)key_bits;
    msg->code_k = (uint32_t)K;
    msg->code_m = (uint32_t)M;
    msg->n_punct = (uint32_t)p;
    return QLDPC_OK;
}

/* the code of an entry: DVB-like IRA profile (12.5 % of the information VNs of degree 11, the rest 3), information part by the seeded socket
 * shuffle or by progressive edge growth (peg_depth); both sides derive the same code from (K, M, peg_depth, seed) */
static int build_code(const qldpc_recon_cfg &cfg, int K, int M, qldpc_code **out)
{
    const int N = K + M;
    return cfg.peg_depth > 0 ? qldpc_code_ira_peg(N, K, 0.125f, 11, 3, cfg.peg_depth, cfg.seed, out) : qldpc_code_ira(N, K, 0.125f, 11, 3, cfg.seed, out);
}

/* an estimator of an entry, plain or merged, and the output rows the two share (qldpc_recon_estimate_blocks, _merged) */
static int entry_estimator(const qldpc_recon *r, recon_entry &e, bool merge)
{
    qldpc_qber *&est = merge ? e.qest_m : e.qest;
    if (est) return QLDPC_OK;
    qldpc_qber_cfg qc;
    qldpc_qber_cfg_default(&qc);
    qc.device = r->cfg.device; qc.max_frames = r->cfg.max_blocks;
    int rc = qldpc_qber_create(e.code, &qc, &est);
    if (!rc && merge && (rc = qldpc_qber_set_merge(est, 1))) { qldpc_qber_free(est); est = nullptr; }
    if (rc) return rc;
    const size_t bins = 2 * (size_t)(QLDPC_QBER_MAX_DEGREE + 1);
    if (!e.d_est && dm_alloc(&e.mem, &e.d_est, (size_t)r->cfg.max_blocks * (bins + 1))) {
        qldpc_qber_free(est); est = nullptr;
        qldpc_set_error("recon: device allocation for the QBER estimator failed");
        return QLDPC_ENOMEM;
    }
    return QLDPC_OK;
}

static int get_entry(qldpc_recon *r, int K, int M, recon_entry **out, qldpc_code *prebuilt)
{
    for (auto it = r->cache.begin(); it != r->cache.end(); ++it)
        if (it->K == K && it->M == M) { r->cache.splice(r->cache.begin(), r->cache, it); *out = &r->cache.front(); return QLDPC_OK; }
    recon_entry e{};
    e.K = K; e.M = M;
    const int N = K + M, Wk = K / 32, Wn = (N + 31) / 32, Wm = (M + 31) / 32, B = r->cfg.max_blocks;
    int rc = QLDPC_OK;
    if (prebuilt) e.code = prebuilt;
    else rc = build_code(r->cfg, K, M, &e.code);
    if (!rc) rc = qldpc_encoder_create(e.code, "IRA", r->cfg.device, &e.enc);
    if (!rc) rc = qldpc_encoder_reserve(e.enc, B);      /* nothing is allocated per block later */
    if (!rc) {
        qldpc_decoder_cfg dc;
        qldpc_decoder_cfg_default(&dc);
        dc.schedule = cfg_layered(r->cfg) ? QLDPC_SCHED_HLAYERED : QLDPC_SCHED_FLOODING; dc.rule = r->cfg.rule; dc.rule_param = r->cfg.rule_param; dc.n_ite = r->cfg.n_ite;
        dc.enable_syndrome = 1; dc.syndrome_depth = 1; dc.max_frames = B; dc.device = r->cfg.device;
        dc.layer_chain = 2;      /* the session's decoders run side by side (lanes): persistent one-launch sweeps would fight for the chip (measured 19.0 -> 23.9 ms) */
        rc = qldpc_decoder_create(e.code, K, nullptr, &dc, &e.dec);
        if (!rc) rc = qldpc_decoder_reserve(e.dec);      /* nothing is allocated per block later */
    }
    if (!rc) rc = dm_alloc(&e.mem, &e.d_cls, (size_t)N);
    if (!rc) rc = dm_alloc(&e.mem, &e.d_out, (size_t)B * Wn);
    if (!rc) rc = dm_alloc(&e.mem, &e.d_iters, (size_t)B);
    if (!rc) rc = dm_alloc(&e.mem, &e.d_ok, (size_t)B);
    /* a full job's staging blocks; an entry serves both sides, so the result block holds the larger of the two layouts */
    /* a tagged call appends the hash-key rows of its blocks to the input block and receives their tags behind the result block: room for RT_MAX_KEYS keys a block */
    const size_t tag_room = (size_t)B * 2 * RT_MAX_KEYS;
    const size_t in_words = recon_in_layout(nullptr, B, Wk, Wm).words + tag_room;
    const size_t res_words = std::max(recon_bob_layout(nullptr, B, Wk).words, recon_alice_layout(nullptr, B, Wm).words) + tag_room;
    for (auto &st : e.set) {
        if (!rc) rc = dm_alloc(&e.mem, &st.d_in, in_words);
        if (!rc) rc = dm_alloc(&e.mem, &st.d_res, res_words);
        if (!rc) rc = dm_alloc(&e.mem, &st.d_bits, (size_t)B * Wn);
        if (!rc) rc = dm_alloc(&e.mem, &st.d_erase, (size_t)B * Wn);
        if (!rc) rc = dm_alloc_pinned(&e.mem, &st.h_in, in_words);
        if (!rc) rc = dm_alloc_pinned(&e.mem, &st.h_res, res_words);
        if (!rc && (hipEventCreateWithFlags(&st.ev_in, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&st.ev_out, hipEventDisableTiming) != hipSuccess ||
                    hipEventCreateWithFlags(&st.ev_done, hipEventDisableTiming) != hipSuccess)) rc = QLDPC_EHIP;
    }
    if (!rc) {
        std::vector<uint8_t> cls((size_t)N, (uint8_t)QLDPC_VN_PINNED);       /* parity VNs are disclosed; key VNs past a block's length are pinned per frame */
        for (int i = 0; i < K; i++) cls[(size_t)i] = (uint8_t)QLDPC_VN_CHANNEL;
        if (hipMemcpy(e.d_cls, cls.data(), (size_t)N, hipMemcpyHostToDevice) != hipSuccess) rc = QLDPC_EHIP;
    }
    if (!rc && r->cfg.preload) rc = entry_estimator(r, e, false);      /* nothing is allocated per block later */
    if (!rc && r->cfg.preload) rc = entry_estimator(r, e, true);
    if (rc) { entry_free(e); return rc; }
    if (r->profiling) qldpc_profile_enable(e.dec, 1);
    r->cache.push_front(std::move(e));      /* the cache is trimmed to `keep` entries at the end of the call (cache_trim): nothing in use is evicted */
    r->created++;
    *out = &r->cache.front();
    return QLDPC_OK;
}

/* a message header must describe the block it came with AND be what the local plan gives for its rate index: the peer cannot make
 * this side build a code of its own choosing */
static int check_msg(const qldpc_recon *r, const qldpc_recon_msg *m, int key_bits)
{
    int K = 0, M = 0;
    const bool idx_ok = m->rate_index < (uint32_t)r->cfg.n_rates;
    if (idx_ok && key_bits >= 32) code_dims(r->cfg, key_bits, r->cfg.rates[m->rate_index], &K, &M);
    if (!idx_ok || key_bits < 32 || (int)m->key_bits != key_bits || (int)m->code_k != K || (int)m->code_m != M || m->n_punct > (uint32_t)(RECON_PUNCT_CAP * M) ||
        (r->cfg.puncture != 1 && m->n_punct != 0)) {
        qldpc_set_error("recon: message header does not match the block (key_bits %u vs %d, rate index %u, K %u vs %d, M %u vs %d, punctured %u)",
                        m->key_bits, key_bits, m->rate_index, m->code_k, K, m->code_m, M, m->n_punct);
        return QLDPC_ESIZE;
    }
    return QLDPC_OK;
}

/* QLDPC_OK if the header is what this side's plan gives for its rate index and the block's length (what the decode calls check per
 * message): lets a packet handler refuse a header before it allocates for its payload */
extern "C" int qldpc_recon_check_header(const qldpc_recon *r, const qldpc_recon_msg *msg, int key_bits)
{
    if (!r || !msg) return QLDPC_EINVAL;
    return check_msg(r, msg, key_bits);
}

extern "C" int qldpc_recon_parity_words(const qldpc_recon_msg *msg) { return msg ? (int)((msg->code_m - msg->n_punct + 31) / 32) : QLDPC_EINVAL; }
extern "C" int qldpc_recon_leaked_bits(const qldpc_recon_msg *msg) { return msg ? (int)(msg->code_m - msg->n_punct) + 32 : QLDPC_EINVAL; }
/* the conservative account of a tagged block: the CRC and every key's tag are both charged; 0 on a bad argument */
extern "C" int qldpc_recon_leaked_bits_tagged(const qldpc_recon_msg *msg, int n_keys)
{
    return msg && n_keys >= 1 && n_keys <= RT_MAX_KEYS ? qldpc_recon_leaked_bits(msg) + RT_TAG_BITS * n_keys : 0;
}

/* ------------------------------------------------------------------ the pipeline ------------------------------------------------
 *
 * A call brings blocks of any mix of codes.  Blocks of one code (entry) form batches of up to max_blocks frames = jobs; the jobs of
 * one entry go to one lane (an entry has one decoder), the entries of a call are spread over up to RECON_LANES lanes, and every
 * lane is a host worker with its own compute and copy stream:
 *
 *     copy stream     H2D(j) assemble(j) | H2D(j+1) assemble(j+1) | D2H(j)            | H2D(j+2) ...
 *     compute stream                     | load(j) BP iterations(j) fetch verify(j)   | load(j+1) ...
 *     host            stage(j) stage(j+1)  ... polls the early-exit mailbox of j ...    results(j-1) stage(j+2)
 *
 * so the rate groups of a stream of epochs decode side by side (their launches fill each other's tails), and within a lane the
 * staging and the copies of the neighbouring batches hide behind the decode.  Nothing runs on the null stream.
 */
struct recon_job {
    recon_entry *e;
    std::vector<int> idx;       /* the job's blocks in the caller's arrays */
    stage_set *st;
    bool any_punct;
    std::vector<uint32_t> h_blind, h_weak;   /* blind rounds: the job's known | value | candidate rows on their way in, its weakest rows on their way back */
};

struct recon_call {
    bool bob;
    int n;
    const int *key_bits;
    /* Bob */
    uint32_t *const *key; const float *qber; const qldpc_recon_msg *msgs; const uint32_t *const *parity; int *status, *corrected, *iterations;
    qldpc_recon_blind *blind; int ask_bits;      /* != NULL: a blind round (qldpc_recon_decode_blind) */
    qldpc_recon_guess *guess; int guess_bits;    /* guess_bits > 0: a call with guessing rounds (qldpc_recon_decode_guess) */
    int n_keys; const uint32_t *const *hash_keys; uint32_t *const *tags; bool hash_shared;      /* n_keys > 0: a tagged call (qldpc_recon_decode_blocks_tagged, _decode_guess_tagged); hash_shared: one key row for all blocks */
    /* Alice */
    const uint32_t *const *akey; qldpc_recon_msg *amsgs; uint32_t *const *aparity;
};

/* guessing rounds: the blocks of an entry whose first decode failed, in pool order (slot k of the entry's pool holds block idx[k]) */
struct guess_sources {
    recon_entry *e;
    std::vector<int> idx;
    bool any_punct;
};

struct lane_run {
    qldpc_recon *r;
    recon_lane *lane;
    const recon_call *call;
    std::vector<recon_job> jobs;
    std::vector<guess_sources> guess;      /* one per entry of the lane that had a failure */
    int rc;
    std::string err;
};

static recon_call call_bob(int n, uint32_t *const *key, const int *key_bits, const float *qber, const qldpc_recon_msg *msgs, const uint32_t *const *parity,
                           int *status, int *corrected, int *iterations, qldpc_recon_blind *blind = nullptr, int ask_bits = 0)
{
    recon_call c = {};
    c.bob = true; c.n = n; c.key_bits = key_bits; c.key = key; c.qber = qber; c.msgs = msgs; c.parity = parity;
    c.status = status; c.corrected = corrected; c.iterations = iterations; c.blind = blind; c.ask_bits = ask_bits;
    return c;
}
static recon_call call_alice(int n, const uint32_t *const *key, const int *key_bits, qldpc_recon_msg *msgs, uint32_t *const *parity)
{
    recon_call c = {};
    c.bob = false; c.n = n; c.key_bits = key_bits; c.akey = key; c.amsgs = msgs; c.aparity = parity;
    return c;
}
static lane_run lane_of(qldpc_recon *r, int l, const recon_call &call)
{
    lane_run L;
    L.r = r; L.lane = &r->lane[l]; L.call = &call; L.rc = QLDPC_OK;
    return L;
}

/* the staging blocks of a job at `base` (a set's pinned or device block) */
static recon_in_view job_in(const recon_job &j, uint32_t *base) { return recon_in_layout(base, (int)j.idx.size(), j.e->K / 32, (j.e->M + 31) / 32); }
static recon_bob_view job_bob_res(const recon_job &j, uint32_t *base) { return recon_bob_layout(base, (int)j.idx.size(), j.e->K / 32); }
static recon_alice_view job_alice_res(const recon_job &j, uint32_t *base) { return recon_alice_layout(base, (int)j.idx.size(), (j.e->M + 31) / 32); }

static int job_stage(lane_run *L, recon_job &j, hipStream_t cs)
{
    recon_entry *e = j.e;
    const recon_call &c = *L->call;
    const int n = (int)j.idx.size(), K = e->K, M = e->M, N = K + M;
    const int Wk = K / 32, Wn = (N + 31) / 32, Wm = (M + 31) / 32;
    stage_set *st = &e->set[e->next_set];
    e->next_set ^= 1;
    j.st = st;
    j.any_punct = false;
    const recon_in_view h = job_in(j, st->h_in), d = job_in(j, st->d_in);
    for (int t = 0; t < n; t++) {
        const int i = j.idx[(size_t)t], kb = c.key_bits[i], Wkey = (kb + 31) / 32;
        uint32_t *f = h.keys + (size_t)t * Wk;
        if (c.bob) {
            /* only the words the kernels read are copied: rk_assemble masks the tail and never looks past the block's length */
            memcpy(f, c.key[i], sizeof(uint32_t) * (size_t)Wkey);
            h.n_punct[t] = (int)c.msgs[i].n_punct;
            memcpy(h.disc + (size_t)t * Wm, c.parity[i], sizeof(uint32_t) * (size_t)((M - h.n_punct[t] + 31) / 32));
            h.mag[t] = c.qber ? qldpc_bsc_llr(clamp_qber(c.qber[i])) : 0.0f;      /* no QBER yet: qldpc_recon_estimate_blocks */
            h.crc[t] = c.msgs[i].crc32;
        } else {
            /* information word of the mother code: the key, then zeros (shortened positions) */
            memcpy(f, c.akey[i], sizeof(uint32_t) * (size_t)Wkey);
            if (kb & 31) f[Wkey - 1] &= 0xFFFFFFFFu << (32 - (kb & 31));
            memset(f + Wkey, 0, sizeof(uint32_t) * (size_t)(Wk - Wkey));
            h.n_punct[t] = (int)c.amsgs[i].n_punct;
            h.mag[t] = 0.0f; h.crc[t] = 0;
        }
        h.key_bits[t] = kb;
        j.any_punct = j.any_punct || h.n_punct[t] != 0;
    }
    size_t in_words = h.words;
    if (c.bob && c.n_keys) {      /* the hash-key rows travel behind the block, in the same copy: one row when the blocks share it */
        const size_t row = 2 * (size_t)c.n_keys;
        for (int t = 0; t < (c.hash_shared ? 1 : n); t++) memcpy(st->h_in + h.words + (size_t)t * row, c.hash_keys[j.idx[(size_t)t]], sizeof(uint32_t) * row);
        in_words += (c.hash_shared ? 1 : (size_t)n) * row;
    }
    HIPCHK(hipMemcpyAsync(st->d_in, st->h_in, sizeof(uint32_t) * in_words, hipMemcpyHostToDevice, cs));
    if (c.bob) {
        hipLaunchKernelGGL(rk_assemble, dim3((unsigned)((Wn + 255) / 256), (unsigned)n), dim3(256), 0, cs, d.keys, d.disc, d.key_bits, d.n_punct, st->d_bits, st->d_erase, Wk, Wn, Wm, M);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(st->ev_in, cs));
    return QLDPC_OK;
}

/*
 * A blind round (qldpc_recon_decode_blind): the positions disclosed so far become known bits of the job's frames (qldpc_load_known_dev, after the
 * erasures: known wins), and the candidates of a later request are the key positions below the block's length that are not known yet.  The rows
 * travel on the compute stream from the job's own host vectors; a job without a known position loads nothing and decodes as in qldpc_recon_decode_blocks.
 */
static int job_load_blind(lane_run *L, recon_job &j)
{
    recon_entry *e = j.e;
    const recon_call &c = *L->call;
    hipStream_t s = L->lane->stream;
    const int n = (int)j.idx.size(), B = L->r->cfg.max_blocks;
    const size_t Wn = (size_t)(e->K + e->M + 31) / 32;
    if (!e->d_blind && dm_alloc(&e->mem, &e->d_blind, 4 * (size_t)B * Wn)) { qldpc_set_error("recon_decode_blind: device allocation failed"); return QLDPC_ENOMEM; }
    j.h_blind.assign(3 * (size_t)n * Wn, 0u);
    uint32_t *known = j.h_blind.data(), *value = known + (size_t)n * Wn, *cand = value + (size_t)n * Wn;
    bool any = false;
    for (int t = 0; t < n; t++) {
        const int i = j.idx[(size_t)t], kb = c.key_bits[i];
        const qldpc_recon_blind &b = c.blind[i];
        uint32_t *kn = known + (size_t)t * Wn, *va = value + (size_t)t * Wn, *ca = cand + (size_t)t * Wn;
        for (int w = 0; w < kb / 32; w++) ca[w] = 0xFFFFFFFFu;
        if (kb & 31) ca[kb / 32] = 0xFFFFFFFFu << (32 - (kb & 31));
        for (int k = 0; k < b.n_known; k++) {
            const uint32_t bit = 0x80000000u >> (b.pos[k] & 31);
            kn[b.pos[k] >> 5] |= bit; ca[b.pos[k] >> 5] &= ~bit;
            if (b.bit[k]) va[b.pos[k] >> 5] |= bit;
            any = true;
        }
    }
    uint32_t *d_known = e->d_blind, *d_value = d_known + (size_t)B * Wn, *d_cand = d_value + (size_t)B * Wn;
    if (any) {
        HIPCHK(hipMemcpyAsync(d_known, known, sizeof(uint32_t) * (size_t)n * Wn, hipMemcpyHostToDevice, s));
        HIPCHK(hipMemcpyAsync(d_value, value, sizeof(uint32_t) * (size_t)n * Wn, hipMemcpyHostToDevice, s));
    }
    HIPCHK(hipMemcpyAsync(d_cand, cand, sizeof(uint32_t) * (size_t)n * Wn, hipMemcpyHostToDevice, s));
    return any ? qldpc_load_known_dev(e->dec, d_known, d_value, n) : (int)QLDPC_OK;
}

/* the three parts of a job on the compute stream: load (after its staging has arrived), run, fetch + verify + results on their way back.  job_launch is
 * the three in order; a gang round (run_call_gang) loads every member, makes one gang run in place of the members' job_run, and fetches every member. */
static int job_load(lane_run *L, recon_job &j, hipStream_t cs)
{
    recon_entry *e = j.e;
    stage_set *st = j.st;
    hipStream_t s = L->lane->stream;
    const int n = (int)j.idx.size();
    const recon_in_view d = job_in(j, st->d_in);
    int rc;
    if (cs != s) HIPCHK(hipStreamWaitEvent(s, st->ev_in, 0));
    if (L->call->bob) {
        if ((rc = qldpc_decoder_set_stream(e->dec, (void *)s))) return rc;
        if ((rc = qldpc_load_bits_short_dev(e->dec, st->d_bits, d.mag, e->d_cls, d.key_bits, n))) return rc;
        if (j.any_punct && (rc = qldpc_load_erasures_dev(e->dec, st->d_erase, n))) return rc;
        if (L->call->blind && (rc = job_load_blind(L, j))) return rc;
    }
    return QLDPC_OK;
}

static int job_run(lane_run *L, recon_job &j)
{
    if (L->call->bob) return qldpc_run(j.e->dec);      /* the host polls the decoder's early-exit mailbox in here */
    return QLDPC_OK;                                   /* Alice: the encoder runs in job_fetch, with what reads its codewords */
}

/* the pool and the trial frames of an entry for a guessing call with `sources` blocks on it: allocated by the first such call, the pool again when a
 * call brings more blocks than it holds (it is empty between calls, and every call ends synchronised) */
static int entry_guess_pool(const qldpc_recon *r, recon_entry &e, int sources)
{
    const size_t B = (size_t)r->cfg.max_blocks, Wk = (size_t)e.K / 32, Wn = (size_t)(e.K + e.M + 31) / 32;
    const int cap = std::max(sources, r->cfg.max_blocks);
    if (!e.d_gtrial && dm_alloc(&e.mem, &e.d_gtrial, 4 * (B * Wn + B))) { qldpc_set_error("recon_decode_guess: device allocation failed"); return QLDPC_ENOMEM; }
    if (e.gpool_cap >= cap) return QLDPC_OK;
    dm_release(&e.mem, &e.d_gpool);
    e.gpool_cap = 0;
    /* ... then, for a tagged call, the tags and the hash-key rows of the sources: room for RT_MAX_KEYS keys each */
    const size_t words = recon_guess_pool_layout(nullptr, cap, (int)Wk, (int)Wn).words + recon_bob_layout(nullptr, cap, (int)Wk).words + (size_t)cap * RG_FIELDS + (size_t)cap * 4 * RT_MAX_KEYS;
    if (dm_alloc(&e.mem, &e.d_gpool, words)) { qldpc_set_error("recon_decode_guess: device allocation failed"); return QLDPC_ENOMEM; }
    e.gpool_cap = cap;
    return QLDPC_OK;
}

/* the rows of a trial launch in d_gtrial */
struct guess_trial_view { uint32_t *known, *value, *bits, *erase; float *mag; int *key_bits, *pass; uint32_t *crc; };
static guess_trial_view guess_trial_layout(const qldpc_recon *r, const recon_entry *e)
{
    const size_t B = (size_t)r->cfg.max_blocks, rows = B * ((size_t)(e->K + e->M + 31) / 32);
    uint32_t *b = e->d_gtrial;
    guess_trial_view v;
    v.known = b; v.value = b + rows; v.bits = b + 2 * rows; v.erase = b + 3 * rows;
    v.mag = reinterpret_cast<float *>(b + 4 * rows); v.key_bits = reinterpret_cast<int *>(b + 4 * rows + B); v.pass = reinterpret_cast<int *>(b + 4 * rows + 2 * B);
    v.crc = b + 4 * rows + 3 * B;
    return v;
}

/*
 * A guessing call, after the results of a job are on their way: they are waited for here (the wait job_finish makes anyway, made before the next job
 * is launched, because the posteriors of this decode are gone once the decoder is loaded again), and only a job with a failed block does more: the
 * select of the g weakest key positions of every failed block (the status column rk_verify wrote is the take column) and rk_guess_capture, which
 * keeps what the trials need in the entry's pool, device to device.  A job without a failure queues nothing.
 */
static int job_capture(lane_run *L, recon_job &j)
{
    recon_entry *e = j.e;
    stage_set *st = j.st;
    hipStream_t s = L->lane->stream;
    const int n = (int)j.idx.size(), Wk = e->K / 32, Wn = (e->K + e->M + 31) / 32;
    HIPCHK(hipEventSynchronize(st->ev_done));
    const recon_bob_view h = job_bob_res(j, st->h_res);
    int failed = 0;
    for (int t = 0; t < n; t++) failed += h.status[t] != QLDPC_OK;
    if (!failed) return QLDPC_OK;
    guess_sources *gs = nullptr;
    for (auto &x : L->guess) if (x.e == e) gs = &x;
    if (!gs) { L->guess.push_back(guess_sources{e, std::vector<int>(), false}); gs = &L->guess.back(); }
    const int base = (int)gs->idx.size();
    if (base + failed > e->gpool_cap) { qldpc_set_error("recon_decode_guess: %d failed blocks pass the pool of %d", base + failed, e->gpool_cap); return QLDPC_ESTATE; }
    const recon_in_view d = job_in(j, st->d_in);
    const recon_bob_view res = job_bob_res(j, st->d_res);
    const guess_trial_view tv = guess_trial_layout(L->r, e);
    uint32_t *d_cand = tv.value, *d_weak = tv.known;      /* free until the trial launches */
    hipLaunchKernelGGL(rk_guess_cand, dim3((unsigned)((Wn + RK_LANES - 1) / RK_LANES), (unsigned)n), dim3(RK_LANES), 0, s, d.key_bits, d_cand, Wk, Wn);
    HIPCHK(hipGetLastError());
    if (int rc = qldpc_fetch_weakest_dev(e->dec, d_cand, res.status, L->call->guess_bits, d_weak)) return rc;
    hipLaunchKernelGGL(rk_guess_capture, dim3((unsigned)n), dim3(RK_LANES), 0, s, res.status, e->d_iters, d_weak, e->d_out, st->d_bits, st->d_erase, d,
                       recon_guess_pool_layout(e->d_gpool, e->gpool_cap, Wk, Wn), base, e->gpool_cap, Wk, Wn);
    HIPCHK(hipGetLastError());
    for (int t = 0; t < n; t++) if (h.status[t] != QLDPC_OK) gs->idx.push_back(j.idx[(size_t)t]);
    gs->any_punct = gs->any_punct || j.any_punct;
    HIPCHK(hipStreamSynchronize(s));      /* the job's staging set may be written again; this is the recovery path */
    return QLDPC_OK;
}

/*
 * The trial launches of an entry, after the lane's ordinary jobs: S = floor(max_blocks / T) sources a launch in pool order (ascending block index).
 * Per launch: the known / value rows of the n_src T slots (qk_guess_expand, unchanged), the frame rows replicated onto them (rk_guess_sources), the
 * loads of a first decode plus qldpc_load_known_dev, the run, rk_guess_crc and rk_guess_settle.  One copy brings the results of all sources back.
 */
static int guess_drain(lane_run *L, guess_sources &gs)
{
    recon_entry *e = gs.e;
    const recon_call &c = *L->call;
    hipStream_t s = L->lane->stream;
    const int g = c.guess_bits, T = 1 << g, S = L->r->cfg.max_blocks / T, count = (int)gs.idx.size();
    const int N = e->K + e->M, Wk = e->K / 32, Wn = (N + 31) / 32;
    const recon_guess_pool_view pool = recon_guess_pool_layout(e->d_gpool, e->gpool_cap, Wk, Wn);
    uint32_t *res_base = e->d_gpool + pool.words;
    const recon_bob_view res = recon_bob_layout(res_base, count, Wk);
    int *d_guess = reinterpret_cast<int *>(res_base + res.words);
    const guess_trial_view tv = guess_trial_layout(L->r, e);
    int rc;
    if ((rc = qldpc_decoder_set_stream(e->dec, (void *)s))) return rc;
    for (int s0 = 0; s0 < count; s0 += S) {
        const int ns = std::min(S, count - s0), nf = ns * T;
        if ((rc = qldpc_guess_expand_dev(N, g, ns, pool.weak + (size_t)s0 * Wn, pool.hard + (size_t)s0 * Wn, tv.known, tv.value, (void *)s))) return rc;
        hipLaunchKernelGGL(rk_guess_sources, dim3((unsigned)((Wn + RK_LANES - 1) / RK_LANES), (unsigned)ns, (unsigned)std::min(T, 16)), dim3(RK_LANES), 0, s,
                           pool.bits + (size_t)s0 * Wn, pool.erase + (size_t)s0 * Wn, pool.mag + s0, pool.key_bits + s0, tv.bits, tv.erase, tv.mag, tv.key_bits, Wn, g);
        HIPCHK(hipGetLastError());
        if ((rc = qldpc_load_bits_short_dev(e->dec, tv.bits, tv.mag, e->d_cls, tv.key_bits, nf))) return rc;
        if (gs.any_punct && (rc = qldpc_load_erasures_dev(e->dec, tv.erase, nf))) return rc;
        if ((rc = qldpc_load_known_dev(e->dec, tv.known, tv.value, nf))) return rc;
        if ((rc = qldpc_run(e->dec))) return rc;
        if ((rc = qldpc_fetch_packed_dev(e->dec, e->d_out))) return rc;
        if ((rc = qldpc_fetch_status_dev(e->dec, e->d_iters, e->d_ok))) return rc;
        hipLaunchKernelGGL(rk_guess_crc, dim3((unsigned)ns, (unsigned)T), dim3(RK_LANES), 0, s, e->d_out, e->d_ok, pool.key_bits + s0, pool.crc + s0, tv.pass, tv.crc, Wk, Wn);
        hipLaunchKernelGGL(rk_guess_settle, dim3((unsigned)ns), dim3(RK_LANES), 0, s, e->d_out, e->d_ok, tv.pass, tv.crc, e->d_iters, pool.keys + (size_t)s0 * Wk,
                           pool.key_bits + s0, pool.iters + s0, res.keys + (size_t)s0 * Wk, res.status + s0, count, d_guess + (size_t)s0 * RG_FIELDS, Wk, Wn, g);
        HIPCHK(hipGetLastError());
    }
    const size_t tag_row = 2 * (size_t)c.n_keys;
    if (c.n_keys) {
        /* the tag of every rescued block, over the winners' keys where rk_guess_settle left them: the status column is the skip column, so a block
         * still failed gets zeros.  The tags lie behind the guess ints and travel back with them, the hash-key rows of the sources behind the tags */
        uint32_t *d_tags = res_base + res.words + (size_t)count * RG_FIELDS, *d_hk = d_tags + (size_t)count * tag_row;
        std::vector<uint32_t> hk((c.hash_shared ? 1 : (size_t)count) * tag_row);
        for (size_t k = 0; k * tag_row < hk.size(); k++) memcpy(hk.data() + k * tag_row, c.hash_keys[gs.idx[k]], sizeof(uint32_t) * tag_row);
        HIPCHK(hipMemcpyAsync(d_hk, hk.data(), sizeof(uint32_t) * hk.size(), hipMemcpyHostToDevice, s));
        HIPCHK(hipStreamSynchronize(s));      /* hk is this scope's */
        rk_tag_launch(c.n_keys, count, s, res.keys, pool.key_bits, res.status, d_hk, c.hash_shared ? 0 : tag_row, d_tags, Wk);
        HIPCHK(hipGetLastError());
    }
    std::vector<uint32_t> back(res.words + (size_t)count * RG_FIELDS + (size_t)count * tag_row);
    HIPCHK(hipMemcpyAsync(back.data(), res_base, sizeof(uint32_t) * back.size(), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    const recon_bob_view h = recon_bob_layout(back.data(), count, Wk);
    const int *hg = reinterpret_cast<const int *>(back.data() + h.words);
    for (int k = 0; k < count; k++) {
        const int i = gs.idx[(size_t)k];
        c.status[i] = h.status[k];
        if (c.corrected) c.corrected[i] = h.flips[k];
        if (c.iterations) c.iterations[i] = h.iters[k];
        if (h.status[k] == QLDPC_OK) memcpy(c.key[i], h.keys + (size_t)k * Wk, sizeof(uint32_t) * (size_t)((c.key_bits[i] + 31) / 32));      /* without a winner the key stays untouched */
        const int *f = hg + (size_t)k * RG_FIELDS;
        qldpc_recon_guess &out = c.guess[i];
        out.tried = f[0]; out.winner = f[1]; out.n_ok = f[2]; out.n_pass = f[3]; out.ambiguous = f[4]; out.trial_iterations = f[5];
        if (c.n_keys) memcpy(c.tags[i], back.data() + h.words + (size_t)count * RG_FIELDS + (size_t)k * tag_row, sizeof(uint32_t) * tag_row);
    }
    return QLDPC_OK;
}

static int job_fetch(lane_run *L, recon_job &j, hipStream_t cs)
{
    recon_entry *e = j.e;
    stage_set *st = j.st;
    hipStream_t s = L->lane->stream;
    const int n = (int)j.idx.size(), K = e->K, M = e->M, N = K + M;
    const int Wk = K / 32, Wn = (N + 31) / 32, Wm = (M + 31) / 32;
    int rc;
    const recon_in_view d = job_in(j, st->d_in);
    size_t res_words;
    if (L->call->bob) {
        if ((rc = qldpc_fetch_packed_dev(e->dec, e->d_out))) return rc;
        if ((rc = qldpc_fetch_status_dev(e->dec, e->d_iters, e->d_ok))) return rc;
        const recon_bob_view res = job_bob_res(j, st->d_res);
        res_words = res.words;
        if (const int r = L->call->n_keys) {      /* the same verdict with the tags of the good blocks, behind the result block: they travel back with it */
            rk_verify_tag_launch(r, n, s, e->d_out, d.keys, d.key_bits, d.crc, e->d_ok, e->d_iters, st->d_in + d.words, L->call->hash_shared ? 0 : 2 * (size_t)r,
                                 res.keys, res.status, st->d_res + res.words, Wk, Wn);
            res_words += (size_t)n * 2 * (size_t)r;
        } else
            hipLaunchKernelGGL(rk_verify, dim3((unsigned)n), dim3(RK_LANES), 0, s, e->d_out, d.keys, d.key_bits, d.crc, e->d_ok, e->d_iters, res.keys, res.status, n, Wk, Wn);
        HIPCHK(hipGetLastError());
        if (L->call->blind) {
            /* the request of every block that failed: its ask_bits weakest candidates, out of the posteriors of this decode.  The status column
             * rk_verify just wrote is the take column (QLDPC_OK = 0 = not wanted).  The rows are waited for here: a blind round gives up the
             * overlap of neighbouring jobs, it is the recovery path */
            const int B = L->r->cfg.max_blocks;
            uint32_t *d_cand = e->d_blind + 2 * (size_t)B * Wn, *d_weak = d_cand + (size_t)B * Wn;
            if ((rc = qldpc_fetch_weakest_dev(e->dec, d_cand, res.status, L->call->ask_bits, d_weak))) return rc;
            j.h_weak.assign((size_t)n * Wn, 0u);
            HIPCHK(hipMemcpyAsync(j.h_weak.data(), d_weak, sizeof(uint32_t) * (size_t)n * Wn, hipMemcpyDeviceToHost, s));
            HIPCHK(hipStreamSynchronize(s));
        }
    } else {
        if ((rc = qldpc_encode_packed_dev(e->enc, d.keys, e->d_out, n, (void *)s))) return rc;
        const recon_alice_view res = job_alice_res(j, st->d_res);
        hipLaunchKernelGGL(rk_disclose, dim3((unsigned)((Wm + 255) / 256), (unsigned)n), dim3(256), 0, s, e->d_out, d.n_punct, res.disc, Wk, Wn, Wm, M);
        hipLaunchKernelGGL(rk_crc, dim3((unsigned)n), dim3(RK_LANES), 0, s, d.keys, d.key_bits, res.crc, Wk);
        HIPCHK(hipGetLastError());
        res_words = res.words;
    }
    if (cs != s) {
        HIPCHK(hipEventRecord(st->ev_out, s));
        HIPCHK(hipStreamWaitEvent(cs, st->ev_out, 0));
    }
    HIPCHK(hipMemcpyAsync(st->h_res, st->d_res, sizeof(uint32_t) * res_words, hipMemcpyDeviceToHost, cs));
    HIPCHK(hipEventRecord(st->ev_done, cs));
    if (L->call->bob && L->call->guess_bits) return job_capture(L, j);
    return QLDPC_OK;
}

static int job_launch(lane_run *L, recon_job &j, hipStream_t cs)
{
    int rc;
    if ((rc = job_load(L, j, cs)) || (rc = job_run(L, j)) || (rc = job_fetch(L, j, cs))) return rc;
    return QLDPC_OK;
}

static int job_finish(lane_run *L, recon_job &j)
{
    recon_entry *e = j.e;
    stage_set *st = j.st;
    const recon_call &c = *L->call;
    const int n = (int)j.idx.size(), K = e->K, M = e->M;
    const int Wk = K / 32, Wm = (M + 31) / 32;
    HIPCHK(hipEventSynchronize(st->ev_done));
    if (c.bob) {
        const recon_bob_view res = job_bob_res(j, st->h_res);
        for (int t = 0; t < n; t++) {
            const int i = j.idx[(size_t)t], Wkey = (c.key_bits[i] + 31) / 32;
            c.status[i] = res.status[t];
            if (c.corrected) c.corrected[i] = res.flips[t];
            if (c.iterations) c.iterations[i] = res.iters[t];
            if (res.status[t] == QLDPC_OK) memcpy(c.key[i], res.keys + (size_t)t * Wk, sizeof(uint32_t) * (size_t)Wkey);      /* a failed block keeps its key untouched */
            if (c.n_keys) memcpy(c.tags[i], st->h_res + res.words + (size_t)t * 2 * (size_t)c.n_keys, sizeof(uint32_t) * 2 * (size_t)c.n_keys);      /* zeros for a failed block */
            if (c.blind) {
                qldpc_recon_blind &b = c.blind[i];
                b.n_ask = 0;
                const size_t Wn = (size_t)(K + M + 31) / 32;
                const uint32_t *row = j.h_weak.data() + (size_t)t * Wn;
                for (int v = 0; res.status[t] != QLDPC_OK && v < c.key_bits[i] && b.n_ask < c.ask_bits; v++)
                    if ((row[v >> 5] >> (31 - (v & 31))) & 1u) b.ask[b.n_ask++] = v;
            }
        }
    } else {
        const recon_alice_view res = job_alice_res(j, st->h_res);
        for (int t = 0; t < n; t++) {
            const int i = j.idx[(size_t)t];
            memcpy(c.aparity[i], res.disc + (size_t)t * Wm, sizeof(uint32_t) * (size_t)qldpc_recon_parity_words(&c.amsgs[i]));
            c.amsgs[i].crc32 = res.crc[t];
        }
    }
    return QLDPC_OK;
}

/*
 * The software pipeline of one host worker, over rounds (a round = the jobs that are launched together; a lane's rounds hold one job each, a gang
 * round one job per group): round k + 1 is staged, round k launched, round k - 1 finished, and at the end the rounds still under way are finished.
 * On an error both streams of the lane are synchronised and L->err keeps the text of the first one.
 * The two staging sets of an entry alternate between its jobs, and the host writes a set's pinned block while the job two back may still be on its way.
 * wait_for_set (the gang rounds): with three jobs per code the set's previous user is waited for (its ev_done) before job_stage writes h_in.  The lanes
 * do not wait: their order (stage k + 1, launch k, finish k - 1) has the set free by then, and a wait would put a host stall in front of Alice's staging.
 */
typedef std::vector<recon_job *> recon_round;

template <class Launch>
static int run_rounds(lane_run *L, const std::vector<recon_round> &rounds, hipStream_t cs, bool wait_for_set, Launch launch)
{
    auto stage = [&](const recon_round &rd) -> int {
        for (recon_job *j : rd) {
            if (wait_for_set) HIPCHK(hipEventSynchronize(j->e->set[j->e->next_set].ev_done));
            if (int rc = job_stage(L, *j, cs)) return rc;
        }
        return QLDPC_OK;
    };
    auto finish = [&](const recon_round &rd) -> int {
        for (recon_job *j : rd)
            if (int rc = job_finish(L, *j)) return rc;
        return QLDPC_OK;
    };
    const size_t nr = rounds.size();
    size_t launched = 0, finished = 0;
    int rc = stage(rounds[0]);
    for (size_t k = 0; k < nr && !rc; k++) {
        if (k + 1 < nr) rc = stage(rounds[k + 1]);
        if (!rc) { rc = launch(rounds[k]); if (!rc) launched = k + 1; }
        if (!rc && k > 0) { rc = finish(rounds[k - 1]); if (!rc) finished = k; }
    }
    for (size_t k = finished; k < launched && !rc; k++) rc = finish(rounds[k]);
    if (rc) {
        L->err = qldpc_last_error();
        (void)hipStreamSynchronize(L->lane->stream);
        (void)hipStreamSynchronize(L->lane->copy);
    }
    return rc;
}

static void lane_main(lane_run *L)
{
    const bool dbg = getenv("QLDPC_DEBUG") != nullptr;
    const auto t_start = std::chrono::steady_clock::now();
    if (hipSetDevice(L->r->cfg.device) != hipSuccess) { L->rc = QLDPC_EHIP; L->err = "hipSetDevice failed"; return; }
    const size_t nj = L->jobs.size();
    /* one job: everything in order on the compute stream (no cross-stream hand-offs on the daemon's one-block path) */
    hipStream_t cs = nj > 1 ? L->lane->copy : L->lane->stream;
    std::vector<recon_round> rounds;
    for (auto &j : L->jobs) rounds.push_back(recon_round(1, &j));
    L->rc = run_rounds(L, rounds, cs, false, [&](const recon_round &rd) { return job_launch(L, *rd[0], cs); });
    /* guessing rounds: every ordinary job has reported by now, the trial launches of the entries that had a failure overwrite what they reported */
    for (auto &gs : L->guess) {
        if (L->rc) break;
        if ((L->rc = guess_drain(L, gs))) { L->err = qldpc_last_error(); (void)hipStreamSynchronize(L->lane->stream); }
    }
    if (dbg) {
        size_t blocks = 0;
        for (auto &j : L->jobs) blocks += j.idx.size();
        fprintf(stderr, "libqldpc: recon lane %d: %zu job(s), %zu blocks, first code K %d M %d, %.3f ms\n", (int)(L->lane - L->r->lane), nj, blocks, L->jobs[0].e->K, L->jobs[0].e->M,
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count());
    }
}

/* groups: the blocks of a call that are not skipped, by code.  Entries are looked up / built here, in the calling thread. */
struct recon_group { recon_entry *e; std::vector<int> idx; double cost; };

static int call_groups(qldpc_recon *r, const recon_call &call, const std::vector<char> &skip, std::vector<recon_group> &groups)
{
    const qldpc_recon_msg *msgs = call.bob ? call.msgs : call.amsgs;
    std::vector<char> taken(skip);
    for (int i = 0; i < call.n; i++) {
        if (taken[(size_t)i]) continue;
        recon_group g;
        for (int j = i; j < call.n; j++)
            if (!taken[(size_t)j] && msgs[j].code_k == msgs[i].code_k && msgs[j].code_m == msgs[i].code_m) { g.idx.push_back(j); taken[(size_t)j] = 1; }
        if (int rc = get_entry(r, (int)msgs[i].code_k, (int)msgs[i].code_m, &g.e)) return rc;
        g.cost = (double)g.idx.size() * (double)(msgs[i].code_k + msgs[i].code_m);
        groups.push_back(std::move(g));
    }
    return QLDPC_OK;
}

/* the jobs of a group: its blocks in batches of up to max_blocks */
static std::vector<recon_job> group_jobs(const qldpc_recon *r, const recon_group &g)
{
    const size_t B = (size_t)r->cfg.max_blocks;
    std::vector<recon_job> jobs;
    for (size_t at = 0; at < g.idx.size(); at += B) {
        recon_job j;
        j.e = g.e; j.st = nullptr; j.any_punct = false;
        j.idx.assign(g.idx.begin() + (long)at, g.idx.begin() + (long)std::min(g.idx.size(), at + B));
        jobs.push_back(std::move(j));
    }
    return jobs;
}

/*
 * QLDPC_RECON_GANG=1, Bob's side, two or more rate groups with layered decoders: the call runs on ONE host thread and one lane, in rounds.  Round k
 * takes the k-th job of every group: all are staged (while round k - 1 decodes), every member is loaded, ONE gang run steps them in lockstep (a launch
 * per colour step and kernel class for all of them instead of a launch per group on its own stream), every member is fetched and verified.  A round
 * that only one group still takes part in runs as a job of today's path.  What a block reports is what job_launch gives: the gang run is bit-identical
 * to the members' own runs.
 */
static int run_call_gang(qldpc_recon *r, const recon_call &call, std::vector<recon_group> &groups)
{
    lane_run L = lane_of(r, 0, call);
    hipStream_t s = L.lane->stream, cs = L.lane->copy;
    std::vector<std::vector<recon_job>> jobs;
    std::vector<recon_round> rounds;
    for (auto &g : groups) jobs.push_back(group_jobs(r, g));
    for (auto &gj : jobs) {
        if (rounds.size() < gj.size()) rounds.resize(gj.size());
        for (size_t k = 0; k < gj.size(); k++) rounds[k].push_back(&gj[k]);
    }
    qldpc_gang *gang = nullptr;
    std::vector<qldpc_decoder *> members, have;
    int rc = run_rounds(&L, rounds, cs, true, [&](const recon_round &rd) -> int {
        if (rd.size() == 1) return job_launch(&L, *rd[0], cs);
        int rc = QLDPC_OK;
        members.clear();
        for (recon_job *j : rd) members.push_back(j->e->dec);
        if (members != have) {      /* groups drop out as their jobs run out: a gang per set of members, at most one per group and call */
            qldpc_gang_free(gang); gang = nullptr; have.clear();
            rc = qldpc_gang_create(members.data(), (int)members.size(), &gang);
            if (!rc) { have = members; rc = qldpc_gang_set_stream(gang, (void *)s); }
        }
        for (size_t t = 0; t < rd.size() && !rc; t++) rc = job_load(&L, *rd[t], cs);
        if (!rc) rc = qldpc_gang_run(gang, nullptr);
        for (size_t t = 0; t < rd.size() && !rc; t++) rc = job_fetch(&L, *rd[t], cs);
        return rc;
    });
    qldpc_gang_free(gang);
    if (rc) qldpc_set_error("%s", L.err.c_str());
    return rc;
}

/* jobs of one entry stay on one lane, the entries are dealt onto the lanes largest first */
static int run_call(qldpc_recon *r, const recon_call &call, const std::vector<char> &skip)
{
    int rc;
    HIPCHK(hipSetDevice(r->cfg.device));
    std::vector<recon_group> groups;
    if ((rc = call_groups(r, call, skip, groups))) { cache_trim(r); return rc; }
    if (groups.empty()) return QLDPC_OK;
    int n_lanes = RECON_LANES;
    if (const char *env = getenv("QLDPC_RECON_LANES")) n_lanes = std::max(1, std::min(RECON_LANES, atoi(env)));
    n_lanes = std::min(n_lanes, (int)groups.size());
    std::sort(groups.begin(), groups.end(), [](const recon_group &a, const recon_group &b) { return a.cost > b.cost; });
    if (call.bob && call.guess_bits)
        for (auto &g : groups)
            if ((rc = entry_guess_pool(r, *g.e, (int)g.idx.size()))) { cache_trim(r); return rc; }
    if (r->gang && call.bob && !call.blind && !call.guess_bits && !call.n_keys && groups.size() >= 2 && groups.size() <= (size_t)QLDPC_GANG_MAX_MEMBERS) {
        /* only when every group's decoder can be a member (layered sessions); otherwise today's path */
        std::vector<qldpc_decoder *> decs;
        for (auto &g : groups) decs.push_back(g.e->dec);
        qldpc_gang *probe = nullptr;
        if (qldpc_gang_create(decs.data(), (int)decs.size(), &probe) == QLDPC_OK) {
            qldpc_gang_free(probe);
            rc = run_call_gang(r, call, groups);
            cache_trim(r);
            return rc;
        }
    }
    std::vector<lane_run> runs;
    std::vector<double> load((size_t)n_lanes, 0.0);
    for (int l = 0; l < n_lanes; l++) runs.push_back(lane_of(r, l, call));
    for (auto &g : groups) {
        const size_t l = (size_t)(std::min_element(load.begin(), load.end()) - load.begin());
        load[l] += g.cost;
        for (auto &j : group_jobs(r, g)) runs[l].jobs.push_back(std::move(j));
    }
    if (n_lanes == 1) lane_main(&runs[0]);
    else {
        std::vector<std::thread> th;
        for (int l = 1; l < n_lanes; l++) th.emplace_back(lane_main, &runs[(size_t)l]);
        lane_main(&runs[0]);
        for (auto &t : th) t.join();
    }
    rc = QLDPC_OK;
    for (auto &L : runs)
        if (L.rc && !rc) { rc = L.rc; qldpc_set_error("%s", L.err.c_str()); }
    cache_trim(r);
    return rc;
}

/*
 * Alice's side for many blocks at once: plans every block (msgs[i] is filled as by qldpc_recon_encode), groups the blocks by
 * code and encodes each group in launches of up to max_blocks frames.  parity_words[i] receives qldpc_recon_parity_words(&msgs[i])
 * words (parity_cap[i] are available).  The key's CRC-32 is computed on the device as well (rk_crc).
 */
extern "C" int qldpc_recon_encode_blocks(qldpc_recon *r, int n, const uint32_t *const *key_words, const int *key_bits, const float *qber,
                                         qldpc_recon_msg *msgs, uint32_t *const *parity_words, const int *parity_cap)
{
    if (!r || !key_words || !key_bits || !qber || !msgs || !parity_words || !parity_cap || n <= 0) return QLDPC_EINVAL;
    int rc;
    for (int i = 0; i < n; i++) {
        if (!key_words[i] || !parity_words[i]) return QLDPC_EINVAL;
        if ((rc = qldpc_recon_plan(r, key_bits[i], qber[i], &msgs[i]))) return rc;
        if (parity_cap[i] < qldpc_recon_parity_words(&msgs[i])) { qldpc_set_error("recon_encode_blocks: parity buffer %d holds %d words, need %d", i, parity_cap[i], qldpc_recon_parity_words(&msgs[i])); return QLDPC_ESIZE; }
    }
    return run_call(r, call_alice(n, key_words, key_bits, msgs, parity_words), std::vector<char>((size_t)n, 0));
}

extern "C" int qldpc_recon_encode(qldpc_recon *r, const uint32_t *key_words, int key_bits, float qber, qldpc_recon_msg *msg, uint32_t *parity_words, int cap)
{
    if (!r || !key_words || !msg || !parity_words) return QLDPC_EINVAL;
    const uint32_t *k = key_words;
    uint32_t *p = parity_words;
    return qldpc_recon_encode_blocks(r, 1, &k, &key_bits, &qber, msg, &p, &cap);
}

/*
 * Alice, second round: the parity bits of a plan that is already on the table (msg as qldpc_recon_plan / qldpc_recon_encode left it, n_punct
 * possibly lowered by the caller -- 0 = every parity bit of the mother code).  After a failed decode the bits withheld by puncturing are
 * the cheapest thing to send next (incremental redundancy): the same codeword, a lower effective rate.  msg->crc32 is (re)written.
 */
extern "C" int qldpc_recon_encode_planned(qldpc_recon *r, const uint32_t *key_words, int key_bits, qldpc_recon_msg *msg, uint32_t *parity_words, int cap)
{
    if (!r || !key_words || !msg || !parity_words) return QLDPC_EINVAL;
    int rc;
    if ((rc = check_msg(r, msg, key_bits))) return rc;
    if (cap < qldpc_recon_parity_words(msg)) { qldpc_set_error("recon_encode_planned: parity buffer holds %d words, need %d", cap, qldpc_recon_parity_words(msg)); return QLDPC_ESIZE; }
    return run_call(r, call_alice(1, &key_words, &key_bits, msg, &parity_words), std::vector<char>(1, 0));
}

/*
 * The Bob-side prologue of block i, shared by qldpc_recon_decode_blocks, qldpc_recon_decode_blind, qldpc_recon_decode_guess and qldpc_recon_estimate_blocks: QLDPC_EINVAL for a NULL
 * key or parity pointer (nothing of the block is written), else the block's outputs at their failure values and *skip = is it left out of the call: its
 * header does not match the block or the local plan, or its QBER is out of range (status QLDPC_ESIZE).  qber_out != NULL is a call that estimates: it has
 * no QBER to check and no status, and zeroes qber_out[i] instead.
 */
static int bob_block_begin(const qldpc_recon *r, const recon_call &c, int i, float *qber_out, char *skip)
{
    if (!c.key[i] || !c.parity[i]) return QLDPC_EINVAL;
    if (qber_out) qber_out[i] = 0.0f;
    else {
        c.status[i] = QLDPC_EDECODE;
        if (c.corrected) c.corrected[i] = 0;
        if (c.iterations) c.iterations[i] = 0;
    }
    *skip = check_msg(r, &c.msgs[i], c.key_bits[i]) || (!qber_out && !(c.qber[i] >= 0.0f && c.qber[i] < 0.5f));
    if (*skip && !qber_out) c.status[i] = QLDPC_ESIZE;
    return QLDPC_OK;
}

/*
 * The tag arguments of a tagged Bob-side call, checked before anything is queued or written: n_keys outside 1 .. RT_MAX_KEYS and a NULL hash-key or tag
 * row are QLDPC_EINVAL, and the error names the block (a NULL key or parity row is refused here as well, before a tag row is written).  Then the call
 * carries them, with hash_shared = every block points to one row; every block's tag starts as zeros, which is what a block that is left out or fails keeps.
 */
static int call_take_tags(const char *who, recon_call &c, int n_keys, const uint32_t *const *hash_keys, uint32_t *const *tag_words)
{
    if (n_keys < 1 || n_keys > RT_MAX_KEYS) { qldpc_set_error("%s: n_keys = %d, outside 1 .. %d", who, n_keys, RT_MAX_KEYS); return QLDPC_EINVAL; }
    if (!hash_keys || !tag_words) { qldpc_set_error("%s: the hash_keys and tag_words arrays are needed", who); return QLDPC_EINVAL; }
    bool shared = true;
    for (int i = 0; i < c.n; i++) {
        if (!c.key[i] || !c.parity[i]) return QLDPC_EINVAL;
        if (!hash_keys[i] || !tag_words[i]) { qldpc_set_error("%s: block %d has no %s row", who, i, !hash_keys[i] ? "hash-key" : "tag"); return QLDPC_EINVAL; }
        shared = shared && hash_keys[i] == hash_keys[0];
    }
    for (int i = 0; i < c.n; i++) memset(tag_words[i], 0, sizeof(uint32_t) * 2 * (size_t)n_keys);
    c.n_keys = n_keys; c.hash_keys = hash_keys; c.tags = tag_words; c.hash_shared = shared;
    return QLDPC_OK;
}

/*
 * Blocks of any mix of lengths, rates and puncturing in one call ("let many blocks queue and decode in one
 * launch"): blocks are grouped by code (code_k, code_m), every group goes through its decoder in batches of up to max_blocks
 * frames, and the groups of a call run side by side (the pipeline above); within a group the blocks may differ in length
 * (shortening per frame) and in efficiency (puncturing per frame).  keys are decoded in place.
 * Every message is validated on its own: status[i] = QLDPC_OK | QLDPC_EDECODE | QLDPC_ESIZE (header does not match the block /
 * the local plan -- that block is not decoded, the others are).  `tagged`: qldpc_recon_decode_blocks_tagged, the same call with the tag arguments.
 */
static int decode_blocks_call(const char *who, bool tagged, qldpc_recon *r, int n, uint32_t *const *key_words, const int *key_bits, const float *qber,
                              const qldpc_recon_msg *msgs, const uint32_t *const *parity_words, int n_keys, const uint32_t *const *hash_keys,
                              uint32_t *const *tag_words, int *status, int *corrected, int *iterations)
{
    if (!r || !key_words || !key_bits || !qber || !msgs || !parity_words || !status || n <= 0) return QLDPC_EINVAL;
    recon_call c = call_bob(n, key_words, key_bits, qber, msgs, parity_words, status, corrected, iterations);
    if (tagged)
        if (int rc = call_take_tags(who, c, n_keys, hash_keys, tag_words)) return rc;
    std::vector<char> skip((size_t)n, 0);
    for (int i = 0; i < n; i++)
        if (int rc = bob_block_begin(r, c, i, nullptr, &skip[(size_t)i])) return rc;
    return run_call(r, c, skip);
}

extern "C" int qldpc_recon_decode_blocks(qldpc_recon *r, int n, uint32_t *const *key_words, const int *key_bits, const float *qber,
                                         const qldpc_recon_msg *msgs, const uint32_t *const *parity_words, int *status, int *corrected, int *iterations)
{
    return decode_blocks_call("recon_decode_blocks", false, r, n, key_words, key_bits, qber, msgs, parity_words, 0, nullptr, nullptr, status, corrected, iterations);
}

/*
 * qldpc_recon_decode_blocks with the keyed tag of every verified block (qldpc_recon_tag_core.h): the same first pass -- validation, grouping, lanes,
 * staging sets and pipeline -- with rk_verify_tag in the place of rk_verify, so the decoded rows are hashed where they lie on the device.  The hash-key
 * rows travel with the input block of a job and the tags come back with its result block; an entry's staging has the room from its creation on.
 */
extern "C" int qldpc_recon_decode_blocks_tagged(qldpc_recon *r, int n, uint32_t *const *key_words, const int *key_bits, const float *qber, const qldpc_recon_msg *msgs,
                                                const uint32_t *const *parity_words, int n_keys, const uint32_t *const *hash_keys, uint32_t *const *tag_words,
                                                int *status, int *corrected, int *iterations)
{
    return decode_blocks_call("recon_decode_blocks_tagged", true, r, n, key_words, key_bits, qber, msgs, parity_words, n_keys, hash_keys, tag_words, status, corrected, iterations);
}

/*
 * The QBER every block's parity message shows (qldpc_qber_estimate_dev on the frames qldpc_recon_decode_blocks would decode): same validation, grouping,
 * staging and assembly (job_stage), then the entry's estimator in place of the decoder, one job at a time on the first lane.  The pooled estimate is
 * taken on the host from the counts of all blocks summed by effective degree (the codes of a call differ in their largest check degree).
 */
static int estimate_blocks(qldpc_recon *r, bool merge, int n, const uint32_t *const *key_words, const int *key_bits, const qldpc_recon_msg *msgs,
                           const uint32_t *const *parity_words, float *qber_out, uint32_t *counts_out, float *pool_qber_out)
{
    if (!r || !key_words || !key_bits || !msgs || !parity_words || !qber_out || n <= 0) return QLDPC_EINVAL;
    const size_t BINS = 2 * (QLDPC_QBER_MAX_DEGREE + 1);
    const recon_call call = call_bob(n, const_cast<uint32_t *const *>(key_words), key_bits, nullptr, msgs, parity_words, nullptr, nullptr, nullptr);
    std::vector<char> skip((size_t)n, 0);
    int rc = QLDPC_OK, max_d = 0;
    for (int i = 0; i < n; i++)
        if ((rc = bob_block_begin(r, call, i, qber_out, &skip[(size_t)i]))) return rc;
    if (counts_out) memset(counts_out, 0, sizeof(uint32_t) * (size_t)n * BINS);
    if (pool_qber_out) *pool_qber_out = 0.0f;
    HIPCHK(hipSetDevice(r->cfg.device));
    lane_run L = lane_of(r, 0, call);
    hipStream_t s = L.lane->stream;
    const size_t B = (size_t)r->cfg.max_blocks;
    std::vector<uint64_t> pool(BINS, 0);
    std::vector<uint32_t> h_est;
    std::vector<recon_group> groups;
    rc = call_groups(r, call, skip, groups);
    for (size_t g = 0; g < groups.size() && !rc; g++) {
        recon_entry *e = groups[g].e;
        if ((rc = entry_estimator(r, *e, merge))) break;
        qldpc_qber *est = merge ? e->qest_m : e->qest;
        const int D = qldpc_qber_count_rows(est) - 1;
        const size_t bins = 2 * (size_t)(D + 1);
        max_d = std::max(max_d, D);
        if ((rc = qldpc_qber_set_stream(est, (void *)s))) break;
        for (recon_job &j : group_jobs(r, groups[g])) {
            const int nb = (int)j.idx.size();
            if ((rc = job_stage(&L, j, s))) break;
            uint32_t *d_counts = e->d_est;
            float *d_q = reinterpret_cast<float *>(d_counts + B * bins);
            rc = qldpc_qber_estimate_dev(est, j.st->d_bits, e->d_cls, job_in(j, j.st->d_in).key_bits, nullptr, j.any_punct ? j.st->d_erase : nullptr, nullptr, nullptr, nb,
                                         d_counts, nullptr, d_q, nullptr, nullptr, nullptr);
            if (rc) break;
            h_est.resize((size_t)nb * (bins + 1));
            hipError_t he = hipMemcpyAsync(h_est.data(), d_counts, sizeof(uint32_t) * (size_t)nb * bins, hipMemcpyDeviceToHost, s);
            if (he == hipSuccess) he = hipMemcpyAsync(h_est.data() + (size_t)nb * bins, d_q, sizeof(float) * (size_t)nb, hipMemcpyDeviceToHost, s);
            if (he == hipSuccess) he = hipStreamSynchronize(s);      /* the staging set's pinned block is free again as well */
            if (he != hipSuccess) { qldpc_set_error("recon_estimate_blocks: %s", hipGetErrorString(he)); rc = QLDPC_EHIP; break; }
            for (int t = 0; t < nb; t++) {
                const int b = j.idx[(size_t)t];
                memcpy(&qber_out[b], h_est.data() + (size_t)nb * bins + t, sizeof(float));
                const uint32_t *row = h_est.data() + (size_t)t * bins;
                if (counts_out) memcpy(counts_out + (size_t)b * BINS, row, sizeof(uint32_t) * bins);
                for (size_t k = 0; k < bins; k++) pool[k] += row[k];
            }
        }
    }
    if (rc) (void)hipStreamSynchronize(s);
    if (!rc && pool_qber_out && max_d > 0) {
        qldpc_qber_cfg qc;
        qldpc_qber_cfg_default(&qc);
        std::vector<int32_t> L1((size_t)(max_d + 1) * (size_t)qc.n_grid), L0(L1.size());
        std::vector<float> q((size_t)qc.n_grid);
        int k = -1;
        rc = qldpc_qber_table_host(max_d, qc.n_grid, qc.q_lo, qc.q_hi, L1.data(), L0.data(), q.data(), nullptr);
        if (!rc) rc = qldpc_qber_argmax_host(pool.data(), max_d, qc.n_grid, L1.data(), L0.data(), &k);
        if (!rc && k >= 0) *pool_qber_out = q[(size_t)k];
    }
    cache_trim(r);
    return rc;
}

extern "C" int qldpc_recon_estimate_blocks(qldpc_recon *r, int n, const uint32_t *const *key_words, const int *key_bits, const qldpc_recon_msg *msgs,
                                           const uint32_t *const *parity_words, float *qber_out, uint32_t *counts_out, float *pool_qber_out)
{
    return estimate_blocks(r, false, n, key_words, key_bits, msgs, parity_words, qber_out, counts_out, pool_qber_out);
}

/* the same through the entries' merged estimators: runs of checks across punctured parity bits are one observation each */
extern "C" int qldpc_recon_estimate_blocks_merged(qldpc_recon *r, int n, const uint32_t *const *key_words, const int *key_bits, const qldpc_recon_msg *msgs,
                                                  const uint32_t *const *parity_words, float *qber_out, uint32_t *counts_out, float *pool_qber_out)
{
    return estimate_blocks(r, true, n, key_words, key_bits, msgs, parity_words, qber_out, counts_out, pool_qber_out);
}

/*
 * One round of blind reconciliation: qldpc_recon_decode_blocks with the positions of blind[i] pinned to Alice's bits; a block that fails comes
 * back with the positions to ask for next.  Stateless across rounds: the caller appends Alice's answers to pos / bit and calls again with the
 * same messages.  The gang path is not taken by these calls.
 */
extern "C" int qldpc_recon_decode_blind(qldpc_recon *r, int n, uint32_t *const *key_words, const int *key_bits, const float *qber, const qldpc_recon_msg *msgs,
                                        const uint32_t *const *parity_words, qldpc_recon_blind *blind, int ask_bits, int *status, int *corrected, int *iterations,
                                        int *leaked)
{
    if (!r || !key_words || !key_bits || !qber || !msgs || !parity_words || !blind || !status || n <= 0 || ask_bits < 0) return QLDPC_EINVAL;
    if (!cfg_layered(r->cfg) && r->cfg.max_blocks <= 8) {
        qldpc_set_error("recon_decode_blind: the decoders of a session with max_blocks <= 8 and the flooding schedule run on the edge-parallel engine, which has no weakest-VN select");
        return QLDPC_EUNSUPPORTED;
    }
    const recon_call c = call_bob(n, key_words, key_bits, qber, msgs, parity_words, status, corrected, iterations, blind, ask_bits);
    std::vector<char> skip((size_t)n, 0);
    std::vector<uint32_t> seen;
    for (int i = 0; i < n; i++) {
        qldpc_recon_blind &b = blind[i];
        if (b.n_known < 0 || (b.n_known && (!b.pos || !b.bit)) || (ask_bits && !b.ask) || key_bits[i] <= 0) return QLDPC_EINVAL;
        seen.assign((size_t)(key_bits[i] + 31) / 32, 0u);
        for (int k = 0; k < b.n_known; k++) {
            const int p = b.pos[k];
            if (p < 0 || p >= key_bits[i] || ((seen[(size_t)p >> 5] >> (31 - (p & 31))) & 1u)) {
                qldpc_set_error("recon_decode_blind: block %d, known position %d (entry %d) is repeated or not below key_bits = %d", i, p, k, key_bits[i]);
                return QLDPC_EINVAL;
            }
            seen[(size_t)p >> 5] |= 0x80000000u >> (p & 31);
        }
        if (int rc = bob_block_begin(r, c, i, nullptr, &skip[(size_t)i])) return rc;
        b.n_ask = 0;
        if (leaked) leaked[i] = qldpc_recon_leaked_bits(&msgs[i]) + b.n_known;
    }
    return run_call(r, c, skip);
}

/*
 * qldpc_recon_decode_blocks with guessing rounds: a block whose first decode ends QLDPC_EDECODE is decoded again with its guess_bits weakest key
 * positions pinned to each of the 2^guess_bits values, and the lowest trial with a zero syndrome and Alice's CRC is kept (qldpc_recon_guess_core.h).
 * Local to Bob, nothing is disclosed.  guess_bits = 0, or a call without a failed block, is qldpc_recon_decode_blocks: a guessing call waits for the
 * results of a job before it launches the next one of the lane (the wait job_finish makes), and only a job with a failure queues anything more
 * (job_capture); the trial launches follow the lane's ordinary jobs (guess_drain).  The gang path is not taken by these calls.
 */
static int decode_guess_call(const char *who, bool tagged, qldpc_recon *r, int n, uint32_t *const *key_words, const int *key_bits, const float *qber,
                             const qldpc_recon_msg *msgs, const uint32_t *const *parity_words, int guess_bits, qldpc_recon_guess *guess, int n_keys,
                             const uint32_t *const *hash_keys, uint32_t *const *tag_words, int *status, int *corrected, int *iterations)
{
    if (!r || !key_words || !key_bits || !qber || !msgs || !parity_words || !status || n <= 0) return QLDPC_EINVAL;
    if (guess_bits > 0 && !guess) { qldpc_set_error("recon_decode_guess: guess_bits = %d needs the guess array (one qldpc_recon_guess per block)", guess_bits); return QLDPC_EINVAL; }
    if (guess_bits < 0 || guess_bits > QLDPC_GUESS_MAX_BITS) {
        qldpc_set_error("recon_decode_guess: guess_bits = %d, outside 0 .. %d", guess_bits, QLDPC_GUESS_MAX_BITS);
        return QLDPC_ESIZE;
    }
    if ((1 << guess_bits) > r->cfg.max_blocks) {
        qldpc_set_error("recon_decode_guess: the %d trials of a block do not fit a launch of max_blocks = %d frames: lower guess_bits or make the session with max_blocks >= %d",
                        1 << guess_bits, r->cfg.max_blocks, 1 << guess_bits);
        return QLDPC_ESIZE;
    }
    if (!cfg_layered(r->cfg) && r->cfg.max_blocks <= 8) {
        qldpc_set_error("recon_decode_guess: the decoders of a session with max_blocks <= 8 and the flooding schedule run on the edge-parallel engine, which has no weakest-VN select: make the session with max_blocks > 8 or the horizontal-layered schedule");
        return QLDPC_EUNSUPPORTED;
    }
    recon_call c = call_bob(n, key_words, key_bits, qber, msgs, parity_words, status, corrected, iterations);
    c.guess = guess; c.guess_bits = guess_bits;
    if (tagged)
        if (int rc = call_take_tags(who, c, n_keys, hash_keys, tag_words)) return rc;
    std::vector<char> skip((size_t)n, 0);
    for (int i = 0; i < n; i++) {
        if (int rc = bob_block_begin(r, c, i, nullptr, &skip[(size_t)i])) return rc;
        if (guess) { const qldpc_recon_guess none = {0, -1, 0, 0, 0, 0}; guess[i] = none; }
    }
    return run_call(r, c, skip);
}

extern "C" int qldpc_recon_decode_guess(qldpc_recon *r, int n, uint32_t *const *key_words, const int *key_bits, const float *qber, const qldpc_recon_msg *msgs,
                                        const uint32_t *const *parity_words, int guess_bits, qldpc_recon_guess *guess, int *status, int *corrected, int *iterations)
{
    return decode_guess_call("recon_decode_guess", false, r, n, key_words, key_bits, qber, msgs, parity_words, guess_bits, guess, 0, nullptr, nullptr, status, corrected, iterations);
}

/*
 * qldpc_recon_decode_guess with the keyed tag of every block that ends QLDPC_OK: a block decoded at once gets its tag from rk_verify_tag, a rescued
 * block the tag of the winner's key from rk_tag (guess_drain), a block still failed zeros.  The refusals are those of qldpc_recon_decode_guess, then
 * those of the tag arguments.
 */
extern "C" int qldpc_recon_decode_guess_tagged(qldpc_recon *r, int n, uint32_t *const *key_words, const int *key_bits, const float *qber, const qldpc_recon_msg *msgs,
                                               const uint32_t *const *parity_words, int guess_bits, qldpc_recon_guess *guess, int n_keys,
                                               const uint32_t *const *hash_keys, uint32_t *const *tag_words, int *status, int *corrected, int *iterations)
{
    return decode_guess_call("recon_decode_guess_tagged", true, r, n, key_words, key_bits, qber, msgs, parity_words, guess_bits, guess, n_keys, hash_keys, tag_words,
                             status, corrected, iterations);
}

/* the staging block of qldpc_recon_tag_blocks, pinned and on the device, of at least `words` words */
static int tag_stage_reserve(qldpc_recon *r, size_t words)
{
    if (r->tag_words >= words) return QLDPC_OK;
    dm_release(&r->tag_mem, &r->d_tag);
    dm_release(&r->tag_mem, &r->h_tag);
    r->tag_words = 0;
    if (dm_alloc_pinned(&r->tag_mem, &r->h_tag, words) || dm_alloc(&r->tag_mem, &r->d_tag, words)) {
        dm_release(&r->tag_mem, &r->h_tag);
        qldpc_set_error("recon_tag_blocks: staging of %zu words could not be allocated", words);
        return QLDPC_ENOMEM;
    }
    r->tag_words = words;
    return QLDPC_OK;
}

/*
 * The tags of host keys, for either side (Alice: her keys, once Bob's hash key has arrived): only a block's length matters, there is no plan and no
 * message.  The keys go through the session's tag staging block (recon_tag_layout) in launches of at most max_blocks rows of rk_tag on the first
 * lane's stream; the rows of a launch are as wide as the longest key of the call.
 */
extern "C" int qldpc_recon_tag_blocks(qldpc_recon *r, int n, const uint32_t *const *key_words, const int *key_bits, int n_keys, const uint32_t *const *hash_keys,
                                      uint32_t *const *tag_words)
{
    if (!r || !key_words || !key_bits || !hash_keys || !tag_words || n <= 0) return QLDPC_EINVAL;
    if (n_keys < 1 || n_keys > RT_MAX_KEYS) { qldpc_set_error("recon_tag_blocks: n_keys = %d, outside 1 .. %d", n_keys, RT_MAX_KEYS); return QLDPC_EINVAL; }
    int W = 1;
    bool shared = true;
    for (int i = 0; i < n; i++) {
        if (!key_words[i] || !hash_keys[i] || !tag_words[i]) { qldpc_set_error("recon_tag_blocks: block %d has no %s row", i, !key_words[i] ? "key" : !hash_keys[i] ? "hash-key" : "tag"); return QLDPC_EINVAL; }
        if (key_bits[i] < 1 || key_bits[i] > RT_MAX_BITS) { qldpc_set_error("recon_tag_blocks: block %d has key_bits = %d, outside 1 .. %d", i, key_bits[i], RT_MAX_BITS); return QLDPC_ESIZE; }
        W = std::max(W, (key_bits[i] + 31) / 32);
        shared = shared && hash_keys[i] == hash_keys[0];
    }
    HIPCHK(hipSetDevice(r->cfg.device));
    const int B = r->cfg.max_blocks;
    const size_t row = 2 * (size_t)n_keys;
    if (int rc = tag_stage_reserve(r, recon_tag_layout(nullptr, std::min(n, B), W, n_keys).words)) return rc;
    hipStream_t s = r->lane[0].stream;
    for (int at = 0; at < n; at += B) {
        const int nb = std::min(B, n - at);
        const recon_tag_view h = recon_tag_layout(r->h_tag, nb, W, n_keys), d = recon_tag_layout(r->d_tag, nb, W, n_keys);
        for (int t = 0; t < nb; t++) {
            const int i = at + t;
            memcpy(h.keys + (size_t)t * W, key_words[i], sizeof(uint32_t) * (size_t)((key_bits[i] + 31) / 32));      /* rk_tag reads no word past a block's length */
            h.key_bits[t] = key_bits[i];
            if (!shared || t == 0) memcpy(h.hash_keys + (size_t)t * row, hash_keys[i], sizeof(uint32_t) * row);
        }
        const size_t in_words = (size_t)(h.tags - h.keys);
        hipError_t he = hipMemcpyAsync(r->d_tag, r->h_tag, sizeof(uint32_t) * in_words, hipMemcpyHostToDevice, s);
        if (he == hipSuccess) {
            rk_tag_launch(n_keys, nb, s, d.keys, d.key_bits, nullptr, d.hash_keys, shared ? 0 : row, d.tags, W);
            he = hipGetLastError();
        }
        if (he == hipSuccess) he = hipMemcpyAsync(h.tags, d.tags, sizeof(uint32_t) * (size_t)nb * row, hipMemcpyDeviceToHost, s);
        const hipError_t hs = hipStreamSynchronize(s);      /* the pinned block is written again by the next launch */
        if (he == hipSuccess) he = hs;
        if (he != hipSuccess) { qldpc_set_error("recon_tag_blocks: %s", hipGetErrorString(he)); return QLDPC_EHIP; }
        for (int t = 0; t < nb; t++) memcpy(tag_words[at + t], h.tags + (size_t)t * row, sizeof(uint32_t) * row);
    }
    return QLDPC_OK;
}

/* the verdict kernel alone over rows that lie on the device (rk_verify_tag), what a tagged job queues after its decode: synthetic rows can be verified without a decode */
extern "C" int qldpc_recon_verify_tag_dev(int n, int n_keys, int Wk, int Wn, const uint32_t *d_out_rows, const uint32_t *d_keys, const int *d_key_bits,
                                          const uint32_t *d_crc_want, const int *d_ok, const int *d_iters, const uint32_t *d_hash_keys, size_t hash_key_stride,
                                          uint32_t *d_res_keys, int *d_res, uint32_t *d_tags, void *hip_stream)
{
    if (!d_out_rows || !d_keys || !d_key_bits || !d_crc_want || !d_ok || !d_iters || !d_hash_keys || !d_res_keys || !d_res || !d_tags) return QLDPC_EINVAL;
    if (n_keys < 1 || n_keys > RT_MAX_KEYS) { qldpc_set_error("recon_verify_tag: n_keys=%d, outside 1 .. %d", n_keys, RT_MAX_KEYS); return QLDPC_EINVAL; }
    if (n < 0 || Wk < 1 || Wn < Wk || (hash_key_stride && hash_key_stride < 2 * (size_t)n_keys)) {
        qldpc_set_error("recon_verify_tag: n=%d (not negative), key row of %d words (at least 1) in decoded rows of %d, hash-key rows %zu words apart (0 or at least %d)",
                        n, Wk, Wn, hash_key_stride, 2 * n_keys);
        return QLDPC_ESIZE;
    }
    if (n == 0) return QLDPC_OK;
    rk_verify_tag_launch(n_keys, n, (hipStream_t)hip_stream, d_out_rows, d_keys, d_key_bits, d_crc_want, d_ok, d_iters, d_hash_keys, hash_key_stride, d_res_keys, d_res,
                         d_tags, Wk, Wn);
    HIPCHK(hipGetLastError());
    return QLDPC_OK;
}

/* the verdict over trial rows that lie on the device (rk_guess_crc + rk_guess_settle), what guess_drain queues per trial launch: synthetic rows can be settled without a decode */
extern "C" int qldpc_recon_guess_settle_dev(int g, int n_src, int Wk, int Wn, const uint32_t *d_trial_rows, const int *d_ok, const int *d_iters, const uint32_t *d_keys,
                                            const int *d_key_bits, const uint32_t *d_crc_want, const int *d_first_iters, int *d_pass_out, uint32_t *d_crc_out,
                                            uint32_t *d_res_keys, int *d_res, int *d_guess, void *hip_stream)
{
    if (!d_trial_rows || !d_ok || !d_iters || !d_keys || !d_key_bits || !d_crc_want || !d_first_iters || !d_pass_out || !d_crc_out || !d_res_keys || !d_res || !d_guess)
        return QLDPC_EINVAL;
    if (g < 0 || g > GS_MAX_BITS || n_src < 0 || Wk < 1 || Wn < Wk || ((uint64_t)n_src << g) > GS_MAX_SLOTS) {
        qldpc_set_error("recon_guess_settle: guess bits=%d (0 .. %d), n_src=%d (not negative, n_src 2^g <= %u), key row of %d words (at least 1) in trial rows of %d",
                        g, GS_MAX_BITS, n_src, GS_MAX_SLOTS, Wk, Wn);
        return QLDPC_ESIZE;
    }
    if (n_src == 0) return QLDPC_OK;
    hipStream_t s = (hipStream_t)hip_stream;
    hipLaunchKernelGGL(rk_guess_crc, dim3((unsigned)n_src, 1u << g), dim3(RK_LANES), 0, s, d_trial_rows, d_ok, d_key_bits, d_crc_want, d_pass_out, d_crc_out, Wk, Wn);
    hipLaunchKernelGGL(rk_guess_settle, dim3((unsigned)n_src), dim3(RK_LANES), 0, s, d_trial_rows, d_ok, d_pass_out, d_crc_out, d_iters, d_keys, d_key_bits, d_first_iters,
                       d_res_keys, d_res, n_src, d_guess, Wk, Wn, g);
    HIPCHK(hipGetLastError());
    return QLDPC_OK;
}

/* n blocks of ONE length, contiguous arrays (the config-3 stream driver's call); parity_words rows are ceil(code_m / 32) words apart */
extern "C" int qldpc_recon_decode_batch(qldpc_recon *r, int n, uint32_t *key_words, int key_bits, const float *qber, const qldpc_recon_msg *msgs,
                                        const uint32_t *parity_words, int *status, int *corrected, int *iterations)
{
    if (!r || !key_words || !qber || !msgs || !parity_words || !status || n <= 0) return QLDPC_EINVAL;
    for (int i = 0; i < n; i++)
        if (msgs[i].code_k != msgs[0].code_k || msgs[i].code_m != msgs[0].code_m) { qldpc_set_error("recon_decode_batch: block %d has a different code", i); return QLDPC_ESIZE; }
    const int Wkey = (key_bits + 31) / 32, Wm = ((int)msgs[0].code_m + 31) / 32;
    std::vector<uint32_t *> k((size_t)n);
    std::vector<const uint32_t *> p((size_t)n);
    std::vector<int> kb((size_t)n, key_bits);
    for (int i = 0; i < n; i++) { k[(size_t)i] = key_words + (size_t)i * Wkey; p[(size_t)i] = parity_words + (size_t)i * Wm; }
    return qldpc_recon_decode_blocks(r, n, k.data(), kb.data(), qber, msgs, p.data(), status, corrected, iterations);
}

extern "C" int qldpc_recon_decode(qldpc_recon *r, uint32_t *key_words, int key_bits, float qber, const qldpc_recon_msg *msg, const uint32_t *parity_words,
                                  int *corrected, int *leaked, int *iterations)
{
    if (!r || !msg) return QLDPC_EINVAL;
    int status = QLDPC_EDECODE, corr = 0, it = 0;
    int rc = qldpc_recon_decode_batch(r, 1, key_words, key_bits, &qber, msg, parity_words, &status, &corr, &it);
    if (rc) return rc;
    if (corrected) *corrected = corr;
    if (iterations) *iterations = it;
    if (leaked) *leaked = qldpc_recon_leaked_bits(msg);      /* disclosed parity bits + the CRC */
    if (status == QLDPC_EDECODE) qldpc_set_error("recon_decode: no verified codeword after %d iterations", it);
    return status;
}
