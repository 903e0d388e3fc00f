// ia_synth.hip — per-level B' synthesis on device.
//
// The reference visits B' pixels in scanline order (image_analogies.py:161-162) and each
// query reads only causal B' samples: rows y-2, y-1 (cols x-2..x+2) and row y (cols
// x-2, x-1) of the fine level through symmetric padding, plus s/im of the same causal
// window for coherence.  Every such sample (including reflected border samples, which
// stay inside rows y-2..y+1 and cols x-2..x+2) satisfies: written before q in scanline
// order  <=>  its wave index x' + 3y' < x + 3y.  So processing the skewed wavefronts
// t = x + 3y in increasing t, each wave fully in parallel, reads exactly the values the
// scanline loop reads (DESIGN.md gives the case analysis; tests/test_oracle.py checks it
// exhaustively for small H, W).  Per wave:
//   k_query_wave  -> q64 / qp / q16 / nq        (ia_features.hip)
//   k_screen16    -> segment minima             (ia_screen16.hip, split-f16 MFMA)
//   k_rescore or k_select/k_items/k_gather -> the exact winner (ia_match.hip, fp64);
//                    on one GPU the same kernel runs the per-pixel tail (ia_finish.h)
//   sharded DB: RCCL all-gather of the per-rank winners, then
//   k_finish      -> coherence, kappa test, B'/s/im update (this file)
#include "ia_finish.h"
#include "ia_split16.h"
#include "ia_rot16.h"
#include "ia_pipe.h"
#include "../../include/ia_diag.h"

#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <vector>

#include <rccl/rccl.h>

namespace ia {

// Sticky schedule-error word of this device: every level's done() folds its fused kernel's
// error word (a neighbour-decision wait that timed out) into it on the level's stream, so
// callers that skip the per-call ia_synth_status (bench.py's timed steps) check once at the
// end with ia_sched_status.  Vector stores only.
__device__ unsigned int g_sched_err;

__global__ __launch_bounds__(64) void k_err_sticky(const unsigned int *__restrict__ ctl,
                                                   const XJob *__restrict__ jt, int K) {
    for (int k = threadIdx.x; k < K; k += 64) {
        const unsigned int e = jt ? jt[k].ctl[2] : ctl[2];
        if (e) g_sched_err = 1u;
    }
}

// Sharded DB, after the cross-rank exchange: one wave per query pixel takes the
// lexicographic (distance, row) minimum over the ranks' ShardRec (lane g = rank g), whose
// weighted distance the owning rank already computed, and finishes the pixel with the
// coherence pick its own exact stage stored (every rank holds the same replicated state,
// so the picks agree; ia_finish.h).  No feature gathers here.
__global__ __launch_bounds__(64) void k_finish(DbSrc src, const ShardRec *__restrict__ rec_all,
                                               const CohSel *__restrict__ coh, int nranks, int M,
                                               FinishArgs f) {
    const int m = blockIdx.x;
    const int lane = threadIdx.x;
    double d = INFINITY, wd = 0.0;
    long long idx = 0x7fffffffffffffffLL;
    for (int g = lane; g < nranks; g += 64) {
        const ShardRec r = rec_all[(long)g * M + m];
        if (r.d < d || (r.d == d && r.idx < idx)) { d = r.d; idx = r.idx; wd = r.wd; }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double od = __shfl_xor(d, o), owd = __shfl_xor(wd, o);
        const long long oi = __shfl_xor(idx, o);
        if (od < d || (od == d && oi < idx)) { d = od; idx = oi; wd = owd; }
    }
    finish_apply(src, idx, m, f, coh[m], wd, lane);
}

// Sharded DB, the other tail form (IA_SHARD_TAIL=0): the exact stage writes only its
// shard's (distance, row); after the exchange wave 1 picks the coherence candidate while
// wave 0 reduces the ranks' winners and weighs the global one, then finishes the pixel
__global__ __launch_bounds__(128) void k_finish_gather(DbSrc src, const Best *__restrict__ best_all,
                                                       int nranks, int M, FinishArgs f,
                                                       const double *__restrict__ q64) {
    __shared__ double qs[IA_DP];
    __shared__ CohSel cs;
    const int m = blockIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    // the query and (wave 0) the first 8 ranks' winners in one memory round trip
    const double qv = threadIdx.x < IA_DP ? q64[(long)m * IA_DP + threadIdx.x] : 0.0;
    constexpr int NB0 = 8;
    Best b0[NB0];
    if (wv == 0) {
#pragma unroll
        for (int g = 0; g < NB0; ++g)
            b0[g] = g < nranks ? best_all[(long)g * M + m] : Best{INFINITY, 0x7fffffffffffffffLL};
    }
    if (threadIdx.x < IA_DP) qs[threadIdx.x] = qv;
    __syncthreads();
    double ad = INFINITY;
    long long app = 0x7fffffffffffffffLL;
    if (wv == 1) {
        const CohSel c = coh_pick(src, m, f, qs, lane);
        if (lane == 0) cs = c;
    } else {
#pragma unroll
        for (int g = 0; g < NB0; ++g) fin_best(ad, app, b0[g].d, b0[g].idx);
        for (int g = NB0; g < nranks; ++g) {
            const Best b = best_all[(long)g * M + m];
            fin_best(ad, app, b.d, b.idx);
        }
    }
    const double d_app = wv == 0 ? app_wdist(src, app, f, qs, lane) : 0.0;
    __syncthreads();
    if (wv == 0) finish_apply(src, app, m, f, cs, d_app, lane);
}

// Sharded DB over the device-side exchange: the exact stage published this shard's winner
// (k_rescore<3> / k_gather<3>, which also left it in best[m]); wave 0 collects every
// rank's from this rank's receive box and weighs the global winner while wave 1 picks the
// coherence candidate, then wave 0 finishes the pixel.  The waits live in these small
// 2-wave workgroups, not in the exact stage's 4-wave, 250-VGPR ones: ranks sharing a GPU,
// or a rank's other streams, keep room to run the kernels the waits depend on (the fused
// form deadlocked two ranks on one GPU).  On timeout the shard's own winner.
__global__ __launch_bounds__(128) void k_peer_finish(DbSrc src, const Best *__restrict__ best,
                                                     FinishArgs f, const double *__restrict__ q64) {
    __shared__ double qs[IA_DP];
    __shared__ CohSel cs;
    const int m = blockIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const double qv = threadIdx.x < IA_DP ? q64[(long)m * IA_DP + threadIdx.x] : 0.0;
    const Best own = best[m];
    if (threadIdx.x < IA_DP) qs[threadIdx.x] = qv;
    __syncthreads();
    double gd = own.d;
    long long gw = own.idx;
    if (wv == 1) {
        const CohSel c = coh_pick(src, m, f, qs, lane);
        if (lane == 0) cs = c;
    } else {
        const bool tron = f.px.trace && m < 8 && f.px.epoch < 1024;
        unsigned long long *tr = tron ? reinterpret_cast<unsigned long long *>(f.px.trace.get()) +
                                            ((long)f.px.epoch * 8 + m) * 12
                                      : nullptr;
        peer_collect(f.px, m, lane, gd, gw, tr ? tr + 4 : nullptr);
        if (tr && lane == 0) {
            tr[0] = __double_as_longlong(own.d); tr[1] = own.idx;
            tr[2] = __double_as_longlong(gd); tr[3] = gw;
        }
    }
    const double d_app = wv == 0 ? app_wdist(src, gw, f, qs, lane) : 0.0;
    __syncthreads();
    if (wv == 0) finish_apply(src, gw, m, f, cs, d_app, lane);
}

// LSH matcher (one shard): wave 1 picks the coherence candidate while wave 0 weighs the
// LSH winner, then wave 0 finishes the pixel (ia_finish.h)
__global__ __launch_bounds__(128) void k_lsh_tail(DbSrc src, const Best *__restrict__ best, int M,
                                                  FinishArgs f, const double *__restrict__ q64) {
    __shared__ double qs[IA_DP];
    __shared__ CohSel cs;
    const int m = blockIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (threadIdx.x < IA_DP) qs[threadIdx.x] = q64[(long)m * IA_DP + threadIdx.x];
    __syncthreads();
    const long long app = best[m].idx;
    if (wv == 1) {
        const CohSel c = coh_pick(src, m, f, qs, lane);
        if (lane == 0) cs = c;
    }
    const double d_app = wv == 0 ? app_wdist(src, app, f, qs, lane) : 0.0;
    __syncthreads();
    if (wv == 0) finish_apply(src, app, m, f, cs, d_app, lane);
}

// k_lsh_tail for a batch of K LSH jobs (ia_synth_levels_lsh_batch): the job is blockIdx.y,
// its images, winners, query rows and level state come from the device job table; the wave's
// t and y_lo stay launch arguments.  (A copy: the single-job kernel keeps its instructions.)
__global__ __launch_bounds__(128) void k_lsh_tail_b(const LJob *__restrict__ jobs, int t, int y_lo) {
    __shared__ double qs[IA_DP];
    __shared__ CohSel cs;
    const LJob &J = jobs[blockIdx.y];
    const DbSrc src = J.src();
    const FinishArgs f = J.finish(t, y_lo);
    const int m = blockIdx.x;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (threadIdx.x < IA_DP) qs[threadIdx.x] = J.q64.p[(long)m * IA_DP + threadIdx.x];
    __syncthreads();
    const long long app = J.best.p[m].idx;
    if (wv == 1) {
        const CohSel c = coh_pick(src, m, f, qs, lane);
        if (lane == 0) cs = c;
    }
    const double d_app = wv == 0 ? app_wdist(src, app, f, qs, lane) : 0.0;
    __syncthreads();
    if (wv == 0) finish_apply(src, app, m, f, cs, d_app, lane);
}

// -------------------------------- workspace ----------------------------------------
struct SynthWs {
    double *q64;
    float *qp;
    _Float16 *q16;
    double *nq;
    void *scratch;           // screen output (candidates or segment minima)
    Best *best_local;
    ShardRec *rec_local;     // sharded DB: this rank's records, then all ranks'
    ShardRec *rec_all;
    CohSel *coh;
    unsigned long long *stats;
    // the fused per-wave kernel (k_xwave): the query rows of odd waves (even waves use
    // q64 / qp / q16 / nq), the decision granules (2 per row) and the control words
    // {tickets[2], error}
    double *q64b;
    float *qpb;
    _Float16 *q16b;
    double *nqb;
    unsigned long long *dbox;
    unsigned int *ctl;
    XJob *jtab;              // a batch's job table, then its DB group table (ia_synth_levels_batch, job 0's workspace)
    unsigned long long *xbox;   // split candidates: the helpers' records, 8 granules per row
};
constexpr int XW_CTL_ERR = 2;

static size_t carve(SynthWs *ws, char *base, int H, int W, long nrows, int nranks) {
    const int Mmax = wave_max_queries(H, W);
    const int qr = qrows_alloc(Mmax);
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += align_up(bytes, 256); return base ? base + o : nullptr; };
    SynthWs w;
    w.q64 = (double *)take((size_t)Mmax * IA_DP * sizeof(double));
    w.qp = (float *)take((size_t)qr * IA_DP * sizeof(float));
    w.q16 = (_Float16 *)take((size_t)qr * Q16_ROW * 16);
    w.nq = (double *)take((size_t)qr * sizeof(double));
    w.scratch = take(match_scratch_bytes(qr, nrows));
    w.best_local = (Best *)take((size_t)Mmax * sizeof(Best));
    w.rec_local = (ShardRec *)take((size_t)Mmax * sizeof(ShardRec));
    w.rec_all = (ShardRec *)take((size_t)Mmax * nranks * sizeof(ShardRec));
    w.coh = (CohSel *)take((size_t)Mmax * sizeof(CohSel));
    w.stats = (unsigned long long *)take(STATS_BYTES);
    w.q64b = (double *)take((size_t)Mmax * IA_DP * sizeof(double));
    w.qpb = (float *)take((size_t)qr * IA_DP * sizeof(float));
    w.q16b = (_Float16 *)take((size_t)qr * Q16_ROW * 16);
    w.nqb = (double *)take((size_t)qr * sizeof(double));
    w.dbox = (unsigned long long *)take((size_t)H * 2 * sizeof(unsigned long long));
    w.ctl = (unsigned int *)take(256);
    w.jtab = (XJob *)take((size_t)IA_BATCH_MAX * sizeof(XJob) + IA_GTAB_INTS * sizeof(int));
    w.xbox = (unsigned long long *)take((size_t)H * 8 * sizeof(unsigned long long));
    if (ws) *ws = w;
    return off;
}

// executable graphs stay alive until their launch has completed (destroyed lazily at the
// next capture, after an event wait; ia_release_thread_resources frees them)
struct GraphKeeper {
    hipStream_t cap = nullptr;
    hipGraphExec_t exec = nullptr;
    hipEvent_t done = nullptr;
    hipError_t retire() {
        if (!exec) return hipSuccess;
        hipError_t e = hipEventSynchronize(done);
        if (e == hipSuccess) e = hipGraphExecDestroy(exec);
        exec = nullptr;
        return e;
    }
    hipError_t hold(hipGraphExec_t x, hipStream_t st) {
        exec = x;
        if (!done) {
            hipError_t e = hipEventCreateWithFlags(&done, hipEventDisableTiming);
            if (e != hipSuccess) return e;
        }
        return hipEventRecord(done, st);
    }
};
static thread_local GraphKeeper g_graphs;

// ---- profiling (IA_SYNTH_PROF): HIP events around every screen launch and the matcher
// statistics, collected WITHOUT synchronising: events come from a process-wide pool and
// the statistics are copied stream-ordered into pinned host memory; ia_prof_end()
// synchronises once and reads everything back.  So a profiled level runs the same
// launches with no host round trip (bench.py profiles its timed steps this way).
struct ProfRec {
    int tag;
    int jobs;                // jobs batched into each launch
    long nrows;
    double pairs;
    size_t ev0;
    int nscreen, timed;
    unsigned long long *hstats;
    std::vector<int> M;      // queries of each screen launch, in launch order
};
struct ProfCollector {
    std::mutex mu;
    bool active = false;
    std::vector<hipEvent_t> ev;
    size_t next = 0;
    std::vector<ProfRec> recs;
    std::vector<unsigned long long *> pinned;
    size_t pinned_next = 0;
};
// never destroyed: the HIP runtime may be torn down before static destructors run
static ProfCollector *const g_prof = new ProfCollector;

static bool prof_active() {
    std::lock_guard<std::mutex> l(g_prof->mu);
    return g_prof->active;
}

// events [*ev0, *ev0 + nev) and one pinned statistics buffer for one level call
static int prof_reserve(size_t nev, size_t *ev0, unsigned long long **hstats) {
    std::lock_guard<std::mutex> l(g_prof->mu);
    while (g_prof->ev.size() < g_prof->next + nev) {
        hipEvent_t e;
        IA_HIP(hipEventCreate(&e));
        g_prof->ev.push_back(e);
    }
    *ev0 = g_prof->next;
    g_prof->next += nev;
    if (g_prof->pinned_next == g_prof->pinned.size()) {
        void *p = nullptr;
        IA_HIP(hipHostMalloc(&p, STATS_BYTES, hipHostMallocDefault));
        g_prof->pinned.push_back(reinterpret_cast<unsigned long long *>(p));
    }
    *hstats = g_prof->pinned[g_prof->pinned_next++];
    return IA_OK;
}

static hipEvent_t prof_event(size_t i) {
    std::lock_guard<std::mutex> l(g_prof->mu);
    return g_prof->ev[i];
}

static void prof_push(const ProfRec &r) {
    std::lock_guard<std::mutex> l(g_prof->mu);
    g_prof->recs.push_back(r);
}

// measured (tools/level_times.py, profiles/r01_level_times_graph.txt): eager launches beat
// a captured graph on every c4 level once instantiation is counted, so capture is opt-in
// (settable through ia_diag_set_graph_mode)
static std::atomic<int> g_graph_mode{env_int("IA_GRAPH", 0)};
static int graph_mode() { return g_graph_mode.load(std::memory_order_relaxed); }

// the compact screen's level threshold (rows; DESIGN.md §4d: c4's finest level pays, measured);
// LONG_MAX: off (ia_diag_set_compact_min_rows)
static std::atomic<long> g_compact_min_rows{1L << 22};
static long compact_min_rows() { return g_compact_min_rows.load(std::memory_order_relaxed); }
// compact waves enqueued by this process (ia_diag_compact_waves: the tests' proof that the form ran)
static std::atomic<long> g_compact_waves{0};
// the column-0 waves (wave_compact_col) of a level whose basis keeps the own-row axes run compact
// too (ia_diag_set_compact_col; IA_COMPACT_COL: the process's initial value, default on)
static std::atomic<int> g_compact_col{env_int("IA_COMPACT_COL", 1) != 0};
static bool compact_col() { return g_compact_col.load(std::memory_order_relaxed) != 0; }
// the split tail's level threshold (rows; DESIGN.md §6b "split": a pixel's candidate segments over
// two workgroups of k_xstrip); LONG_MAX: off (ia_diag_set_xsplit_min_rows).  2^22 rows, as the
// compact form: c4's finest level, 1.5-1.7 % of the step on two boxes; 2^20 measured no better
// (profiles/xsplit_ab.txt).  IA_XSPLIT_MIN_ROWS: the process's initial threshold (0: off)
static long xsplit_initial() {
    const int v = env_int("IA_XSPLIT_MIN_ROWS", 1 << 22);
    return v > 0 ? v : LONG_MAX;
}
static std::atomic<long> g_xsplit_min_rows{xsplit_initial()};
static long xsplit_min_rows() { return g_xsplit_min_rows.load(std::memory_order_relaxed); }
// workgroups of the fused kernel's launch for R pixel rows: two per pixel where the split applies
// (eligible: one unsharded job's strip-form R16 level), else one
static int xsplit_grid(bool eligible, long nrows, int R) {
    return eligible && nrows >= xsplit_min_rows() && db_nsegs(nrows) <= (1L << 20) ? 2 * R : R;
}

// IA_SHARED_SCREEN (ia_diag_set_shared_screen): 1 a batch whose jobs share rotated databases
// screens them in one k_screen16rs launch per wave, 0 every job through the K-job k_screen16r
static std::atomic<int> g_shared_screen{env_int("IA_SHARED_SCREEN", 1) != 0};
// waves whose screen was k_screen16rs (ia_diag_shared_screen_waves)
static std::atomic<long> g_shared_waves{0};

// a job's database: its rotated rows where it has them, else the image form, else the rows
static const void *job_db(const IaSynthArgs &a) { return a.dbr ? a.dbr : a.dbi ? a.dbi : a.db; }
// the DB groups of one level's K jobs (ia_batch_groups): jobs passing the same non-null database
// form a group, numbered in order of first appearance; returns their number
static int batch_groups(const IaSynthArgs *jobs, int K, int *group_of_job) {
    int G = 0, first[IA_BATCH_MAX];
    for (int k = 0; k < K; ++k) {
        int g = 0;
        while (g < G && !(job_db(jobs[k]) && job_db(jobs[first[g]]) == job_db(jobs[k]))) ++g;
        if (g == G) first[G++] = k;
        group_of_job[k] = g;
    }
    return G;
}

int screen16_attributes(bool img, hipFuncAttributes *at);
int screen_resources_r16(hipFuncAttributes *at);
int comm_allgather(void *comm, const void *send, void *recv, size_t bytes, hipStream_t st);
int comm_nranks(void *comm);
PeerView comm_peer_wave(void *comm);
int comm_peer_mcap(void *comm);

// sharded tail form (IA_SHARD_TAIL): 0 [default] the exchange carries (distance, row) and
// k_finish_gather does the coherence pick and the weighting after it; 1 the exact stage
// prepares the tail (ShardRec, CohSel) and k_finish only reduces.  Measured on the
// simulated G = 8 rank (`tools/gpu.sh abknob ... -- python tools/shard_sim.py 8`, one box): finest level 335 vs 361 ms, pipelined
// step 415 vs 450 ms, so 0
static int shard_tail() {
    static const int v = env_int("IA_SHARD_TAIL", 0);
    return v;
}

// the fused per-wave kernel (k_xwave, ia_xwave.hip): after each screen ONE launch runs the
// exact stage, the device-side exchange, the per-pixel tail and the next wave's query rows
// (IA_XWAVE / ia_diag_set_xwave: 2 [default] wherever it applies, with k_xstrip on
// strip-order image-form levels; 1 k_xwave only; 0 the separate kernels)
static std::atomic<int> g_xwave{env_int("IA_XWAVE", 2)};
static int xwave_on() { return g_xwave.load(std::memory_order_relaxed); }

// diagnostic: k_xwave phase stamps of the level tagged IA_XW_TRACE (one process-wide buffer)
static unsigned long long *g_xw_trace = nullptr;
static unsigned long long *xw_trace(int tag) {
    static const int want = env_int("IA_XW_TRACE", -1);
    if (want < 0 || tag != want) return nullptr;
    if (!g_xw_trace) {
        const size_t n = (size_t)XW_TRACE_T * XW_TRACE_PX * XW_TRACE_N * sizeof(unsigned long long);
        if (hipMalloc(&g_xw_trace, n) != hipSuccess) { g_xw_trace = nullptr; return nullptr; }
        (void)hipMemset(g_xw_trace, 0, n);
    }
    return g_xw_trace;
}

bool compact_level(const DbSrc &src, const StageMap &sm, long nrows) {
    return sm.W > 0 && xstrip_applies(src) && nrows >= compact_min_rows();
}

// The one place a level's launch forms are decided (ia_internal.h LevelPlan).
// K: the jobs sharing the level's launches; sim: the in-process shard simulation.
int level_plan(const IaSynthArgs &a, int K, bool sim, LevelPlan *p) {
    LevelPlan &l = *p;
    l = LevelPlan{};
    l.form = -1;
    IA_SRC_NA(a.src, "ia_synth_level");
    l.pairs = src_pairs(a.src);
    l.nranks = comm_nranks(a.comm);
    // the device-side exchange: the exact stage (or the fused kernel) publishes, no RCCL call
    l.peer = a.comm && comm_peer_mcap(a.comm) > 0;
    l.tail = sim ? TAIL_SIM : a.lsh ? TAIL_LSH : l.peer ? TAIL_PEER
           : a.comm ? (shard_tail() ? TAIL_REC : TAIL_GATHER) : TAIL_FUSED;
    l.fused = l.tail == TAIL_FUSED;
    // one launch per wave after the screen wherever the exact matcher runs on one GPU or over
    // the device-side exchange (not the LSH matcher, RCCL, the simulation or a forced work list)
    const int xwave = xwave_on();
    l.xw = xwave && !a.lsh && !sim && (!a.comm || l.peer) && exact_stage_mode() != 1;
    l.r16 = l.xw && a.dbr && a.rot;   // (either form of the fused kernel takes the R16 bound)
    if (a.lsh || sim) return IA_OK;
    const DbSrc src = make_dbsrc(a.src);
    const int rc = db_view(src, a.row0, a.nrows, a.db, a.dbi, &l.v);
    if (rc || !l.xw) return rc;
    l.form = !l.v.im ? XW_ROWS : (xwave == 2 && l.v.sm.W > 0 && xstrip_applies(src)) ? XW_STRIP : XW_IMG;
    // compact waves (ia_rot16.h RK_*) and split candidates: one unsharded job's strip-form R16
    // level, above each one's row threshold
    const bool one = l.r16 && K == 1 && !a.comm && l.form == XW_STRIP;
    l.rk = one && a.dbk && compact_level(src, l.v.sm, a.nrows);
    l.rkcol = l.rk && a.rot_axes == RK_NAXES && compact_col();
    l.split = xsplit_grid(one, a.nrows, 1) == 2;
    return IA_OK;
}

static int check_args(const IaSynthArgs *a) {
    IA_ARG(a && (a->db || a->dbi || a->lsh) && a->center && a->amax && a->B_sm && a->B_lg && a->Bp_sm && a->Bp_lg &&
               a->weights && a->s && a->im && a->workspace,
           "ia_synth_level: null argument");
    IA_ARG(a->H > 0 && a->W > 0 && a->nrows > 0 && a->row0 >= 0 &&
               a->row0 + a->nrows <= a->N_total,
           "ia_synth_level: bad sizes");
    IA_ARG(a->N_total == (long)a->src.nAp * a->src.Ah * a->src.Aw, "ia_synth_level: N_total mismatch");
    IA_ARG(a->B_hs == (a->H + 1) / 2 && a->B_ws == (a->W + 1) / 2, "ia_synth_level: B level shapes");
    IA_ARG(a->src.A_hs == (a->src.Ah + 1) / 2 && a->src.A_ws == (a->src.Aw + 1) / 2,
           "ia_synth_level: A level shapes");
    IA_ARG(!a->dbg_px == !a->dbg_dist, "ia_synth_level: debug outputs come in pairs");
    IA_ARG(comm_nranks(a->comm) >= 1, "ia_synth_level: bad communicator");
    IA_ARG(!(a->lsh && a->comm), "ia_synth_level: the LSH matcher runs unsharded (comm must be NULL)");
    return IA_OK;
}

// One level's synthesis state: init() on its stream, then wave(t) for t = 0..nw-1 in order
// (each enqueues that wave's launches), then done().
struct LevelRun {
    const IaSynthArgs *a = nullptr;
    const IaShardDb *sim = nullptr;   // diagnostic: nsim DB shards in this process
    int nsim = 0;
    SynthWs ws{};
    DbSrc src{};
    ImgPair B{}, Bp{};
    int H = 0, W = 0, nw = 0, nranks = 1;
    bool prof = false, timed = false;
    LevelPlan plan{};        // the level's launch forms, decided once (init)
    XArgs xa{};              // the fused kernel's arguments that no wave changes (plan.xw)
    // a batch of K identical-shape jobs (ia_synth_levels_batch): this run is job 0 and owns
    // the launches; part[k - 1] holds job k's state (member runs record no profile)
    int K = 1;
    bool member = false;
    std::vector<LevelRun> part;
    size_t ev0 = 0;
    unsigned long long *hstats = nullptr;
    double pairs = 0.0;
    int nscreen = 0;
    std::vector<int> Ms;

    int init(const IaSynthArgs *args, hipStream_t st, int njobs = 1) {
        a = args;
        K = njobs;
        int rc = check_args(a);
        if (rc || (rc = level_plan(*a, K, sim != nullptr, &plan))) return rc;
        nranks = sim ? nsim : plan.nranks;
        H = a->H; W = a->W;
        nw = wave_count(H, W);
        long rows_ws = a->nrows;
        for (int r = 0; r < nsim; ++r) rows_ws = sim[r].nrows > rows_ws ? sim[r].nrows : rows_ws;
        carve(&ws, reinterpret_cast<char *>(a->workspace), H, W, rows_ws, nranks);
        const int Mmax = wave_max_queries(H, W);
        IA_HIP(hipMemsetAsync(ws.qp, 0, (size_t)qrows_alloc(Mmax) * IA_DP * sizeof(float), st));
        IA_HIP(hipMemsetAsync(ws.q16, 0, (size_t)qrows_alloc(Mmax) * Q16_ROW * 16, st));
        IA_HIP(hipMemsetAsync(ws.stats, 0, STATS_BYTES, st));
        IA_HIP(hipMemsetAsync(ws.scratch, 0, 256, st));   // the exact stage's empty work list
        src = make_dbsrc(a->src);
        B = ImgPair{a->B_sm, a->B_lg, a->B_hs, a->B_ws, H, W};
        Bp = ImgPair{a->Bp_sm, a->Bp_lg, a->B_hs, a->B_ws, H, W};
        prof = !member && (a->flags & IA_SYNTH_PROF) && prof_active();
        timed = prof;
        if (prof && (rc = prof_reserve(3 * (size_t)nw, &ev0, &hstats))) return rc;
        IA_ARG(!plan.peer || comm_peer_mcap(a->comm) >= Mmax,
               "ia_synth_level: the peer exchange's box holds fewer queries than a wave");
        IA_ARG(!plan.peer || a->N_total < (1L << 32),
               "ia_synth_level: the peer exchange carries 32-bit rows (N_total >= 2^32)");
        IA_HIP(hipMemsetAsync(ws.ctl, 0, 256, st));   // tickets, error word (ia_synth_status)
        if (!plan.xw) return IA_OK;
        IA_HIP(hipMemsetAsync(ws.qpb, 0, (size_t)qrows_alloc(Mmax) * IA_DP * sizeof(float), st));
        IA_HIP(hipMemsetAsync(ws.q16b, 0, (size_t)qrows_alloc(Mmax) * Q16_ROW * 16, st));
        IA_HIP(hipMemsetAsync(ws.dbox, 0, (size_t)H * 2 * sizeof(unsigned long long), st));
        IA_HIP(hipMemsetAsync(ws.xbox, 0, (size_t)H * 8 * sizeof(unsigned long long), st));
        const DbView &v = plan.v;
        xa.src = src; xa.im = v.img; xa.db = v.db;
        xa.row0 = v.row0; xa.nrows = v.nrows; xa.nseg = v.nseg; xa.seg_rows = v.seg_rows; xa.smap = v.sm;
        xa.segmin = match_segmin(ws.scratch);
        xa.amax = a->amax; xa.center = a->center;
        xa.B = B; xa.Bp = Bp; xa.H = H;
        xa.dbox = ws.dbox; xa.tickets = ws.ctl; xa.err = ws.ctl + XW_CTL_ERR;
        xa.stats = prof ? ws.stats : nullptr;
        xa.f = finish_args(0, 0, nullptr, nullptr);
        xa.jobs = K > 1 ? ws.jtab : nullptr;
        xa.trace = xw_trace(a->tag);
        xa.rot = plan.r16 ? a->rot : nullptr;
        xa.askc = plan.r16 ? r16_askc(a->dbr, a->nrows) : nullptr;
        xa.rk = plan.rk ? 1 : 0;
        return IA_OK;
    }

    // wave t's view of the level state the per-pixel tail updates
    FinishArgs finish_args(int t, int y_lo, ShardRec *shard_out, CohSel *coh_out) const {
        return FinishArgs{t, y_lo, W, a->N_total, a->weights, a->kappa_factor, a->Bp_lg, a->s,
                          a->im, a->dbg_px, a->dbg_dist, shard_out, coh_out};
    }

    // this wave's profiling events (null unless timed): 0 / 1 bracket the screen, 2 follows the
    // exact stage (the unfused tails are not bracketed)
    hipEvent_t wave_event(int i) const { return timed ? prof_event(ev0 + 3 * nscreen + i) : nullptr; }
    // after wave t's exact stage: event 2, the profile's counts and the IA_SYNC_EVERY=n wait (every n
    // waves: bounds the dispatches in flight, rocprofv3 --pmc runs of the whole bench crash otherwise)
    int wave_counted(int t, int M, hipStream_t sq) {
        if (timed) IA_HIP(hipEventRecord(wave_event(2), sq));
        ++nscreen;
        pairs += (double)M * (double)a->nrows * K;
        if (prof) Ms.push_back(M);
        static const int sync_every = env_int("IA_SYNC_EVERY", 0);
        if (sync_every > 0 && t % sync_every == sync_every - 1) IA_HIP(hipStreamSynchronize(sq));
        return IA_OK;
    }

    int wave(int t, hipStream_t sq) {
        int y_lo, M;
        wave_rows(H, W, t, y_lo, M);
        if (M <= 0) return IA_OK;
        int rc;
        const int tail = plan.tail;
        if (tail == TAIL_SIM) return sim_wave(t, y_lo, M, sq);
        if (plan.xw) return xw_wave(t, y_lo, M, sq);
        if (lshb) return lsh_wave_batch(t, y_lo, M, sq);
        if ((rc = launch_query_wave(B, Bp, t, y_lo, M, a->center, ws.q64, ws.qp, ws.nq, a->amax,
                                    ws.q16, sq)))
            return rc;
        hipEvent_t e0 = wave_event(0), e1 = wave_event(1);
        FinishArgs fa = finish_args(t, y_lo, tail == TAIL_REC ? ws.rec_local : nullptr,
                                    tail == TAIL_REC ? ws.coh : nullptr);
        if (tail == TAIL_PEER) fa.px = comm_peer_wave(a->comm);
        if (tail == TAIL_LSH) {   // approximate matcher: the events bracket the LSH query kernel
            if (e0) IA_HIP(hipEventRecord(e0, sq));
            if ((rc = launch_lsh_match(a->lsh, src, a->row0, a->nrows, M, ws.q64, a->center,
                                       ws.best_local, prof ? ws.stats : nullptr, sq)))
                return rc;
            if (e1) IA_HIP(hipEventRecord(e1, sq));
        } else if ((rc = launch_match(src, a->row0, a->nrows, a->db, a->dbi, ws.qp, ws.q16, M, ws.q64, ws.nq,
                                      a->amax, ws.scratch, ws.best_local,
                                      prof ? ws.stats : nullptr, sq, e0, e1,
                                      tail == TAIL_GATHER ? nullptr : &fa))) {
            return rc;
        }
        if ((rc = wave_counted(t, M, sq))) return rc;
        switch (tail) {
        case TAIL_FUSED:    // the exact stage already ran the per-pixel tail
            return IA_OK;
        case TAIL_PEER:     // collect the ranks' winners, finish the pixel
            k_peer_finish<<<M, 128, 0, sq>>>(src, ws.best_local, fa, ws.q64);
            break;
        case TAIL_LSH:      // one shard, LSH winners
            k_lsh_tail<<<M, 128, 0, sq>>>(src, ws.best_local, M, fa, ws.q64);
            break;
        // sharded DB over RCCL (also with one rank: the same path, exercised by the tests): the
        // exchange of the ranks' winners, or of the records and coherence picks the exact stage
        // left, then the finish
        case TAIL_GATHER: {
            Best *all = reinterpret_cast<Best *>(ws.rec_all);
            if ((rc = comm_allgather(a->comm, ws.best_local, all, (size_t)M * sizeof(Best), sq)))
                return rc;
            k_finish_gather<<<M, 128, 0, sq>>>(src, all, nranks, M, fa, ws.q64);
            break;
        }
        default:
            if ((rc = comm_allgather(a->comm, ws.rec_local, ws.rec_all, (size_t)M * sizeof(ShardRec), sq)))
                return rc;
            k_finish<<<M, 64, 0, sq>>>(src, ws.rec_all, ws.coh, nranks, M, fa);
        }
        IA_LAUNCH_CHECK("the unfused tail");
        return IA_OK;
    }

    // ---- a batch of K > 1 LSH jobs (ia_synth_levels_lsh_batch, which has validated
    // args[0..nj)): this run is job 0; the LJob table takes the XJob table's place in its
    // workspace and is staged once per level through `pinned`
    bool lshb = false;
    LJob lsh_entry() const {
        LJob J{};
        J.A_sm = a->src.A_sm; J.A_lg = a->src.A_lg; J.Ap_sm = a->src.Ap_sm; J.Ap_lg = a->src.Ap_lg;
        J.A_hs = a->src.A_hs; J.A_ws = a->src.A_ws; J.Ah = a->src.Ah; J.Aw = a->src.Aw;
        J.pairs = src_pairs(a->src) ? 1 : 0;
        J.B_sm = a->B_sm; J.B_lg = a->B_lg; J.Bp_sm = a->Bp_sm; J.Bp_lg = a->Bp_lg;
        J.B_hs = a->B_hs; J.B_ws = a->B_ws; J.H = H; J.W = W;
        lsh_job_tables(a->lsh, a->nrows, &J);
        J.row0 = a->row0; J.nrows = a->nrows; J.N_total = a->N_total;
        J.center = a->center; J.q64 = ws.q64; J.best = ws.best_local;
        J.stats = prof ? ws.stats : nullptr;
        J.weights = a->weights; J.kappa_factor = a->kappa_factor;
        J.s = a->s; J.im = a->im; J.dbg_px = a->dbg_px; J.dbg_dist = a->dbg_dist;
        return J;
    }
    int init_lsh_batch(const IaSynthArgs *args, int nj, hipStream_t st, LJob *pinned) {
        int rc = init(&args[0], st, nj);
        if (rc) return rc;
        IA_ARG(plan.tail == TAIL_LSH && nj > 1 && nj <= IA_BATCH_MAX, "ia_synth_levels_lsh_batch: bad batch");
        lshb = true;
        part.resize(K - 1);
        pinned[0] = lsh_entry();
        for (int k = 1; k < K; ++k) {
            part[k - 1].member = true;
            if ((rc = part[k - 1].init(&args[k], st, K))) return rc;
            IA_ARG(part[k - 1].plan.tail == TAIL_LSH, "ia_synth_levels_lsh_batch: a job without lsh");
            pinned[k] = part[k - 1].lsh_entry();
        }
        IA_HIP(hipMemcpyAsync(ws.jtab, pinned, (size_t)K * sizeof(LJob), hipMemcpyHostToDevice, st));
        return IA_OK;
    }
    // wave t of an LSH batch: the single job's three launches with the job as a grid dimension
    // (the events bracket the LSH query kernel, as for one job)
    int lsh_wave_batch(int t, int y_lo, int M, hipStream_t sq) {
        const LJob *jt = reinterpret_cast<const LJob *>(ws.jtab);
        int rc;
        if ((rc = launch_query_wave_lsh_batch(jt, K, t, y_lo, M, sq))) return rc;
        hipEvent_t e0 = wave_event(0), e1 = wave_event(1);
        if (e0) IA_HIP(hipEventRecord(e0, sq));
        if ((rc = launch_lsh_match_batch(jt, K, M, sq))) return rc;
        if (e1) IA_HIP(hipEventRecord(e1, sq));
        if ((rc = wave_counted(t, M, sq))) return rc;
        k_lsh_tail_b<<<dim3(M, K), 128, 0, sq>>>(jt, t, y_lo);
        IA_LAUNCH_CHECK("k_lsh_tail_b");
        return IA_OK;
    }

    // job k's table entry (the batched launches read their pointers from it)
    XJob job_entry() const {
        XJob J{};
        J.A_sm = a->src.A_sm; J.A_lg = a->src.A_lg; J.Ap_sm = a->src.Ap_sm; J.Ap_lg = a->src.Ap_lg;
        const ImgDb &img = plan.v.img;
        J.fa = img.fa; J.ca = img.ca; J.norm = img.norm; J.ap = img.ap;
        J.db = a->db;
        J.segmin = match_segmin(ws.scratch);
        J.q64[0] = ws.q64; J.q64[1] = ws.q64b;
        J.qp[0] = ws.qp; J.qp[1] = ws.qpb;
        J.nq[0] = ws.nq; J.nq[1] = ws.nqb;
        J.q16[0] = ws.q16; J.q16[1] = ws.q16b;
        J.amax = a->amax; J.center = a->center;
        J.B_sm = a->B_sm; J.B_lg = a->B_lg; J.Bp_sm = a->Bp_sm; J.Bp_lg = a->Bp_lg;
        J.weights = a->weights; J.kappa_factor = a->kappa_factor;
        J.s = a->s; J.im = a->im; J.dbg_px = a->dbg_px; J.dbg_dist = a->dbg_dist;
        J.dbox = ws.dbox; J.ctl = ws.ctl;
        J.dbr = plan.r16 ? a->dbr : nullptr;
        J.askc = plan.r16 ? r16_askc(a->dbr, a->nrows) : nullptr;
        J.rot = plan.r16 ? a->rot : nullptr;
        return J;
    }

    // K jobs (args[0..K)) of identical shapes in one set of launches per wave; the job
    // table is staged through `pinned` (kept alive by the caller until the copy has run)
    int init_batch(const IaSynthArgs *args, int nj, hipStream_t st, XJob *pinned) {
        IA_ARG(nj <= IA_BATCH_MAX, "ia_synth_levels_batch: too many jobs in one batch");
        int rc = init(&args[0], st, nj);
        if (rc || nj == 1) return rc;
        IA_ARG(plan.xw, "ia_synth_levels_batch: batches run the exact matcher on one GPU (fused kernel)");
        // XJob carries no exchange view: K jobs would publish into one box (cells indexed by
        // query only) and advance its epoch once per wave for K jobs
        IA_ARG(!a->comm && !a->lsh,
               "ia_synth_levels_batch: a batch of K > 1 jobs takes neither a comm nor an LSH index");
        part.resize(K - 1);
        for (int k = 1; k < K; ++k) {
            const IaSynthArgs &b = args[k];
            IA_ARG(b.H == a->H && b.W == a->W && b.nrows == a->nrows && b.N_total == a->N_total &&
                       b.row0 == a->row0 && b.B_hs == a->B_hs && b.B_ws == a->B_ws &&
                       b.src.Ah == a->src.Ah && b.src.Aw == a->src.Aw && b.src.A_hs == a->src.A_hs &&
                       b.src.A_ws == a->src.A_ws && b.src.nAp == a->src.nAp && b.src.nA == a->src.nA &&
                       !b.comm == !a->comm && !b.lsh == !a->lsh && !b.dbi == !a->dbi &&
                       !b.dbg_px == !a->dbg_px,
                   "ia_synth_levels_batch: the jobs of a batch must have identical shapes and forms");
            part[k - 1].member = true;
            if ((rc = part[k - 1].init(&b, st, K))) return rc;
            IA_ARG(part[k - 1].plan.xw, "ia_synth_levels_batch: a job without the fused kernel");
            IA_ARG(part[k - 1].plan.r16 == plan.r16, "ia_synth_levels_batch: jobs with and without the rotated DB");
        }
        pinned[0] = job_entry();
        for (int k = 1; k < K; ++k) pinned[k] = part[k - 1].job_entry();
        // the DB groups (the caller has checked that jobs of one database agree in everything read
        // with it): jobs per group and the jobs in group order, behind the job entries
        int grp[IA_BATCH_MAX];
        const int G = batch_groups(args, K, grp);
        int *gt = reinterpret_cast<int *>(pinned + K);
        gt[0] = G;
        gcount.assign(G, 0);
        for (int k = 0; k < K; ++k) ++gcount[grp[k]];
        for (int g = 0, i = 0; g < IA_BATCH_MAX; ++g) {
            gt[1 + g] = g < G ? gcount[g] : 0;
            for (int k = 0; k < K && g < G; ++k)
                if (grp[k] == g) gt[1 + IA_BATCH_MAX + i++] = k;
        }
        for (int i = K; i < IA_BATCH_MAX; ++i) gt[1 + IA_BATCH_MAX + i] = 0;
        shared_screen = G < K && plan.r16 && g_shared_screen.load(std::memory_order_relaxed) != 0;
        IA_HIP(hipMemcpyAsync(ws.jtab, pinned, batch_table_bytes(K), hipMemcpyHostToDevice, st));
        return IA_OK;
    }
    // a batch's staged tables: K job entries, then the DB group table
    static size_t batch_table_bytes(int K) { return (size_t)K * sizeof(XJob) + IA_GTAB_INTS * sizeof(int); }
    // a batch's DB groups: jobs per group; shared_screen: some jobs share a rotated database and
    // the wave's screen is k_screen16rs (else the K-job k_screen16r, every job for itself)
    std::vector<int> gcount;
    bool shared_screen = false;

    // wave t on the fused path: [wave 0's query rows,] the screen, then k_xwave (exact
    // stage, exchange, tail, and wave t + 1's query rows into the other buffer set)
    int xw_wave(int t, int y_lo, int M, hipStream_t sq) {
        int rc;
        double *q64s[2] = {ws.q64, ws.q64b};
        float *qps[2] = {ws.qp, ws.qpb};
        _Float16 *q16s[2] = {ws.q16, ws.q16b};
        double *nqs[2] = {ws.nq, ws.nqb};
        const int b = t & 1;
        const bool r16 = plan.r16;
        if (t == 0 && (rc = launch_query_wave(B, Bp, 0, y_lo, M, a->center, q64s[0], qps[0], nqs[0],
                                              a->amax, q16s[0], sq, r16 ? a->rot : nullptr)))
            return rc;
        for (int k = 1; k < K && t == 0; ++k) {
            const LevelRun &p = part[k - 1];
            if ((rc = launch_query_wave(p.B, p.Bp, 0, y_lo, M, p.a->center, p.ws.q64, p.ws.qp, p.ws.nq,
                                        p.a->amax, p.ws.q16, sq, r16 ? p.a->rot : nullptr)))
                return rc;
        }
        const DbView &v = plan.v;
        float *segmin = match_segmin(ws.scratch);
        hipEvent_t e0 = wave_event(0), e1 = wave_event(1);
        if (e0) IA_HIP(hipEventRecord(e0, sq));
        const bool cmp = plan.rk && (wave_compact(W, t) || (plan.rkcol && wave_compact_col(W, t)));
        if (r16 && shared_screen) {
            if ((rc = launch_screen16rs(ws.jtab, reinterpret_cast<const int *>(ws.jtab + K), gcount.data(),
                                        (int)gcount.size(), v.nrows, v.sm, M, sq, b)))
                return rc;
            g_shared_waves.fetch_add(1, std::memory_order_relaxed);
        } else if (r16) {
            if ((rc = launch_screen16r(cmp ? a->dbk : a->dbr, v.nrows, v.sm, q16s[b], M, segmin, sq, xa.jobs, K, b,
                                       cmp)))
                return rc;
        } else if ((rc = launch_screen16(v.db, v.im ? &v.img : nullptr, v.nrows, v.sm, q16s[b], M, segmin, sq,
                                         xa.jobs, K, b, a->comm != nullptr))) {
            return rc;
        }
        if (e1) IA_HIP(hipEventRecord(e1, sq));
        // the level's arguments (init), and what wave t changes
        XArgs x = xa;
        x.q64 = q64s[b]; x.qp = qps[b]; x.nq = nqs[b];
        x.q64n = q64s[b ^ 1]; x.qpn = qps[b ^ 1]; x.nqn = nqs[b ^ 1]; x.q16n = q16s[b ^ 1];
        x.M = M;
        if (t + 1 < nw) wave_rows(H, W, t + 1, x.y_lo_n, x.M_n);
        x.f.t = t;
        x.f.y_lo = y_lo;
        if (plan.peer) x.f.px = comm_peer_wave(a->comm);
        if (cmp) {
            g_compact_waves.fetch_add(1, std::memory_order_relaxed);
            const char *dbk = reinterpret_cast<const char *>(a->dbk);
            x.restc = reinterpret_cast<const unsigned char *>(dbk + rk_code_off(v.nrows));
            x.rmax = reinterpret_cast<const float *>(dbk + rk_rmax_off(v.nrows));
            x.q16 = q16s[b];
        }
        const int R = M > x.y_lo_n + x.M_n - y_lo ? M : x.y_lo_n + x.M_n - y_lo;
        if (plan.split) x.xbox = ws.xbox;
        if ((rc = launch_xwave(x, plan.split ? 2 * R : R, plan.variant(K, cmp), sq, K))) return rc;
        return wave_counted(t, M, sq);
    }

    // diagnostic: the sharded path with every shard's exact stage run here, one after the
    // other, each writing its records straight into the all-ranks array; then k_finish
    int sim_wave(int t, int y_lo, int M, hipStream_t sq) {
        int rc;
        for (int r = 0; r < nsim; ++r) {
            if ((rc = launch_query_wave(B, Bp, t, y_lo, M, a->center, ws.q64, ws.qp, ws.nq,
                                        sim[r].amax, ws.q16, sq)))
                return rc;
            const FinishArgs fr = finish_args(t, y_lo, ws.rec_all + (long)r * M, ws.coh);
            if ((rc = launch_match(src, sim[r].row0, sim[r].nrows, sim[r].db, sim[r].dbi, ws.qp, ws.q16, M,
                                   ws.q64, ws.nq, sim[r].amax, ws.scratch, ws.best_local, nullptr,
                                   sq, nullptr, nullptr, &fr)))
                return rc;
        }
        k_finish<<<M, 64, 0, sq>>>(src, ws.rec_all, ws.coh, nsim, M, finish_args(t, y_lo, nullptr, nullptr));
        IA_LAUNCH_CHECK("k_finish");
        return IA_OK;
    }

    int done(hipStream_t st) {
        if (plan.xw) {
            k_err_sticky<<<1, 64, 0, st>>>(ws.ctl, K > 1 ? ws.jtab : nullptr, K);
            IA_HIP(hipGetLastError());
        }
        if (prof) {   // read back by ia_prof_end (no synchronisation here)
            IA_HIP(hipMemcpyAsync(hstats, ws.stats, STATS_BYTES, hipMemcpyDeviceToHost, st));
            prof_push(ProfRec{a->tag, K, a->nrows, pairs, ev0, nscreen, timed ? 1 : 0, hstats,
                              std::move(Ms)});
        }
        return IA_OK;
    }
};

// ---- pipelined levels (ia_synth_levels): the schedule, executor and pool of ia_pipe.h ----
// waves a coarse level is enqueued ahead of its need (IA_PIPE_AHEAD, default 16): every
// coarse wave enqueued before the finest level's first costs ~10 us of host time; same box,
// two passes: c1 16.22 / 16.30 (64), 15.99 / 15.95 (32), 15.24 / 15.12 (16), 15.55 / 15.72 (8)
// ms/step, c3 1 % better at 16-32, c4 unchanged (profiles/r06_pipe_ahead_sweep.txt)
static int pipe_ahead() {
    static const int v = env_int("IA_PIPE_AHEAD", 16);
    return v < 0 ? 0 : v;
}

thread_local PipeRes g_pipe;

}  // namespace ia

using namespace ia;

extern "C" {

int ia_diag_xwave_trace(unsigned long long *out) {
    IA_ARG(out && g_xw_trace, "ia_diag_xwave_trace: no trace (IA_XW_TRACE=<level>)");
    IA_HIP(hipDeviceSynchronize());
    IA_HIP(hipMemcpy(out, g_xw_trace, (size_t)XW_TRACE_T * XW_TRACE_PX * XW_TRACE_N * 8,
                     hipMemcpyDeviceToHost));
    return IA_OK;
}

int ia_diag_wave_rows(int H, int W, int t, int Hc, int Wc, int *out) {
    IA_ARG(out && H > 0 && W > 0 && t >= 0 && t < wave_count(H, W), "ia_diag_wave_rows: bad args");
    wave_rows(H, W, t, out[0], out[1]);
    out[2] = wave_count(H, W);
    out[3] = wave_max_queries(H, W);
    out[4] = Hc > 0 && Wc > 0 ? coarse_need(H, W, Hc, Wc, t) : -1;
    return IA_OK;
}

int ia_diag_pipe_schedule(const int *shapes, const int *builds_next, const int *serial, int n, int order,
                          int ahead, int *out, int cap) {
    IA_ARG(shapes && builds_next && serial && n >= 1 && n <= 64 && ahead >= 0 && (out || cap == 0),
           "ia_diag_pipe_schedule: bad args");
    std::vector<PipeLevel> lv(n);
    for (int j = 0; j < n; ++j) {
        IA_ARG(shapes[2 * j] > 0 && shapes[2 * j + 1] > 0, "ia_diag_pipe_schedule: bad shape");
        lv[j] = PipeLevel{shapes[2 * j], shapes[2 * j + 1], builds_next[j] != 0, serial[j] != 0};
    }
    struct Log {
        int *out, cap, len;
        int put(int kind, int j, int a, int b) {
            if (len < cap) { int *o = out + 4 * len; o[0] = kind; o[1] = j; o[2] = a; o[3] = b; }
            ++len;
            return IA_OK;
        }
        int wave(int j, int t) { return put(0, j, t, 0); }
        int record(int j, int b) { return put(1, j, b, 0); }
        int wait(int j, int i, int b) { return put(2, j, i, b); }
    } log{out, cap, 0};
    const int rc = PipeSched<Log>(lv, ahead, log).run(order);
    return rc ? rc : log.len;
}

int ia_diag_set_xwave(int on) {
    const int prev = xwave_on();
    if (on >= 0 && on <= 2) g_xwave.store(on);
    return prev;
}

int ia_level_resources(const IaSynthArgs *a, int *out) {
    // the kernels this level's plan launches per wave (per level: ADVICE r05): out =
    // {waiting kernel LDS bytes, VGPRs; screen LDS bytes, VGPRs} of the plain one-job variant and
    // the widest screen instance.  Compact waves and split candidates run only without a comm,
    // where no kernel waits for another rank, and fit wherever these do (159 and 155 / 161 VGPRs
    // against 151, the same LDS and 3 workgroups per CU; k_screen16c: less LDS, fewer VGPRs)
    IA_ARG(a && out && a->nrows > 0, "ia_level_resources: bad args");
    LevelPlan p;
    int rc = level_plan(*a, 1, false, &p);
    if (rc) return rc;
    hipFuncAttributes f{}, sc{};
    if (p.xw) rc = xwave_attributes(XwVariant{p.form, false, p.r16, false, false, p.pairs}, &f);
    else IA_HIP(hipFuncGetAttributes(&f, reinterpret_cast<const void *>(&k_peer_finish)));
    if (rc) return rc;
    rc = p.r16 ? screen_resources_r16(&sc) : screen16_attributes(a->dbi != nullptr, &sc);
    if (rc) return rc;
    out[0] = (int)f.sharedSizeBytes;
    out[1] = f.numRegs;
    out[2] = (int)sc.sharedSizeBytes;
    out[3] = sc.numRegs;
    return IA_OK;
}

int ia_synth_status(const IaSynthArgs *levels, int n, void *stream) {
    return levels_status(
        "ia_synth_status", levels, n, stream,
        [](const IaSynthArgs &a) {
            SynthWs w;
            carve(&w, reinterpret_cast<char *>(a.workspace), a.H, a.W, a.nrows, comm_nranks(a.comm));
            return w.ctl + XW_CTL_ERR;
        },
        [](const IaSynthArgs &a) { return comm_peer_mcap(a.comm) > 0 ? ia_peer_status(a.comm) : IA_OK; });
}

int ia_sched_status(int clear) {
    IA_HIP(hipDeviceSynchronize());
    unsigned int e = 0;
    IA_HIP(hipMemcpyFromSymbol(&e, HIP_SYMBOL(g_sched_err), sizeof(e), 0, hipMemcpyDeviceToHost));
    if (clear && e) {
        const unsigned int z = 0;
        IA_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_sched_err), &z, sizeof(z), 0, hipMemcpyHostToDevice));
    }
    if (e) {
        set_error("ia_sched_status: a wait for a neighbouring pixel's decision timed out in some "
                  "level since the last clear (device schedule fault)");
        return IA_E_SCHED;
    }
    return IA_OK;
}

int ia_diag_set_graph_mode(int mode) {
    const int prev = graph_mode();
    if (mode >= 0 && mode <= 2) g_graph_mode.store(mode);
    return prev;
}

int ia_diag_wave_compact(int W, int t) { return wave_compact(W, t) ? 1 : 0; }
int ia_diag_wave_compact_col(int W, int t) { return wave_compact_col(W, t) ? 1 : 0; }

int ia_diag_set_compact_col(int on) {
    const int prev = compact_col() ? 1 : 0;
    if (on == 0 || on == 1) g_compact_col.store(on);
    return prev;
}

int ia_diag_level_compact_col(const IaSynthArgs *a, int K) {
    IA_ARG(a && a->nrows > 0 && K >= 1, "ia_diag_level_compact_col: bad args");
    LevelPlan p;
    const int rc = level_plan(*a, K, false, &p);
    return rc ? rc : (p.rkcol ? 1 : 0);
}

long ia_diag_compact_waves(void) { return g_compact_waves.load(std::memory_order_relaxed); }

// a row threshold's setter: 0 turns the form off, negative leaves it; the previous value (0: off)
static long set_min_rows(std::atomic<long> &g, long rows) {
    const long prev = g.load(std::memory_order_relaxed);
    if (rows >= 0) g.store(rows > 0 ? rows : LONG_MAX);
    return prev == LONG_MAX ? 0 : prev;
}
long ia_diag_set_compact_min_rows(long rows) { return set_min_rows(g_compact_min_rows, rows); }
long ia_diag_set_xsplit_min_rows(long rows) { return set_min_rows(g_xsplit_min_rows, rows); }

int ia_diag_xsplit_grid(int eligible, long nrows, int R) { return xsplit_grid(eligible != 0, nrows, R); }

int ia_diag_level_plan(const IaSynthArgs *a, int K, int *out) {
    IA_ARG(a && out && a->nrows > 0 && K >= 1, "ia_diag_level_plan: bad args");
    LevelPlan p;
    const int rc = level_plan(*a, K, false, &p);
    const int f[IA_PLAN_FIELDS] = {p.xw, p.form, p.r16, p.rk, p.split, p.peer, p.fused, p.tail,
                                   (int)p.v.nseg, p.v.seg_rows, p.v.sm.W > 0};
    for (int i = 0; i < IA_PLAN_FIELDS && !rc; ++i) out[i] = f[i];
    return rc;
}

int ia_release_thread_resources(void) {
    IA_HIP(g_graphs.retire());
    IA_HIP(hipDeviceSynchronize());
    {
        const int rc = g_pipe.release();
        if (rc) return rc;
    }
    if (g_graphs.cap) { IA_HIP(hipStreamDestroy(g_graphs.cap)); g_graphs.cap = nullptr; }
    if (g_graphs.done) { IA_HIP(hipEventDestroy(g_graphs.done)); g_graphs.done = nullptr; }
    return IA_OK;
}

int ia_prof_begin(void) {
    std::lock_guard<std::mutex> l(g_prof->mu);
    g_prof->active = true;
    g_prof->next = 0;
    g_prof->pinned_next = 0;
    g_prof->recs.clear();
    return IA_OK;
}

int ia_prof_prepare(long nevents) {
    std::lock_guard<std::mutex> l(g_prof->mu);
    while ((long)g_prof->ev.size() < nevents) {
        hipEvent_t e;
        IA_HIP(hipEventCreate(&e));
        g_prof->ev.push_back(e);
    }
    return IA_OK;
}

int ia_prof_launches(int rec, float *ms, int *M, int max) {
    std::lock_guard<std::mutex> l(g_prof->mu);
    IA_ARG(rec >= 0 && rec < (int)g_prof->recs.size(), "ia_prof_launches: no such record");
    const ProfRec &p = g_prof->recs[rec];
    const int n = p.timed ? p.nscreen : 0;
    for (int i = 0; i < n && i < max; ++i) {
        if (ms) IA_HIP(hipEventElapsedTime(&ms[i], g_prof->ev[p.ev0 + 3 * i], g_prof->ev[p.ev0 + 3 * i + 1]));
        if (M) M[i] = p.M[i];
    }
    return n;
}

int ia_prof_waves(int rec, float *tail_ms, float *gap_ms, int max) {
    std::lock_guard<std::mutex> l(g_prof->mu);
    IA_ARG(rec >= 0 && rec < (int)g_prof->recs.size(), "ia_prof_waves: no such record");
    const ProfRec &p = g_prof->recs[rec];
    const int n = p.timed ? p.nscreen : 0;
    for (int i = 0; i < n && i < max; ++i) {
        const size_t e = p.ev0 + 3 * i;
        if (tail_ms) IA_HIP(hipEventElapsedTime(&tail_ms[i], g_prof->ev[e + 1], g_prof->ev[e + 2]));
        if (gap_ms) {
            gap_ms[i] = 0.f;
            if (i + 1 < n) IA_HIP(hipEventElapsedTime(&gap_ms[i], g_prof->ev[e + 2], g_prof->ev[e + 3]));
        }
    }
    return n;
}

int ia_prof_end(double *out, int maxrec) {
    IA_HIP(hipDeviceSynchronize());
    std::lock_guard<std::mutex> l(g_prof->mu);
    g_prof->active = false;
    const int n = (int)g_prof->recs.size();
    for (int r = 0; r < n && r < maxrec && out; ++r) {
        const ProfRec &p = g_prof->recs[r];
        double ms = 0.0;
        for (int i = 0; p.timed && i < p.nscreen; ++i) {
            float e = 0.f;
            IA_HIP(hipEventElapsedTime(&e, g_prof->ev[p.ev0 + 3 * i], g_prof->ev[p.ev0 + 3 * i + 1]));
            ms += e;
        }
        unsigned long long st[STATS_LINE] = {};
        for (int sl = 0; sl < STATS_SLOTS; ++sl)
            for (int i = 0; i < STATS_LINE; ++i) st[i] += p.hstats[sl * STATS_LINE + i];
        double *o = out + (size_t)r * IA_PROF_FIELDS;
        o[0] = p.tag;
        o[1] = (double)p.nrows;
        o[2] = p.pairs;
        o[3] = p.timed ? ms : 0.0;
        o[4] = p.timed ? p.nscreen : 0;
        o[5] = (double)st[0];
        o[6] = (double)st[1];
        o[7] = (double)st[2];
        o[8] = (double)st[3] * 1e-2;   // 100 MHz ticks -> us
        o[9] = (double)st[4] * 1e-2;
        o[10] = p.jobs;
    }
    return n;
}

size_t ia_synth_workspace_bytes(int H, int W, long nrows, int nranks) {
    if (H <= 0 || W <= 0 || nrows <= 0 || nranks <= 0) return 0;
    return carve(nullptr, nullptr, H, W, nrows, nranks);
}

int ia_synth_level(const IaSynthArgs *a, void *stream) {
    hipStream_t st = S(stream);
    LevelRun run;
    int rc = run.init(a, st);
    if (rc) return rc;
    // HIP-graph capture of the whole wave loop (IA_GRAPH / ia_diag_set_graph_mode: 0 off
    // [default], 1 levels of <= 2^18 rows, 2 every single-GPU level).  Sharded levels stay
    // eager (RCCL calls per wave).  Launches inside a graph are not timed.
    const int gm = graph_mode();
    const bool use_graph = !a->comm && !(a->flags & IA_SYNTH_EAGER) &&
                           (gm == 2 || (gm == 1 && a->nrows <= (1L << 18)));
    if (!use_graph) {
        for (int t = 0; t < run.nw; ++t)
            if ((rc = run.wave(t, st))) return rc;
    } else {
        // capture on a private stream (the legacy default stream cannot capture)
        run.timed = false;
        IA_HIP(g_graphs.retire());
        if (!g_graphs.cap) IA_HIP(hipStreamCreateWithFlags(&g_graphs.cap, hipStreamNonBlocking));
        IA_HIP(hipStreamBeginCapture(g_graphs.cap, hipStreamCaptureModeThreadLocal));
        for (int t = 0; t < run.nw && !rc; ++t) rc = run.wave(t, g_graphs.cap);
        hipGraph_t graph = nullptr;
        const hipError_t ec = hipStreamEndCapture(g_graphs.cap, &graph);
        if (rc) { if (graph) (void)hipGraphDestroy(graph); return rc; }
        IA_HIP(ec);
        hipGraphExec_t exec = nullptr;
        const hipError_t ei = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        IA_HIP(ei);
        IA_HIP(hipGraphLaunch(exec, st));
        IA_HIP(g_graphs.hold(exec, st));
    }
    return run.done(st);
}

int ia_diag_synth_level_shards(const IaSynthArgs *a, const IaShardDb *shards, int n,
                               void *stream) {
    IA_ARG(a && shards && n >= 1 && !a->comm && !a->lsh, "ia_diag_synth_level_shards: bad args");
    long total = 0;
    for (int r = 0; r < n; ++r) {
        IA_ARG((shards[r].db || shards[r].dbi) && shards[r].amax && shards[r].row0 == total && shards[r].nrows > 0,
               "ia_diag_synth_level_shards: shards must tile the rows in order");
        total += shards[r].nrows;
    }
    IA_ARG(total == a->N_total, "ia_diag_synth_level_shards: shards must cover the DB");
    hipStream_t st = S(stream);
    LevelRun run;
    run.sim = shards;
    run.nsim = n;
    int rc = run.init(a, st);
    if (rc) return rc;
    for (int t = 0; t < run.nw; ++t)
        if ((rc = run.wave(t, st))) return rc;
    return run.done(st);
}

// n consecutive levels of K identical-shape jobs (levels[j * K + k]: level j of job k)
static int synth_levels(const IaSynthArgs *levels, int n, int K, void *stream) {
    IA_ARG(levels && n >= 1 && n <= 64 && K >= 1 && K <= IA_BATCH_MAX, "ia_synth_levels: bad level count");
    auto lv = [&](int j) -> const IaSynthArgs & { return levels[(size_t)j * K]; };
    for (int j = 1; j < n; ++j)
        for (int k = 0; k < K; ++k)
            IA_ARG(levels[(size_t)j * K + k].Bp_sm == levels[(size_t)(j - 1) * K + k].Bp_lg &&
                       levels[(size_t)j * K + k].B_hs == levels[(size_t)(j - 1) * K + k].H &&
                       levels[(size_t)j * K + k].B_ws == levels[(size_t)(j - 1) * K + k].W,
                   "ia_synth_levels: levels must be consecutive (level j's coarse B' = level j-1's B')");
    hipStream_t st = S(stream);
    int rc = g_pipe.begin(n, st);
    if (rc) return rc;
    // the batch job tables go through a pinned host buffer kept by this thread (reused once
    // the previous call's copies have run)
    XJob *pinned = nullptr;
    if (K > 1) {
        IA_HIP(g_pipe.staging((size_t)n * LevelRun::batch_table_bytes(K), reinterpret_cast<void **>(&pinned)));
    }
    // Levels whose DB is sharded over several ranks and exchanged over RCCL never overlap
    // one another: each one's first wave waits for the previous such level's last.  RCCL's
    // kernels wait in-kernel for the other ranks, and two communicators in flight on
    // different streams can deadlock when the waiting kernels hold the CUs the awaited
    // ones need.  The same held for the first device-side exchange, whose waits sat inside
    // the exact stage's 4-wave, 250-VGPR workgroups (two bench ranks on one GPU deadlocked
    // on c3 with the levels pipelined).  Its waits now live in k_peer_finish's small 2-wave
    // workgroups (c4: at most (171 + 342) x 2 waves of 152 VGPRs when two sharded levels
    // overlap, a quarter of a GPU's wave slots), so those levels overlap: 3 ranks sharing
    // one GPU with every c3 level sharded and overlapping complete, and the simulated
    // G = 8 rank gains 3.6 % (profiles/r02_shard_overlap.txt).  IA_SHARD_OVERLAP=0
    // serializes them too.
    // Ranks sharing ONE GPU (IA_SHARE_GPU=1, the tests' multi-rank mode) serialize them as
    // well: their waiting workgroups (k_xwave's, up to ~343 per level and rank) could then
    // fill the one GPU's slots while a third rank's awaited ones cannot start.
    static const int overlap = env_int("IA_SHARD_OVERLAP", 1) && !env_int("IA_SHARE_GPU", 0);
    auto multi_rank = [&](int j) {
        if (lv(j).comm == nullptr || lv(j).nrows >= lv(j).N_total) return false;
        return !(overlap && comm_peer_mcap(lv(j).comm) > 0);
    };
    std::vector<LevelRun> run(n);
    std::vector<PipeLevel> pl(n);
    for (int j = 0; j < n; ++j) {
        if ((rc = g_pipe.level_begin(j)) ||
            (rc = run[j].init_batch(&levels[(size_t)j * K], K, g_pipe.stream(j),
                                    K > 1 ? reinterpret_cast<XJob *>(reinterpret_cast<char *>(pinned) +
                                                                     (size_t)j * LevelRun::batch_table_bytes(K))
                                          : nullptr)))
            return rc;
        // (on the fused path wave t's launch also builds wave t + 1's query rows)
        pl[j] = PipeLevel{run[j].H, run[j].W, run[j].plan.xw, multi_rank(j)};
    }
    // enqueue order (IA_PIPE_ORDER): 0 [default] the finest level first, coarse waves just
    // ahead of their need; 1 every level whole, coarse to fine.  One host thread enqueues
    // ~10 us of launches per wave, so with 1 the finest level's first wave was enqueued only
    // after every coarse wave (c1: at +14 ms of a 27 ms traced step, tools/trace_queues.py).
    // Same box, round 6: c1 18.51 -> 16.30, c3 76.0 -> 71.3, c4 783.7 -> 750.8, c5 794 -> 786
    // ms/step (profiles/r06_pipe_order_ab.txt)
    static const int order = env_int("IA_PIPE_ORDER", 0);
    return pipe_execute(run, pl, order, pipe_ahead(), st);
}

int ia_synth_levels(const IaSynthArgs *levels, int n, void *stream) { return synth_levels(levels, n, 1, stream); }

int ia_synth_levels_batch(const IaSynthArgs *levels, int n, int K, void *stream) {
    // jobs of a level that pass one database are one DB group (ia_batch_groups): it stands for
    // one level index, so everything read with it is the same memory too
    for (int j = 0; levels && j < n && n <= 64 && K > 1 && K <= IA_BATCH_MAX; ++j)
        for (int k = 1; k < K; ++k) {
            const IaSynthArgs &b = levels[(size_t)j * K + k];
            for (int p = 0; p < k; ++p) {
                const IaSynthArgs &c = levels[(size_t)j * K + p];
                if (!((b.db && b.db == c.db) || (b.dbi && b.dbi == c.dbi) || (b.dbr && b.dbr == c.dbr))) continue;
#define IA_SAME(field) IA_ARG(b.field == c.field, "ia_synth_levels_batch: jobs sharing a database differ in " #field)
                IA_SAME(db); IA_SAME(dbi); IA_SAME(dbr); IA_SAME(dbk); IA_SAME(rot); IA_SAME(center); IA_SAME(amax);
                IA_SAME(row0); IA_SAME(nrows);
                IA_SAME(src.A_sm); IA_SAME(src.A_lg); IA_SAME(src.Ap_sm); IA_SAME(src.Ap_lg); IA_SAME(src.nA);
#undef IA_SAME
            }
        }
    return synth_levels(levels, n, K, stream);
}

/* K LSH jobs per set of launches (k_query_wave_lb, k_lsh_query_b, k_lsh_tail_b; K = 1: the
 * single job's launches).  Everything that cannot run is refused here, before anything is
 * enqueued; the message names the field. */
int ia_synth_levels_lsh_batch(const IaSynthArgs *levels, int n, int K, void *stream) {
    const std::string who = "ia_synth_levels_lsh_batch";
    IA_ARG(K >= 1 && K <= IA_BATCH_MAX, who + ": K out of range (1 .. 128)");
    IA_ARG(levels && n >= 1 && n <= 64, who + ": bad level count");
    for (int j = 0; j < n; ++j) {
        const IaSynthArgs &a = levels[(size_t)j * K];
        for (int k = 0; k < K; ++k) {
            const IaSynthArgs &b = levels[(size_t)j * K + k];
            IA_ARG(b.lsh, who + ": every job of every level needs lsh (exact batches: ia_synth_levels_batch)");
            IA_ARG(b.center, who + ": lsh needs center (55 doubles)");
            IA_ARG(!b.comm, who + ": an lsh batch takes no comm (the LSH matcher runs unsharded)");
#define IA_SAME(field) IA_ARG(b.field == a.field, who + ": the jobs of an lsh batch differ in " #field)
            IA_SAME(H); IA_SAME(W); IA_SAME(B_hs); IA_SAME(B_ws);
            IA_SAME(src.Ah); IA_SAME(src.Aw); IA_SAME(src.A_hs); IA_SAME(src.A_ws); IA_SAME(src.nAp);
            IA_SAME(src.nA);
            IA_SAME(nrows); IA_SAME(lsh->L); IA_SAME(lsh->k);
#undef IA_SAME
            {
                int rc = check_args(&b);
                if (rc || (rc = lsh_check(b.lsh, who.c_str()))) return rc;
            }
            if (j > 0) {
                const IaSynthArgs &c = levels[(size_t)(j - 1) * K + k];
                IA_ARG(b.Bp_sm == c.Bp_lg && b.B_hs == c.H && b.B_ws == c.W,
                       who + ": levels must be consecutive (level j's coarse B' = level j-1's B')");
            }
            IA_ARG(b.row0 == 0 && b.nrows == b.N_total,
                   who + ": an lsh batch takes no partial row range (row0, nrows)");
            IA_ARG(!b.dbg_px == !a.dbg_px,
                   who + ": the jobs of an lsh batch differ in having debug outputs (dbg_px, dbg_dist)");
            // jobs passing one table set are one DB group: it stands for one level index, so
            // everything read with it is the same memory too
            for (int p = 0; p < k; ++p) {
                const IaSynthArgs &c = levels[(size_t)j * K + p];
                if (c.lsh->mem != b.lsh->mem) continue;
#define IA_SAME(field) IA_ARG(b.field == c.field, who + ": jobs sharing lsh->mem differ in " #field)
                IA_SAME(lsh->proj); IA_SAME(lsh->w); IA_SAME(center);
                IA_SAME(src.A_sm); IA_SAME(src.A_lg); IA_SAME(src.Ap_sm); IA_SAME(src.Ap_lg); IA_SAME(src.nA);
#undef IA_SAME
                break;   // (p agrees with the group's earlier jobs already)
            }
        }
    }
    if (K == 1) return synth_levels(levels, n, 1, stream);
    hipStream_t st = S(stream);
    int rc = g_pipe.begin(n, st);
    if (rc) return rc;
    // one job table per level, staged once through this thread's pinned buffer (ia_pipe.h)
    LJob *pinned = nullptr;
    IA_HIP(g_pipe.staging((size_t)n * K * sizeof(LJob), reinterpret_cast<void **>(&pinned)));
    std::vector<LevelRun> run(n);
    std::vector<PipeLevel> pl(n);
    for (int j = 0; j < n; ++j) {
        if ((rc = g_pipe.level_begin(j)) ||
            (rc = run[j].init_lsh_batch(&levels[(size_t)j * K], K, g_pipe.stream(j), pinned + (size_t)j * K)))
            return rc;
        pl[j] = PipeLevel{run[j].H, run[j].W, false, false};
    }
    static const int order = env_int("IA_PIPE_ORDER", 0);
    return pipe_execute(run, pl, order, pipe_ahead(), st);
}

int ia_batch_groups(const IaSynthArgs *level_jobs, int K, int *group_of_job) {
    IA_ARG(level_jobs && group_of_job, "ia_batch_groups: bad args");
    IA_ARG(K >= 1 && K <= IA_BATCH_MAX, "ia_batch_groups: K out of range (1 .. 128)");
    for (int k = 0; k < K; ++k) IA_SRC_NA(level_jobs[k].src, "ia_batch_groups");
    return batch_groups(level_jobs, K, group_of_job);
}

int ia_diag_set_shared_screen(int on) {
    const int prev = g_shared_screen.load();
    if (on == 0 || on == 1) g_shared_screen.store(on);
    return prev;
}

long ia_diag_shared_screen_waves(void) { return g_shared_waves.load(std::memory_order_relaxed); }

}  // extern "C"
