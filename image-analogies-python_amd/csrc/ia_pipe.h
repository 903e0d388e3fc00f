// ia_pipe.h — the level pipeline of ia_synth_levels and ia_synth_levels3 (host code only):
// the wavefront geometry of a level, the schedule that runs level j behind level j-1, the
// executor that turns it into launches, event records and stream waits, and the per-thread
// pool of streams and events it uses.  DESIGN.md §6.
#ifndef IA_PIPE_H
#define IA_PIPE_H

#include "ia_common.h"

#include <string>
#include <vector>

namespace ia {

// ---- wave geometry: wave t of an H x W level holds the pixels x + 3y = t -----------------
static inline int wave_count(int H, int W) { return (W - 1) + 3 * (H - 1) + 1; }

// wave t: pixels y in [y_lo, y_lo + M), x = t - 3y
static inline void wave_rows(int H, int W, int t, int &y_lo, int &M) {
    const int lo_num = t - (W - 1);
    y_lo = lo_num > 0 ? (lo_num + 2) / 3 : 0;
    const int y_hi = t / 3 < H - 1 ? t / 3 : H - 1;
    M = y_hi - y_lo + 1;
}

// Wave t may take the compact screen (ia_rot16.h RK_*) iff none of its pixels has B'
// initialisation noise in its window's causal part, i.e. lies in row 0 (y = 0, x = t: t <= W - 1)
// or column 0 (x = 0: t = 3y): those queries' noise is in the dropped components
static inline bool wave_compact(int W, int t) { return t >= W && t % 3 != 0; }
// The other waves past row 0: t = 3y, whose only border pixel is (y, 0) (none once y is past the
// last row).  Its noise lies on the two own-row axes (ia_rot16.h RK_AXES), so the wave may take
// the compact screen where the level's basis keeps them (LevelPlan::rkcol)
static inline bool wave_compact_col(int W, int t) { return t >= W && t % 3 == 0; }

// the most queries of one wave, + 1 (the workspaces are sized by it)
static inline int wave_max_queries(int H, int W) {
    const int byw = (W + 2) / 3;   // ceil(W/3)
    return (H < byw ? H : byw) + 1;
}

// Wave t of an H x W level reads the coarse Hc x Wc level only through the 3x3 coarse windows
// of its pixels: coarse pixels up to (y/2 + 1, x/2 + 1), i.e. coarse waves <= the maximum over
// the wave's pixels of min(x/2 + 1, Wc-1) + 3 min(y/2 + 1, Hc-1) (the mirror at the coarse
// level's far edges stays inside that box).
static inline int coarse_need(int H, int W, int Hc, int Wc, int t) {
    int y_lo, M;
    wave_rows(H, W, t, y_lo, M);
    int need = 0;
    for (int y = y_lo; y < y_lo + M; ++y) {
        const int x = t - 3 * y;
        const int cy = y / 2 + 1 < Hc - 1 ? y / 2 + 1 : Hc - 1;
        const int cx = x / 2 + 1 < Wc - 1 ? x / 2 + 1 : Wc - 1;
        need = cx + 3 * cy > need ? cx + 3 * cy : need;
    }
    return need;
}

// ---- the schedule ------------------------------------------------------------------------
// Level j may start as soon as level j-1 has finished coarse_need(0) and run concurrently
// behind it on its own stream: the step's critical path becomes ~ the finest level's waves
// instead of the sum of all levels' waves.  Levels wait on events recorded every PIPE_BLOCK
// waves of the level below.
// waves per recorded event (build-time IA_PIPE_BLOCK).  8 against 4, same boxes, two
// rounds: c1 14.73-15.07 vs 14.93-15.19, c3 69.2-70.7 vs 69.9-72.3, c4 734-743 vs 735-744
// ms/step, colour at the c3 size 112.6 / 111.0 vs 113.8 / 112.6; 2 is slower (c1 16.1), 16
// mixed (profiles/r06_pipe_block_ab.txt)
#ifndef IA_PIPE_BLOCK
#define IA_PIPE_BLOCK 8
#endif
constexpr int PIPE_BLOCK = IA_PIPE_BLOCK;

struct PipeLevel {
    int H, W;
    bool builds_next;   // the launch of wave t also builds wave t + 1's query rows
    // a serialised multi-rank level: its first wave waits for the last wave of the nearest
    // such level below (ia_synth.hip, synth_levels)
    bool serial;
};

// Decides, in order, what the pipeline enqueues and hands each action to the sink as it is
// decided: sink.wave(j, t) enqueues wave t of level j on level j's stream, sink.record(j, b)
// records "level j done through block b" there, sink.wait(j, i, b) makes level j's stream
// wait for block b of level i.  Every wave comes behind a wait covering the coarse waves it
// reads (tests/test_host.py checks this on ia_diag_pipe_schedule).  order 0: the finest
// level first, each coarse level enqueued `ahead` waves past the block a finer wave needs;
// order 1: every level whole, coarse to fine.  No HIP call here.
template <class Sink>
struct PipeSched {
    const std::vector<PipeLevel> &lv;
    const int ahead;
    Sink &sink;
    std::vector<int> nw, next, waited, need_max;

    PipeSched(const std::vector<PipeLevel> &levels, int ahead_, Sink &s)
        : lv(levels), ahead(ahead_), sink(s), nw(levels.size()), next(levels.size(), 0),
          waited(levels.size(), -1), need_max(levels.size(), 0) {
        for (size_t j = 0; j < lv.size(); ++j) nw[j] = wave_count(lv[j].H, lv[j].W);
    }

    // enqueue level j through wave `target` (and the coarse waves it needs, first)
    int advance(int j, int target) {
        int rc;
        if (target > nw[j] - 1) target = nw[j] - 1;
        if (next[j] == 0 && target >= 0 && lv[j].serial) {
            for (int i = j - 1; i >= 0; --i) {
                if (!lv[i].serial) continue;
                if ((rc = advance(i, nw[i] - 1)) || (rc = sink.wait(j, i, (nw[i] - 1) / PIPE_BLOCK))) return rc;
                break;
            }
        }
        for (; next[j] <= target; ++next[j]) {
            const int t = next[j];
            if (j > 0) {
                const int w = coarse_need(lv[j].H, lv[j].W, lv[j - 1].H, lv[j - 1].W,
                                          lv[j].builds_next && t + 1 < nw[j] ? t + 1 : t);
                need_max[j] = w > need_max[j] ? w : need_max[j];
                if (need_max[j] > waited[j]) {
                    const int b = need_max[j] / PIPE_BLOCK;
                    if ((rc = advance(j - 1, b * PIPE_BLOCK + PIPE_BLOCK - 1 + ahead)) || (rc = sink.wait(j, j - 1, b)))
                        return rc;
                    waited[j] = b * PIPE_BLOCK + PIPE_BLOCK - 1;
                }
            }
            if ((rc = sink.wave(j, t))) return rc;
            if (((t + 1) % PIPE_BLOCK == 0 || t == nw[j] - 1) && (rc = sink.record(j, t / PIPE_BLOCK))) return rc;
        }
        return IA_OK;
    }

    int run(int order) {
        const int n = (int)lv.size();
        for (int i = 0; i < n; ++i) {
            const int j = order ? i : n - 1 - i;
            const int rc = advance(j, nw[j] - 1);
            if (rc) return rc;
        }
        return IA_OK;
    }
};

// ---- the pool ----------------------------------------------------------------------------
struct PipeRes {   // per host thread: the level streams and events of a pipelined call
    std::vector<hipStream_t> streams;   // levels 0 .. n-2 of a call (coarser): high priority
    hipStream_t plain = nullptr;        // level n-1 of a call (the finest): plain priority
    int n = 0;                          // levels of the call under way
    std::vector<hipEvent_t> events;
    size_t next_event = 0;
    // pinned staging of the batch job tables: reused after the previous call's copies ran
    void *pin = nullptr;
    size_t pin_bytes = 0;
    hipEvent_t staged = nullptr;
    bool staged_rec = false, pin_used = false;
    hipEvent_t start = nullptr;         // this call's beginning on its caller's stream (one of `events`)
    hipEvent_t last = nullptr;          // the previous call's end (on its caller's stream)
    bool last_rec = false;

    // the finest level always takes the plain-priority stream, whatever n earlier calls had
    hipStream_t stream(int j) const { return j == n - 1 ? plain : streams[j]; }

    hipError_t event(hipEvent_t *e) {
        if (next_event == events.size()) {
            hipEvent_t x;
            hipError_t r = hipEventCreateWithFlags(&x, hipEventDisableTiming);
            if (r != hipSuccess) return r;
            events.push_back(x);
        }
        *e = events[next_event++];
        return hipSuccess;
    }

    hipError_t staging(size_t bytes, void **p) {
        hipError_t r = hipSuccess;
        if (!staged && (r = hipEventCreateWithFlags(&staged, hipEventDisableTiming)) != hipSuccess) return r;
        if (staged_rec && (r = hipEventSynchronize(staged)) != hipSuccess) return r;
        if (bytes > pin_bytes) {
            if (pin && (r = hipHostFree(pin)) != hipSuccess) return r;
            pin = nullptr;
            if ((r = hipHostMalloc(&pin, bytes, hipHostMallocDefault)) != hipSuccess) return r;
            pin_bytes = bytes;
        }
        staged_rec = pin_used = true;
        *p = pin;
        return r;
    }

    // start an n-level call on the caller's stream st; then level_begin(j) before anything is
    // enqueued for level j
    int begin(int levels, hipStream_t st) {
        // a call waits on the host for this thread's previous call to end (IA_PIPE_DRAIN,
        // default 1) before it enqueues anything.  Queued behind a running call, the coarse
        // levels' first packets (their waits on `start`) sit in the high-priority queues for the
        // whole of the previous call's finest level, and while they do the finest level's
        // launches run ~4x slower (c1 with no host sync between steps: 61 vs 15 ms/step, screens
        // 39 vs 9.4 us; IA_PIPE_PRIO=0 18 ms; profiles/r06_pipe_drain_ab.txt).  The host's other
        // per-call work (the level indexes) still overlaps the previous call
        static const int drain = env_int("IA_PIPE_DRAIN", 1);
        if (drain && last_rec) IA_HIP(hipEventSynchronize(last));
        // one stream per level; coarser levels at high priority (IA_PIPE_PRIO, default 1) so
        // that they run ahead of the finest level instead of time-sharing with it.  Measured
        // (c4, one box, `tools/gpu.sh abknob`): one level at a time 1706-1713 ms/step; pipelined
        // with the coarse levels enqueued whole first at high priority 1641-1643 ms (the finest
        // level's plateau screens undisturbed: k_screen16<11> 400 vs 396 us); enqueued just
        // ahead of their need 1619-1621 ms but the plateau screens contended (414 us).
        // The pools grow as needed (a pool sized by a smaller first call used to hand a later
        // call's coarse level a plain stream and its finest a high-priority one)
        static const int prio_on = env_int("IA_PIPE_PRIO", 1);
        while ((int)streams.size() < levels - 1) {
            int lo = 0, hi = 0;
            IA_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
            hipStream_t s;
            if (prio_on)
                IA_HIP(hipStreamCreateWithPriority(&s, hipStreamNonBlocking, hi));
            else
                IA_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
            streams.push_back(s);
        }
        if (!plain) IA_HIP(hipStreamCreateWithFlags(&plain, hipStreamNonBlocking));
        n = levels;
        next_event = 0;
        pin_used = false;
        IA_HIP(event(&start));
        IA_HIP(hipEventRecord(start, st));
        return IA_OK;
    }
    // level j's stream comes behind the caller's work (its init's memsets too).  Level by
    // level, wait then init: every wait issued first cost c1 1.7 % (profiles/r07_one_pipeline_ab.txt)
    int level_begin(int j) {
        IA_HIP(hipStreamWaitEvent(stream(j), start, 0));
        return IA_OK;
    }

    // ia_release_thread_resources: after a device synchronisation
    int release() {
        for (hipStream_t s : streams) IA_HIP(hipStreamDestroy(s));
        if (plain) IA_HIP(hipStreamDestroy(plain));
        for (hipEvent_t e : events) IA_HIP(hipEventDestroy(e));
        if (pin) IA_HIP(hipHostFree(pin));
        if (staged) IA_HIP(hipEventDestroy(staged));
        if (last) IA_HIP(hipEventDestroy(last));
        *this = PipeRes{};
        return IA_OK;
    }
};
extern thread_local PipeRes g_pipe;   // (ia_synth.hip)

// ---- the executor ------------------------------------------------------------------------
// Run: nw, wave(t, stream), done(stream); run[j] was initialised on g_pipe.stream(j) after
// g_pipe.begin and level_begin(j).  Enqueues every level's waves as PipeSched decides, then joins the level
// streams into the caller's stream st.
template <class Run>
struct PipeExec {
    PipeRes &P;
    std::vector<Run> &run;
    std::vector<std::vector<hipEvent_t>> blk;   // blk[j][b]: level j done through block b
    int wave(int j, int t) { return run[j].wave(t, P.stream(j)); }
    int record(int j, int b) {
        IA_HIP(P.event(&blk[j][b]));
        IA_HIP(hipEventRecord(blk[j][b], P.stream(j)));
        return IA_OK;
    }
    int wait(int j, int i, int b) {
        IA_HIP(hipStreamWaitEvent(P.stream(j), blk[i][b], 0));
        return IA_OK;
    }
};

template <class Run>
static int pipe_execute(std::vector<Run> &run, const std::vector<PipeLevel> &lv, int order, int ahead,
                        hipStream_t st) {
    PipeRes &P = g_pipe;
    const int n = (int)run.size();
    PipeExec<Run> ex{P, run, std::vector<std::vector<hipEvent_t>>(n)};
    for (int j = 0; j < n; ++j) ex.blk[j].assign((run[j].nw + PIPE_BLOCK - 1) / PIPE_BLOCK, nullptr);
    int rc = PipeSched<PipeExec<Run>>(lv, ahead, ex).run(order);
    if (rc) return rc;
    for (int j = 0; j < n; ++j) {
        if ((rc = run[j].done(P.stream(j)))) return rc;
        hipEvent_t e;
        IA_HIP(P.event(&e));
        IA_HIP(hipEventRecord(e, P.stream(j)));
        IA_HIP(hipStreamWaitEvent(st, e, 0));
    }
    if (P.pin_used) IA_HIP(hipEventRecord(P.staged, st));
    if (!P.last) IA_HIP(hipEventCreateWithFlags(&P.last, hipEventDisableTiming));
    IA_HIP(hipEventRecord(P.last, st));
    P.last_rec = true;
    return IA_OK;
}

// ---- status: the error word {tickets[2], error} of each level's workspace ----------------
// err_word(a) -> the device address of level a's error word; after(a) -> a further per-level
// check (IA_OK: none)
template <class ErrWord, class After>
static int levels_status(const std::string &who, const IaSynthArgs *levels, int n, void *stream,
                         ErrWord err_word, After after) {
    IA_ARG(levels && n >= 1, who + ": bad args");
    IA_HIP(hipStreamSynchronize(S(stream)));
    for (int j = 0; j < n; ++j) {
        const IaSynthArgs &a = levels[j];
        IA_ARG(a.workspace && a.H > 0 && a.W > 0 && a.nrows > 0, who + ": bad level");
        unsigned int e = 0;
        IA_HIP(hipMemcpy(&e, err_word(a), sizeof(e), hipMemcpyDeviceToHost));
        if (e) {
            set_error(who + ": a wait for a neighbouring pixel's decision timed out "
                            "(device schedule fault)");
            return IA_E_SCHED;
        }
        const int rc = after(a);
        if (rc) return rc;
    }
    return IA_OK;
}

}  // namespace ia
#endif
