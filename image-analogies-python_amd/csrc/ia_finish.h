// ia_finish.h — per-pixel tail of one synthesis step (image_analogies.py:169-217 with
// best_coherence_match and compute_distance, algorithms.py:92-135).  The tail core below is
// channel-agnostic and written once: the luminance tails (coh_pick / finish_apply here, used
// by ia_synth.hip and ia_match.hip) and the 3-channel ones (k_exact3, k_finish3w,
// ia_color3.hip) differ only in how they compute the distances and in how many channels of
// B' they write.  The fused kernels' xw_finish (ia_xwave.hip) keeps its own copy of the kappa
// test and the record: on kappa_pick / tail_record k_xwave and k_xstrip (250 VGPRs) kept
// every resource figure but were scheduled differently throughout, and the c4 A/B cannot
// resolve the 0.3 % in question (profiles/r08_colour_tail_ab.txt), so their code stays as
// it was.
#pragma once
#include "ia_internal.h"

namespace ia {

// the coherence candidate of one query pixel (coh_pick)
struct CohSel {
    long long wix;       // winning candidate's DB row
    int wr, wc, wim;     // its pixel and A' image
    int rr, rc;          // r*: the B' pixel whose source it continues
    int valid;           // 0: no candidate (first pixel of the level, or none in range)
    double dcoh;         // its weighted distance to the query
};

__device__ __forceinline__ void fin_best(double &bd, long long &bi, double d, long long i) {
    if (d < bd || (d == bd && i < bi)) { bd = d; bi = i; }
}

// ---- the tail core ---------------------------------------------------------------------
// Window position k (0..14 = the reference's product(rows, cols) order over rows y-2..y,
// cols x-2..x+2) of query pixel (y, x): the candidate s(r*) + (q - r*) of the B' pixel r*
// (algorithms.py:101-118).  row: its DB row, -1 where r* is not scanline-earlier, lies
// outside B', or the candidate falls outside A'.  found(row) runs where there is a candidate,
// inside the bounds branches: coh_pick's 55-load gather placed after the call behind a
// row >= 0 test compiles to another schedule (85 instead of 152 VGPRs, not measured).
struct CohPos {
    long long row;
    int r, c, im;
};
template <class F>
__device__ __forceinline__ CohPos coh_pos(int k, int y, int x, int W, int Ah, int Aw,
                                          const int32_t *s, const int32_t *im, F &&found) {
    CohPos p{-1, 0, 0, 0};
    const int rr = y - 2 + k / 5, rc = x - 2 + k % 5;
    if (rr >= 0 && rc >= 0 && rc < W && (rr < y || rc < x)) {
        const long sidx = (long)rr * W + rc;
        const int sr = s[2 * sidx] + y - rr, sc = s[2 * sidx + 1] + x - rc;
        if (sr >= 0 && sr < Ah && sc >= 0 && sc < Aw) {
            p.im = im[sidx];
            p.row = ((long)Ah * p.im + sr) * Aw + sc;
            p.r = sr;
            p.c = sc;
            found(p.row);
        }
    }
    return p;
}
__device__ __forceinline__ CohPos coh_pos(int k, int y, int x, int W, int Ah, int Aw,
                                          const int32_t *s, const int32_t *im) {
    return coh_pos(k, y, x, W, Ah, Aw, s, im, [](long long) {});
}

// One whole wave: lane k's plain distance d (+inf: no candidate) -> the first minimum in
// lane order (np.argmin, algorithms.py:126-128).  False: no lane has a candidate (win = 0).
__device__ __forceinline__ bool coh_first_min(double d, int lane, int &win) {
    long long bl = d < INFINITY ? lane : 0x7fffffffffffffffLL;
    for (int o = 32; o > 0; o >>= 1) {
        const double od = __shfl_xor(d, o);
        const long long ol = __shfl_xor(bl, o);
        fin_best(d, bl, od, ol);
    }
    const bool valid = bl != 0x7fffffffffffffffLL;
    win = valid ? (int)bl : 0;
    return valid;
}
// the CohSel of coh_first_min's result for pixel (y, x): p the CohPos of window position win,
// dcoh its weighted distance
__device__ __forceinline__ CohSel coh_sel(const CohPos &p, int win, bool valid, int y, int x,
                                          double dcoh) {
    return CohSel{p.row, p.r, p.c, p.im, y - 2 + win / 5, x - 2 + win % 5, valid, dcoh};
}

// The kappa test (image_analogies.py:200-211): the pixel's source is the coherence candidate
// c when its weighted distance is within kappa_factor of the exact winner's (d_app), else the
// exact winner, DB row app of a database of hw = Ah x Aw pixels per image.
struct TailSel {
    int img, pr, pc;     // the chosen source: A' image and pixel
    int ar, ac;          // the exact winner's own pixel (debug record)
};
__device__ __forceinline__ TailSel kappa_pick(long long app, long hw, int Aw, double d_app,
                                              const CohSel &c, double kappa_factor) {
    const long img = app / hw;
    const long rem = app - img * hw;
    const int ar = (int)(rem / Aw), ac = (int)(rem - (long)(rem / Aw) * Aw);
    if (c.valid && c.dcoh <= d_app * kappa_factor) return TailSel{c.wim, c.wr, c.wc, ar, ac};
    return TailSel{(int)img, ar, ac, ar, ac};
}

// One lane: s and im of pixel q = y W + x (image_analogies.py:215-217; the B' value is the
// caller's: one channel or three) and, with the debug outputs (:141-159, 222-240), per pixel
// {p_app row, col, p_coh row, col, r* row, col, has coherence} and {d_app, d_coh} (zeros
// where there is no coherence candidate, as the reference).
__device__ __forceinline__ void tail_record(long q, const TailSel &p, const CohSel &c, double d_app,
                                            int32_t *s, int32_t *im, int32_t *dbg_px,
                                            double *dbg_dist) {
    if (dbg_px) {
        int32_t *o = dbg_px + 7 * q;
        o[0] = p.ar;
        o[1] = p.ac;
        o[2] = c.valid ? c.wr : 0;
        o[3] = c.valid ? c.wc : 0;
        o[4] = c.valid ? c.rr : 0;
        o[5] = c.valid ? c.rc : 0;
        o[6] = c.valid;
        dbg_dist[2 * q] = c.valid ? d_app : 0.0;
        dbg_dist[2 * q + 1] = c.valid ? c.dcoh : 0.0;
    }
    s[2 * q] = p.pr;
    s[2 * q + 1] = p.pc;
    im[q] = p.img;
}

// One 256-thread block: the lexicographic (distance, row) minimum over p[0 .. nb), valid in
// every thread (sd / si: 4 LDS words each; one barrier inside).
__device__ __forceinline__ Best block_best(const Best *p, int nb, double *sd, long long *si) {
    double bd = INFINITY;
    long long bi = 0x7fffffffffffffffLL;
    for (int i = threadIdx.x; i < nb; i += 256) fin_best(bd, bi, p[i].d, p[i].idx);
    for (int o = 32; o > 0; o >>= 1) {
        const double od = __shfl_xor(bd, o);
        const long long oi = __shfl_xor(bi, o);
        fin_best(bd, bi, od, oi);
    }
    if ((threadIdx.x & 63) == 0) { sd[threadIdx.x >> 6] = bd; si[threadIdx.x >> 6] = bi; }
    __syncthreads();
    bd = sd[0];
    bi = si[0];
    for (int w = 1; w < 4; ++w) fin_best(bd, bi, sd[w], si[w]);
    return Best{bd, bi};
}

// ---- the luminance tail ------------------------------------------------------------------
// Coherence half of the tail, executed by ONE 64-lane wave for query pixel m of wave t
// (query in qs, LDS): best_coherence_match (algorithms.py:92-130) over the causal 3x5
// window (lanes 0..14) and the weighted distance of its winner (algorithms.py:133-135).
// Needs only s / im of earlier waves.  Result valid in every lane.
__device__ __forceinline__ CohSel coh_pick(const DbSrc &src, int m, const FinishArgs &f,
                                           const double *qs, int lane) {
    CohSel r{0, 0, 0, 0, 0, 0, 0, 0.0};
    const int y = f.y_lo + m, x = f.t - 3 * y;
    if (y == 0 && x == 0) return r;
    CohPos p{-1, 0, 0, 0};
    double cd = INFINITY;
    if (lane < 15)
        p = coh_pos(lane, y, x, f.W, src.A.h, src.A.w, f.s, f.im,
                    [&](long long row) { cd = sqrt(row_dist2(src, row, qs)); });
    int win;
    if (!coh_first_min(cd, lane, win)) return r;
    p = CohPos{__shfl(p.row, win), __shfl(p.r, win), __shfl(p.c, win), __shfl(p.im, win)};
    double d = 0.0;
    if (lane == 1) d = row_wdist(src, p.row, qs, f.weights);
    return coh_sel(p, win, true, y, x, __shfl(d, 1));
}

// Weighted distance of the exact-match winner app (algorithms.py:133-135) for the kappa
// test: one gather round by lane 0, valid in every lane.  Runs beside coh_pick (another
// wave), so the tail's critical path is max(exact winner + 1 round, coh_pick's 2 rounds).
__device__ __forceinline__ long long app_clamp(long long app, const FinishArgs &f) {
    return (app < 0 || app >= f.N_total) ? 0 : app;   // unreachable: every search has a winner
}
__device__ __forceinline__ double app_wdist(const DbSrc &src, long long app, const FinishArgs &f,
                                            const double *qs, int lane) {
    double d = 0.0;
    if (lane == 0) d = row_wdist(src, app_clamp(app, f), qs, f.weights);
    return __shfl(d, 0);
}

// The rest of the tail: the kappa test of the coherence candidate c against the exact-match
// winner app (weighted distance d_app, app_wdist), and the B' / s / im update with the debug
// record (kappa_pick, tail_record).
__device__ __forceinline__ void finish_apply(const DbSrc &src, long long app, int m,
                                             const FinishArgs &f, const CohSel &c, double d_app,
                                             int lane) {
    const int y = f.y_lo + m, x = f.t - 3 * y;
    const int Aw = src.A.w;
    const long hw = src.hw;
    const TailSel p = kappa_pick(app_clamp(app, f), hw, Aw, d_app, c, f.kappa_factor);
    if (lane == 0) {
        const long q = (long)y * f.W + x;
        f.Bp_lg[q] = src.Ap.lg[p.img * hw + (long)p.pr * Aw + p.pc];
        tail_record(q, p, c, d_app, f.s, f.im, f.dbg_px, f.dbg_dist);
    }
}

// ---- device-side exchange of a sharded level (PeerView, ia_internal.h) ----------------
// granules of (slot, source rank, query) in a receive box
__device__ __forceinline__ unsigned long long *peer_cell(unsigned long long *box, const PeerView &p,
                                                         int src, int q) {
    return box + (((long)(p.epoch & 1) * p.nranks + src) * p.mcap + q) * PEER_CELL;
}
// rank g's box pointer (selects over the kernel argument, not an indexed private copy)
__device__ __forceinline__ unsigned long long *peer_box(const PeerView &p, int g) {
    unsigned long long *box = p.box[0];
#pragma unroll
    for (int k = 1; k < IA_PEER_MAX; ++k) box = g == k ? p.box[k].get() : box;
    return box;
}
// lanes g < nranks of one wave: this rank's winner of query q into rank g's box (system-
// scope 8-byte stores: each granule arrives whole, over xGMI for a peer GPU's box)
__device__ __forceinline__ void peer_publish(const PeerView &p, int q, double d, long long row,
                                             int lane) {
    if (lane >= p.nranks) return;
    unsigned long long *dst = peer_cell(peer_box(p, lane), p, p.rank, q);
    const unsigned long long tag = (unsigned long long)p.epoch << 32;
    const unsigned long long bits = (unsigned long long)__double_as_longlong(d);
    __hip_atomic_store(dst, tag | (bits & 0xffffffffULL), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(dst + 1, tag | (bits >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(dst + 2, tag | (unsigned long long)(unsigned int)row, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_SYSTEM);
}
// 10 s at the 100 MHz real-time counter: a peer that never publishes (a dead rank, or
// memory the peer's stores do not reach) sets the error word instead of hanging the GPU;
// once it is set every later wait of this rank gives up at once (ia_peer_status reports it)
constexpr unsigned long long PEER_TIMEOUT_TICKS = 1000000000ULL;
// one whole wave: lane g < nranks reads rank g's granules of query q from this rank's box
// until all three carry this wave's epoch; then the lexicographic (distance, row) minimum
// over the ranks, valid in every lane.  bd / bi: this rank's own winner (uniform) on entry;
// kept as the result on timeout (false; the error word is then set).
__device__ __forceinline__ bool peer_collect(const PeerView &p, int q, int lane, double &bd,
                                             long long &bi, unsigned long long *raw = nullptr) {
    const bool mine = lane < p.nranks;
    const unsigned long long *src = peer_cell(peer_box(p, p.rank), p, mine ? lane : 0, q);
    unsigned long long g0 = 0, g1 = 0, g2 = 0;
    bool dead = __hip_atomic_load(p.err.get(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0;
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    bool ok;
    for (;;) {
        ok = true;
        if (mine) {
            g0 = __hip_atomic_load(src, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            g1 = __hip_atomic_load(src + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            g2 = __hip_atomic_load(src + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            ok = (unsigned)(g0 >> 32) == p.epoch && (unsigned)(g1 >> 32) == p.epoch &&
                 (unsigned)(g2 >> 32) == p.epoch;
        }
        if (__all(ok) || dead) break;
        if (__builtin_amdgcn_s_memrealtime() - t0 > PEER_TIMEOUT_TICKS) {
            if (lane == 0) __hip_atomic_fetch_or(p.err.get(), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            dead = true;
            break;
        }
        __builtin_amdgcn_s_sleep(1);
    }
    if (raw && lane < 2) { raw[3 * lane] = g0; raw[3 * lane + 1] = g1; raw[3 * lane + 2] = g2; }
    if (dead) return false;
    double d = INFINITY;
    long long i = 0x7fffffffffffffffLL;
    if (mine) {
        d = __longlong_as_double((long long)(((g1 & 0xffffffffULL) << 32) | (g0 & 0xffffffffULL)));
        i = (long long)(g2 & 0xffffffffULL);
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double od = __shfl_xor(d, o);
        const long long oi = __shfl_xor(i, o);
        fin_best(d, i, od, oi);
    }
    bd = d;
    bi = i;
    return true;
}

// ---- the fused per-wave kernel's records (k_xwave, ia_xwave.hip) ---------------------
// one rank's exact winner of one query: distance, global row, the row's weighted (kappa)
// distance to the query and its A' value (the B' value it would write)
struct XRec {
    double d;
    long long i;
    double wd, val;
};
__device__ __forceinline__ void xrec_take(XRec &b, const XRec &o) {
    if (o.d < b.d || (o.d == b.d && o.i < b.i)) b = o;
}
// lexicographic (distance, row) minimum over the wave, valid in every lane
__device__ __forceinline__ XRec xrec_wave_min(XRec b) {
    for (int o = 32; o > 0; o >>= 1) {
        const XRec x{__shfl_xor(b.d, o), __shfl_xor(b.i, o), __shfl_xor(b.wd, o), __shfl_xor(b.val, o)};
        xrec_take(b, x);
    }
    return b;
}
// lanes g < nranks: this rank's record of query q into rank g's box, 7 granules
// {epoch << 32 | 32-bit payload} (d lo/hi, row, wd lo/hi, val lo/hi); rows < 2^32 (checked
// on the host)
__device__ __forceinline__ void peer_publish_rec(const PeerView &p, int q, const XRec &r, int lane) {
    if (lane >= p.nranks) return;
    unsigned long long *dst = peer_cell(peer_box(p, lane), p, p.rank, q);
    const unsigned long long tag = (unsigned long long)p.epoch << 32;
    const unsigned long long bd = (unsigned long long)__double_as_longlong(r.d);
    const unsigned long long bw = (unsigned long long)__double_as_longlong(r.wd);
    const unsigned long long bv = (unsigned long long)__double_as_longlong(r.val);
    auto put = [&](int k, unsigned long long v) {
        __hip_atomic_store(dst + k, tag | v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    };
    put(0, bd & 0xffffffffULL);
    put(1, bd >> 32);
    put(2, (unsigned long long)(unsigned int)r.i);
    put(3, bw & 0xffffffffULL);
    put(4, bw >> 32);
    put(5, bv & 0xffffffffULL);
    put(6, bv >> 32);
}
// one whole wave: lane g < nranks polls rank g's record of query q in this rank's box until
// all 7 granules carry this wave's epoch; r = the lexicographic minimum over the ranks
// (valid in every lane).  On timeout (or an earlier one on this exchange) r is left as the
// caller's own record and false is returned (the error word is set).
__device__ __forceinline__ bool peer_collect_rec(const PeerView &p, int q, int lane, XRec &r) {
    const bool mine = lane < p.nranks;
    const unsigned long long *src = peer_cell(peer_box(p, p.rank), p, mine ? lane : 0, q);
    unsigned long long g0 = 0, g1 = 0, g2 = 0, g3 = 0, g4 = 0, g5 = 0, g6 = 0;
    bool dead = __hip_atomic_load(p.err.get(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0;
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    auto ld = [&](int k) { return __hip_atomic_load(src + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); };
    auto tagged = [&](unsigned long long v) { return (unsigned)(v >> 32) == p.epoch; };
    for (;;) {
        bool ok = true;
        if (mine) {
            g0 = ld(0); g1 = ld(1); g2 = ld(2); g3 = ld(3); g4 = ld(4); g5 = ld(5); g6 = ld(6);
            ok = tagged(g0) && tagged(g1) && tagged(g2) && tagged(g3) && tagged(g4) && tagged(g5) &&
                 tagged(g6);
        }
        if (__all(ok) || dead) break;
        if (__builtin_amdgcn_s_memrealtime() - t0 > PEER_TIMEOUT_TICKS) {
            if (lane == 0) __hip_atomic_fetch_or(p.err.get(), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            dead = true;
            break;
        }
        __builtin_amdgcn_s_sleep(1);
    }
    if (dead) return false;
    auto dbl = [](unsigned long long lo, unsigned long long hi) {
        return __longlong_as_double((long long)(((hi & 0xffffffffULL) << 32) | (lo & 0xffffffffULL)));
    };
    XRec x{INFINITY, 0x7fffffffffffffffLL, 0.0, 0.0};
    if (mine) x = XRec{dbl(g0, g1), (long long)(g2 & 0xffffffffULL), dbl(g3, g4), dbl(g5, g6)};
    r = xrec_wave_min(x);
    return true;
}

// The tail kernels run coh_pick on one wave and app_wdist + finish_apply on another.
// (Picking the coherence candidate ahead, on a side stream beside the screen, measured 5 %
// slower on c4: the per-wave cross-stream event waits cost more than the two gather rounds
// they hide.)

}  // namespace ia
