// ia_color3.hip — 3-channel matching (the reference's convert=False on colour images:
// config.py:29-42 num_ch = 3, algorithms.py:11-47 with channel-interleaved windows).
//
// Each feature row has 165 values: [A coarse 3x3x3 | A fine 5x5x3 | A' coarse 3x3x3 | A'
// fine first 12 pixels x 3], every window flattened (row, col, channel) as
// extract_patches_2d + flatten do.  Distances follow numpy's pairwise summation for n = 165
// (two halves of 80 and 85, 8 accumulators each, algorithms.py:74 / :126 / :135 through
// norm / add.reduce), so the matcher is exact against the oracle.
//
// Per level (ia_db3_build) the rows are materialised in fp64 (1,344 B per row: the exact
// stage's input) with the split-f16 screen operand (704 B per row) after them;
// ia_db3_build_rot adds the rotated split operand (R16c, 352 B per row, §4e).  Per wave: the
// query rows (k_query3s / k_query3r), the MFMA screen's minimum per (query, 32-row tile)
// (k_screen3: 33 MFMAs per 32x32 tile; k_screen3r: 11), then k_exact3: every row of the tiles
// within the bound rescored in fp64 in the oracle's order, and the per-pixel tail, one
// 256-thread workgroup per pixel.  On R16c levels k_exact3<true> (IA_C3_FUSE, default 1) also
// writes the next wave's query rows, so a wave is two launches.  IA_COLOR16=0 keeps the
// exhaustive fp64 search (k_match3) with the tail in k_finish3w.  The tail itself (coherence
// pick over the causal 3x5 window, kappa test, s / im and the debug record) is the tail core
// of ia_finish.h, shared with the luminance kernels (c3_window, c3_decide); the kernels here
// add the 165-term distances and the B' store of all three channels.  ia_synth_levels3 runs
// the levels pipelined; ia_synth_levels3_batch runs K jobs of identical shapes with the job as
// a grid dimension of the R16c wave's launches (k_query3rb, k_screen3rb, k_exact3b: the same
// bodies, per-job pointers from a device job table).  The exact matcher is the default; an
// unsharded level with IaSynthArgs.lsh runs the approximate one (k_query3, then k_lsh3_pixel
// over ia_lsh3_build's tables: ia_lsh.hip's definition with D = 165).  A level sharded over
// ranks (IaSynthArgs.comm) runs the four-launch wave with k_exact3p, which publishes the
// shard's winner, and k_peer_finish3, which collects the ranks' and finishes the pixel.
#include "ia_common.h"
#include "ia_internal.h"
#include "ia_finish.h"
#include "ia_split16.h"
#include "ia_pipe.h"

#include <algorithm>
#include <atomic>
#include <cstring>
#include <vector>

namespace ia {

constexpr int D3 = 165, D3P = 168;              // features, padded row stride (doubles)
constexpr int D3_FULL = 102, D3_HALF = 63;      // A full / A' half feature counts

// numpy pairwise sum of n = 165 values fed in order k = 0..164
struct Pw165 {
    double r[8];
    double h1, h2;
    __device__ __forceinline__ static double tree(const double *r) {
        return ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    }
    __device__ __forceinline__ void feed(int k, double v) {
        const int j = k < 80 ? k : k - 80;
        if (j < 8) r[j] = v;
        else if (j < 80) r[j & 7] += v;
        if (k == 79) h1 = tree(r);
        if (k == 159) h2 = tree(r);
        if (k >= 160) h2 += v;
    }
    __device__ __forceinline__ double result() const { return h1 + h2; }
};

// Pw165's sum of t[0..164] (the same accumulator order, the accumulators in registers: the
// struct's runtime-indexed r[] lives in scratch when its feeding loop is not unrolled)
__device__ __forceinline__ double pw165_sum(const double *t) {
    double h[2];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const double *u = t + 80 * half;
        double r[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = u[j];
#pragma unroll 1
        for (int i = 8; i < 80; i += 8)
#pragma unroll
            for (int j = 0; j < 8; ++j) r[j] += u[i + j];
        h[half] = Pw165::tree(r);
    }
#pragma unroll
    for (int k = 160; k < D3; ++k) h[1] += t[k];
    return h[0] + h[1];
}

struct Img3 {            // a channel-interleaved image (h x w x 3, fp64)
    const double *p;
    int h, w;
    __device__ __forceinline__ double at(int r, int c, int ch) const {
        return p[((long)symi2(r, h) * w + symi2(c, w)) * 3 + ch];
    }
};

// feature k (< 102: full window of the pair sm/lg; the half window keeps the first 63) of
// pixel (r, c): coarse 3x3x3 at (r/2, c/2), then fine 5x5x3 at (r, c)
__device__ __forceinline__ double feat3(const Img3 &sm, const Img3 &lg, int r, int c, int k) {
    if (k < 27) {
        const int t = k / 3, ch = k - 3 * t;
        return sm.at((r >> 1) + t / 3 - 1, (c >> 1) + t % 3 - 1, ch);
    }
    const int t = (k - 27) / 3, ch = (k - 27) - 3 * t;
    return lg.at(r + t / 5 - 2, c + t % 5 - 2, ch);
}

// one thread per (row, feature): the materialised database rows [A full | A'_img half]; the A
// of image img lies a_sm / a_lg doubles per image after Asm / Alg (0: one A for every A' image)
__global__ __launch_bounds__(256) void k_db3_build(Img3 Asm, Img3 Alg, long a_sm, long a_lg,
                                                   const double *Ap_sm, const double *Ap_lg, long row0,
                                                   long nrows, double *__restrict__ db3) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nrows * D3P) return;
    const long lr = i / D3P;
    const int k = (int)(i - lr * D3P);
    double v = 0.0;
    if (k < D3) {
        const long hw = (long)Alg.h * Alg.w;
        const long ix = row0 + lr;
        const long img = ix / hw;
        const long rem = ix - img * hw;
        const int r = (int)(rem / Alg.w), c = (int)(rem - (long)(rem / Alg.w) * Alg.w);
        if (k < D3_FULL) {
            v = feat3(Img3{Asm.p + img * a_sm, Asm.h, Asm.w}, Img3{Alg.p + img * a_lg, Alg.h, Alg.w}, r, c, k);
        } else {
            const Img3 psm{Ap_sm + img * (long)Asm.h * Asm.w * 3, Asm.h, Asm.w};
            const Img3 plg{Ap_lg + img * hw * 3, Alg.h, Alg.w};
            v = feat3(psm, plg, r, c, k - D3_FULL);
        }
    }
    db3[i] = v;
}

// compute_feature_array for one level pair (algorithms.py:11-47), 3 channels
__global__ __launch_bounds__(256) void k_level_features3(Img3 sm, Img3 lg, int nf,
                                                         double *__restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    const long n = (long)lg.h * lg.w;
    if (i >= n * nf) return;
    const long px = i / nf;
    const int k = (int)(i - px * nf);
    out[i] = feat3(sm, lg, (int)(px / lg.w), (int)(px - (px / lg.w) * lg.w), k);
}

// queries of wave t (y = y_lo + m, x = t - 3y): [B full | B' half], one block per pixel
__global__ __launch_bounds__(256) void k_query3(Img3 Bsm, Img3 Blg, Img3 Bpsm, Img3 Bplg, int t,
                                                int y_lo, double *__restrict__ q3) {
    const int m = blockIdx.x, k = threadIdx.x;
    const int y = y_lo + m, x = t - 3 * y;
    if (k >= D3P) return;
    double v = 0.0;
    if (k < D3_FULL) v = feat3(Bsm, Blg, y, x, k);
    else if (k < D3) v = feat3(Bpsm, Bplg, y, x, k - D3_FULL);
    q3[(long)m * D3P + k] = v;
}

// ---- the split-f16 screen for 165-dim rows (IA_COLOR16=1) ---------------
// The screen value of row r and query j is e = |a'|^2 - 2 a'.q' over 166 slots (165
// centred features + the norm slot), carried as f16 pairs exactly like the luminance screen
// (ia_split16.h: the same scales sa, 2^R, sq): alpha = [sa a'_k, sa 2^-R |a'|^2], beta =
// [sq (-2 q'_k), sq 2^R], alpha . beta = sa sq e.  The 176 slots (166 + 10 zeros) are 11
// chunks of 16, each one v_mfma_f32_32x32x16_f16 per product: the 22 cross-term MFMAs
// (a_h q_l, a_l q_h) first, then the 11 main ones (a_h q_h, the norm slot in the last): 33
// per 32x32 tile.  The screen keeps the minimum per (query, 32-row tile); the exact stage
// (k_exact3) rescores in fp64 every row of the tiles whose minimum is within 2 eps3
// of the smallest (the error bound of DESIGN.md §4c).
constexpr int C16_CH = 11;                 // 16-slot chunks
constexpr int C16_GRP = 2 * C16_CH;        // half8 groups per lane and tile: (chunk, hi / lo)
constexpr int C16_TILE = C16_GRP * 64;     // half8 per 32-row (or 32-query) tile
constexpr int C3_NSLOT = 16 * C16_CH;      // 176
constexpr int C3_CAND = 64;                // candidate tiles listed per query (more: all)
constexpr int C3_REG = 8;                  // float4s of tile minima per thread in registers
typedef float floatx16 __attribute__((ext_vector_type(16)));

// lane (row / query l & 31, half h = l >> 5) of group (chunk c, part p) holds slots
// 16c + 8h .. +7: half8 index within a tile
__host__ __device__ constexpr int c16_at(int c, int p, int h, int j) { return (2 * c + p) * 64 + h * 32 + j; }

struct Col16Meta {                         // per database: centre, range keys, bound
    double center[D3P];
    unsigned long long rng[2 * D3P];       // order keys of min and of -max per feature
    unsigned int amax_bits;                // fp32 bits of A >= max row |a'| (atomicMax)
    unsigned int pad;
};

struct Db3View {                           // the ia_db3_build buffer: fp64 rows | split | meta
    double *rows;
    half8 *db16;
    Col16Meta *meta;
    long ntiles;
};
static inline size_t db3_rows_bytes(long nrows) { return align_up((size_t)nrows * D3P * sizeof(double), 256); }
__host__ __device__ inline long db3_tiles(long nrows) { return (nrows + 31) / 32; }
// row stride of the tile minima (M x stride floats): whole float4s, read into registers by
// the exact stage in one round trip (the pad entries are never written nor read as minima)
__host__ __device__ constexpr int c3_stride(int ntiles) { return (ntiles + 3) & ~3; }
static inline size_t db3_split_bytes(long nrows) { return (size_t)db3_tiles(nrows) * C16_TILE * sizeof(half8); }
static inline Db3View db3_view(void *base, long nrows) {
    char *b = reinterpret_cast<char *>(base);
    Db3View v;
    v.rows = reinterpret_cast<double *>(b);
    v.db16 = reinterpret_cast<half8 *>(b + db3_rows_bytes(nrows));
    v.meta = reinterpret_cast<Col16Meta *>(b + db3_rows_bytes(nrows) + db3_split_bytes(nrows));
    v.ntiles = db3_tiles(nrows);
    return v;
}

__device__ __forceinline__ unsigned long long c3key(double x) {   // order-preserving key
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ULL);
}
__device__ __forceinline__ double c3key_inv(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffULL) : ~k));
}

// per-feature range of the rows: thread k of a block scans RB rows of feature k
constexpr int C3_RB = 1024;
__global__ __launch_bounds__(D3P) void k_db3_range(const double *__restrict__ rows, long nrows,
                                                   Col16Meta *__restrict__ meta) {
    const int k = threadIdx.x;
    if (k >= D3) return;
    const long r0 = (long)blockIdx.x * C3_RB;
    const long r1 = r0 + C3_RB < nrows ? r0 + C3_RB : nrows;
    double lo = INFINITY, hi = -INFINITY;
    for (long r = r0; r < r1; ++r) {
        const double v = rows[r * D3P + k];
        lo = fmin(lo, v);
        hi = fmax(hi, v);
    }
    atomicMin(&meta->rng[2 * k], c3key(lo));
    atomicMin(&meta->rng[2 * k + 1], c3key(-hi));
}

// the centre (midrange) into LDS from the range keys
__device__ __forceinline__ void c3_center(const Col16Meta *meta, double *cs) {
    for (int k = threadIdx.x; k < D3P; k += blockDim.x)
        cs[k] = k < D3 ? 0.5 * (c3key_inv(meta->rng[2 * k]) - c3key_inv(meta->rng[2 * k + 1])) : 0.0;
}

__device__ __forceinline__ double c3_norm(const double *a, const double *cs) {
    double n = 0.0;
#pragma unroll 5
    for (int k = 0; k < D3; ++k) {
        const double d = a[k] - cs[k];
        n = fma(d, d, n);
    }
    return n;
}

// A: max over rows of |a'| rounded up to fp32 (one thread per row); block 0 stores the centre
__global__ __launch_bounds__(256) void k_db3_bound(const double *__restrict__ rows, long nrows,
                                                   Col16Meta *__restrict__ meta) {
    __shared__ double cs[D3P];
    __shared__ float red[4];
    c3_center(meta, cs);
    __syncthreads();
    if (blockIdx.x == 0)
        for (int k = threadIdx.x; k < D3P; k += 256) meta->center[k] = cs[k];
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    float a = 0.f;
    if (r < nrows) {
        const double n = c3_norm(rows + r * D3P, cs);
        a = (float)sqrt(n);
        if ((double)a * (double)a < n) a = nextafterf(a, INFINITY);
        a = nextafterf(a, INFINITY);   // the fp64 norm's own rounding
    }
    for (int o = 32; o > 0; o >>= 1) a = fmaxf(a, __shfl_xor(a, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0)
        atomicMax(&meta->amax_bits, __float_as_uint(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]))));
}

// the split rows, one thread per row (rows >= nrows repeat the last row): 22 half8 per row,
// lanes of consecutive rows writing consecutive 16 B
__global__ __launch_bounds__(256) void k_db3_split(const double *__restrict__ rows, long nrows,
                                                   const Col16Meta *__restrict__ meta,
                                                   half8 *__restrict__ db16) {
    __shared__ double cs[D3P];
    for (int k = threadIdx.x; k < D3P; k += 256) cs[k] = meta->center[k];
    __syncthreads();
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r >= db3_tiles(nrows) * 32) return;
    const double *a = rows + (r < nrows ? r : nrows - 1) * D3P;
    const float amax = __uint_as_float(meta->amax_bits);
    const Split16Db sc = split16_db_scale(amax);
    const double nrm = c3_norm(a, cs);
    half8 *t = db16 + (r >> 5) * C16_TILE + (r & 31);
#pragma unroll 1
    for (int c = 0; c < C16_CH; ++c)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            half8 vh, vl;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int k = 16 * c + 8 * h + e;
                double x = 0.0;
                if (k < D3) x = ldexp(a[k] - cs[k], sc.ea);
                else if (k == D3) x = ldexp((double)(float)nrm, sc.ea - sc.R);
                _Float16 xh, xl;
                split16d(x, xh, xl);
                vh[e] = xh;
                vl[e] = xl;
            }
            t[c16_at(c, 0, h, 0)] = vh;
            t[c16_at(c, 1, h, 0)] = vl;
        }
}

// the split operand of query m (q16) and |q'|^2 (qn) from thread k's feature v (256
// threads; m >= M: zero columns)
__device__ __forceinline__ void c3_query_split(int m, int M, int k, double v, const Col16Meta *meta,
                                               double *qn, _Float16 *q16, double *red) {
    _Float16 *qt = q16 + (long)(m >> 5) * C16_TILE * 8;
    const int col = m & 31;
    auto put = [&](int slot, _Float16 h, _Float16 l) {
        const int c = slot >> 4, hh = (slot >> 3) & 1, e = slot & 7;
        qt[c16_at(c, 0, hh, col) * 8 + e] = h;
        qt[c16_at(c, 1, hh, col) * 8 + e] = l;
    };
    if (m >= M) {
        if (k < C3_NSLOT) put(k, (_Float16)0.f, (_Float16)0.f);
        return;
    }
    const double d = k < D3 ? v - meta->center[k] : 0.0;
    double n = d * d;
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
    if ((k & 63) == 0) red[k >> 6] = n;
    __syncthreads();
    const double nq = (red[0] + red[1]) + (red[2] + red[3]);
    if (k == 0) qn[m] = nq;
    if (k < C3_NSLOT) {
        const Split16Db sc = split16_db_scale(__uint_as_float(meta->amax_bits));
        const int eq = split16_q_scale(nq, sc.R);
        double b = 0.0;
        if (k < D3) b = ldexp(-2.0 * d, eq);
        else if (k == D3) b = ldexp(1.0, eq + sc.R);
        _Float16 h, l;
        split16d(b, h, l);
        put(k, h, l);
    }
}

// queries of wave t for the split-f16 screen: the fp64 row (q3, as k_query3), |q'|^2 (qn)
// and the split operand (q16); blocks M .. Mpad-1 zero their query columns
__global__ __launch_bounds__(256) void k_query3s(Img3 Bsm, Img3 Blg, Img3 Bpsm, Img3 Bplg, int t,
                                                 int y_lo, int M, const Col16Meta *__restrict__ meta,
                                                 double *__restrict__ q3, double *__restrict__ qn,
                                                 _Float16 *__restrict__ q16) {
    __shared__ double red[4];
    const int m = blockIdx.x, k = threadIdx.x;
    double v = 0.0;
    if (m < M) {
        const int y = y_lo + m, x = t - 3 * y;
        if (k < D3_FULL) v = feat3(Bsm, Blg, y, x, k);
        else if (k < D3) v = feat3(Bpsm, Bplg, y, x, k - D3_FULL);
        if (k < D3P) q3[(long)m * D3P + k] = v;
    }
    c3_query_split(m, M, k, v, meta, qn, q16, red);
}

// diagnostic: the split operand of given queries (M x 165)
__global__ __launch_bounds__(256) void k_qsplit3(const double *__restrict__ q165, int M,
                                                 const Col16Meta *__restrict__ meta,
                                                 double *__restrict__ qn, _Float16 *__restrict__ q16) {
    __shared__ double red[4];
    const int m = blockIdx.x, k = threadIdx.x;
    const double v = m < M && k < D3 ? q165[(long)m * D3 + k] : 0.0;
    c3_query_split(m, M, k, v, meta, qn, q16, red);
}

// diagnostic: the screen's tile minima in unscaled units (e = s / (sa sq)), eps3 per query
// (R16c: nsk, rmeta given, eps = r3_eps)
struct Rot3Meta;
__device__ double r3_eps_m(const Rot3Meta *rm, double A, double nqq, double nsk);
__global__ void k_screen3_unscale(const float *__restrict__ smin, int M, int ntiles,
                                  const double *__restrict__ qn, const Col16Meta *__restrict__ meta,
                                  double *__restrict__ e, double *__restrict__ eps,
                                  const double *__restrict__ nsk = nullptr, const Rot3Meta *rm = nullptr) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)M * ntiles) return;
    const int m = (int)(i / ntiles), tl = (int)(i - (long)m * ntiles);
    const float amax = __uint_as_float(meta->amax_bits);
    const Split16Db sc = split16_db_scale(amax);
    const int eq = split16_q_scale(qn[m], sc.R);
    e[i] = ldexp((double)smin[(long)m * c3_stride(ntiles) + tl], -(sc.ea + eq));
    if (i % ntiles == 0) {
        constexpr double U32 = 5.9604644775390625e-08;
        const double A = (double)amax;
        eps[m] = nsk ? r3_eps_m(rm, A, qn[m], nsk[m]) : U32 * (900.0 * A * sqrt(qn[m]) + 450.0 * A * A);
    }
}

// the screen: block (x, query group y) of 4 waves.  The group's query tiles (up to S3_QG)
// are staged in LDS once; each wave then walks row tiles t = (x tpw + i) 4 + wave, holding
// the tile's 22 operand groups in registers (the next tile's loaded while this one's chains
// run) against every staged query tile: 33 MFMAs per (row tile, query tile), and per query
// the minimum over the tile's 32 rows.  Each DB tile is read once per query group (round 4's
// first form read it once per query tile: 7 times per wave at the c3 size).
constexpr int S3_QG = 4;                  // query tiles per group (LDS: 4 x 22.5 KB)
__device__ __forceinline__ void s3_load(const half8 *db16, int t, int lane, half8 (&ah)[C16_CH],
                                        half8 (&al)[C16_CH]) {
    const half8 *db = db16 + (long)t * C16_TILE + lane;
#pragma unroll
    for (int c = 0; c < C16_CH; ++c) {
        ah[c] = db[(2 * c) * 64];
        al[c] = db[(2 * c + 1) * 64];
    }
}
__global__ __launch_bounds__(256, 1) void k_screen3(const half8 *__restrict__ db16, int ntiles,
                                                    const half8 *__restrict__ q16, int M, int tpw,
                                                    float *__restrict__ smin) {
    __shared__ half8 qsh[S3_QG * C16_TILE];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int qt0 = blockIdx.y * S3_QG;
    const int QT = (M + 31) / 32;
    const int nq = QT - qt0 < S3_QG ? QT - qt0 : S3_QG;
    for (int i = threadIdx.x; i < nq * C16_TILE; i += 256) qsh[i] = q16[(long)qt0 * C16_TILE + i];
    __syncthreads();
    const floatx16 zero = {};
    const int tb = blockIdx.x * tpw * 4 + wv;
    int t = tb;
    if (t >= ntiles) return;   // (after the only barrier)
    half8 ah[C16_CH], al[C16_CH], nh[C16_CH], nl[C16_CH];
    s3_load(db16, t, lane, ah, al);
    for (int it = 0; it < tpw; ++it, t += 4) {
        const int tn = t + 4;
        const bool more = it + 1 < tpw && tn < ntiles;
        if (more) s3_load(db16, tn, lane, nh, nl);
        for (int j = 0; j < nq; ++j) {
            const half8 *qb = qsh + j * C16_TILE + lane;
            floatx16 acc = zero;
#pragma unroll
            for (int c = 0; c < C16_CH; ++c) {
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[c], qb[(2 * c + 1) * 64], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[c], qb[(2 * c) * 64], acc, 0, 0, 0);
            }
#pragma unroll
            for (int c = 0; c < C16_CH; ++c)
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[c], qb[(2 * c) * 64], acc, 0, 0, 0);
            float mn = acc[0];
#pragma unroll
            for (int i = 1; i < 16; ++i) mn = fminf(mn, acc[i]);
            mn = fminf(mn, __shfl_xor(mn, 32));
            const int q = (qt0 + j) * 32 + lane;
            if (lane < 32 && q < M) smin[(long)q * c3_stride(ntiles) + t] = mn;
        }
        if (!more) break;
#pragma unroll
        for (int c = 0; c < C16_CH; ++c) {
            ah[c] = nh[c];
            al[c] = nl[c];
        }
    }
}

// grid of k_screen3: row tiles per wave so that about 512 workgroups cover the
// (row tile, query group) pairs
static inline dim3 screen3_grid(int ntiles, int M, int &tpw) {
    const int QG = ((M + 31) / 32 + S3_QG - 1) / S3_QG;
    tpw = (int)std::max(1L, ((long)ntiles * QG + 4L * 512 - 1) / (4L * 512));
    return dim3((unsigned)((ntiles + 4 * tpw - 1) / (4 * tpw)), (unsigned)QG);
}

// ---- the rotated split screen for 3-channel rows (R16c) -----------------
// As ia_rot16.h for D = 165: per level the principal directions V (165 x 165, fp32, host
// eigh of the centred rows' covariance), rows rho = V^T a', queries kappa = V^T q'; the top
// R3_P components keep f16 split pairs (three products), the other 162 one f16 product, the
// norm its split pair: 2P cross slots, norm_lo, 165 main slots, norm_hi, zeros -> 176 slots =
// 11 MFMAs per 32x32 tile (33 in k_screen3), 352 B per row (704).  Same scales and units as
// §4c; the bound adds the skipped components' dropped cross terms (A_skip, |kappa_skip|).
constexpr int R3_P = 3;
constexpr int R3_NL = 2 * R3_P, R3_M0 = R3_NL + 1, R3_NH = R3_M0 + D3;   // 6, 7, 172
constexpr int R3_SLOTS = (R3_NH + 16) / 16 * 16;                           // 176
constexpr int R3_MFMA = R3_SLOTS / 16;                                     // 11
constexpr int R3_TILE = R3_MFMA * 64;                                      // half8 per tile
constexpr int R3_LD = 168;                                                 // rot[k * R3_LD + j]
constexpr int R3_ROT_FLOATS = D3 * R3_LD;
static_assert(R3_MFMA == 11, "R16c: 11 MFMAs per tile at P = 3");
// half8 index of slot s of tile row (or query column) j, and its element s & 7
__host__ __device__ constexpr int r3_h8(int s, int j) { return (s >> 4) * 64 + ((s & 15) >> 3) * 32 + j; }

struct Rot3Meta {   // after the rotated tiles: A_skip (fp32 bits, rounded up; atomicMax)
    unsigned int askip_bits;
    unsigned int pad[63];
};
static inline size_t db3r_tiles_bytes(long nrows) { return align_up((size_t)db3_tiles(nrows) * R3_TILE * sizeof(half8), 256); }
static inline Rot3Meta *db3r_meta(void *dbr, long nrows) {
    return reinterpret_cast<Rot3Meta *>(reinterpret_cast<char *>(dbr) + db3r_tiles_bytes(nrows));
}

// the rotated tiles: one 256-thread block per 32-row tile (rows past nrows repeat the last);
// V and the tile's centred rows staged in LDS; thread (row r = tid & 31, g = tid >> 5) takes
// components j = g + 8i in fp64 from the fp32 V; then the split slots through an LDS stage
// (reusing the rows' space) into the tile layout, and A_skip = max ||fl32(rho_skip)||
__global__ __launch_bounds__(256, 1) void k_db3_rot(const double *__restrict__ rows, long nrows,
                                                    const Col16Meta *__restrict__ meta,
                                                    const float *__restrict__ rot, half8 *__restrict__ dbr,
                                                    Rot3Meta *__restrict__ rmeta) {
    __shared__ __attribute__((aligned(16))) float V[R3_ROT_FLOATS];      // 110,880 B
    __shared__ __attribute__((aligned(16))) double X[32 * D3];          // 42,240 B (odd row stride)
    __shared__ double skp[32][8];
    __shared__ double nrm[32];
    __shared__ float red[4];
    const int tid = threadIdx.x, r = tid & 31, g = tid >> 5;
    for (int i = tid; i < R3_ROT_FLOATS / 4; i += 256)
        reinterpret_cast<float4 *>(V)[i] = reinterpret_cast<const float4 *>(rot)[i];
    const long t = blockIdx.x;
    for (int i = tid; i < 32 * D3; i += 256) {
        const int rr = i / D3, k = i - rr * D3;
        const long row = t * 32 + rr < nrows ? t * 32 + rr : nrows - 1;
        X[i] = rows[row * D3P + k] - meta->center[k];
    }
    __syncthreads();
    constexpr int NJ = (D3 + 7) / 8;   // 21 components per thread
    double acc[NJ];
#pragma unroll
    for (int i = 0; i < NJ; ++i) acc[i] = 0.0;
    double n2 = 0.0;
    for (int k = 0; k < D3; ++k) {
        const double dk = X[r * D3 + k];
        if (g == 0) n2 += dk * dk;
#pragma unroll
        for (int i = 0; i < NJ; ++i) {
            const int j = g + 8 * i;
            if (j < D3) acc[i] = fma((double)V[k * R3_LD + j], dk, acc[i]);
        }
    }
    __syncthreads();   // every read of X done: it becomes the slot stage
    _Float16 *stage = reinterpret_cast<_Float16 *>(X);   // [32][R3_SLOTS]
    const Split16Db sc = split16_db_scale(__uint_as_float(meta->amax_bits));
    double sk = 0.0;
#pragma unroll
    for (int i = 0; i < NJ; ++i) {
        const int j = g + 8 * i;
        if (j >= D3) continue;
        const float r32 = (float)acc[i];
        if (j >= R3_P) sk += (double)r32 * (double)r32;
        _Float16 h, l;
        split16f(ldexpf(r32, sc.ea), h, l);
        stage[r * R3_SLOTS + R3_M0 + j] = h;
        if (j < R3_P) {
            stage[r * R3_SLOTS + 2 * j] = l;
            stage[r * R3_SLOTS + 2 * j + 1] = h;
        }
    }
    skp[r][g] = sk;
    if (g == 0) nrm[r] = n2;
    __syncthreads();
    float askip = 0.f;
    if (g == 0) {
        _Float16 nh, nl;
        split16f(ldexpf((float)nrm[r], sc.ea - sc.R), nh, nl);
        stage[r * R3_SLOTS + R3_NL] = nl;
        stage[r * R3_SLOTS + R3_NH] = nh;
        for (int z = R3_NH + 1; z < R3_SLOTS; ++z) stage[r * R3_SLOTS + z] = (_Float16)0.f;
        double s = 0.0;
        for (int q = 0; q < 8; ++q) s += skp[r][q];
        const double a = sqrt(s * (1.0 + 1e-12));
        askip = (float)a;
        if ((double)askip < a) askip = nextafterf(askip, INFINITY);
    }
    for (int o = 32; o > 0; o >>= 1) askip = fmaxf(askip, __shfl_xor(askip, o));
    if ((tid & 63) == 0) red[tid >> 6] = askip;
    __syncthreads();
    if (tid == 0)
        atomicMax(&rmeta->askip_bits, __float_as_uint(fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]))));
    // the tile layout: half8 (m, hh, j) = slots 16 m + 8 hh .. +7 of row j
    half8 *out = dbr + t * R3_TILE;
    for (int i = tid; i < R3_TILE; i += 256) {
        const int m = i >> 6, hh = (i >> 5) & 1, j = i & 31;
        out[i] = *reinterpret_cast<const half8 *>(&stage[j * R3_SLOTS + 16 * m + 8 * hh]);
    }
}

// ---- the covariance of a 3-channel level's rows (ia_db3_cov, rot3_build's matrix) -------
// ~64 k rows sampled every `step` (rot3_build's rows[::max(1, N // 65536)]), centred at their
// mean, fp64: column sums per sample slice, the mean, then per (16 output rows a, slice) the
// centred products with every column b, 32 sampled rows staged in LDS at a time; partials
// reduced in slice order (deterministic).  Any orthonormal basis keeps the matcher exact; the
// principal one of this matrix keeps its bound tight.
constexpr int C3C_SPLIT = 128, C3C_AB = 16, C3C_NA = (D3 + C3C_AB - 1) / C3C_AB, C3C_TR = 32;
__global__ __launch_bounds__(256) void k_db3_colsum(const double *__restrict__ rows, long step, long nsamp,
                                                    double *__restrict__ part) {
    __shared__ double X[C3C_TR][D3P];
    const int t = threadIdx.x, sl = blockIdx.x;
    const long i0 = nsamp * sl / C3C_SPLIT, i1 = nsamp * (sl + 1) / C3C_SPLIT;
    double acc = 0.0;
    for (long r0 = i0; r0 < i1; r0 += C3C_TR) {
        __syncthreads();
        for (int e = t; e < C3C_TR * D3P; e += 256) {
            const int rr = e / D3P, k = e - rr * D3P;
            const long i = r0 + rr;
            X[rr][k] = i < i1 ? rows[i * step * D3P + k] : 0.0;
        }
        __syncthreads();
        if (t < D3)
            for (int rr = 0; rr < C3C_TR; ++rr) acc += X[rr][t];
    }
    if (t < D3P) part[sl * D3P + t] = t < D3 ? acc : 0.0;
}
__global__ __launch_bounds__(256) void k_db3_mean(const double *__restrict__ part, long nsamp, double *__restrict__ mean) {
    const int t = threadIdx.x;
    if (t >= D3P) return;
    double acc = 0.0;
    for (int sl = 0; sl < C3C_SPLIT; ++sl) acc += part[sl * D3P + t];
    mean[t] = t < D3 ? acc / (double)nsamp : 0.0;
}
__global__ __launch_bounds__(256) void k_db3_cov(const double *__restrict__ rows, long step, long nsamp,
                                                 const double *__restrict__ mean, double *__restrict__ part) {
    __shared__ double X[C3C_TR][D3P];
    const int t = threadIdx.x, a0 = blockIdx.x * C3C_AB, sl = blockIdx.y;
    const long i0 = nsamp * sl / C3C_SPLIT, i1 = nsamp * (sl + 1) / C3C_SPLIT;
    double acc[C3C_AB];
#pragma unroll
    for (int j = 0; j < C3C_AB; ++j) acc[j] = 0.0;
    const double mu = t < D3 ? mean[t] : 0.0;
    for (long r0 = i0; r0 < i1; r0 += C3C_TR) {
        __syncthreads();
        for (int e = t; e < C3C_TR * D3P; e += 256) {
            const int rr = e / D3P, k = e - rr * D3P;
            const long i = r0 + rr;
            X[rr][k] = i < i1 && k < D3 ? rows[i * step * D3P + k] - mean[k] : 0.0;
        }
        __syncthreads();
        if (t < D3) {
            for (int rr = 0; rr < C3C_TR; ++rr) {
                const double xb = X[rr][t];
#pragma unroll
                for (int j = 0; j < C3C_AB; ++j) acc[j] += X[rr][a0 + j < D3 ? a0 + j : 0] * xb;
            }
        }
    }
    (void)mu;
    if (t < D3) {
#pragma unroll
        for (int j = 0; j < C3C_AB; ++j)
            if (a0 + j < D3) part[((long)sl * D3 + a0 + j) * D3P + t] = acc[j];
    }
}
__global__ __launch_bounds__(256) void k_db3_cov_reduce(const double *__restrict__ part, double *__restrict__ cov) {
    const int a = blockIdx.x, t = threadIdx.x;
    if (t >= D3P) return;
    double acc = 0.0;
    if (t < D3)
        for (int sl = 0; sl < C3C_SPLIT; ++sl) acc += part[((long)sl * D3 + a) * D3P + t];
    cov[(long)a * D3P + t] = acc;
}

// the R16c query operand of query m from thread k's centred feature d (256 threads):
// kappa_j = sum_k V[k][j] d_k (thread j, fp64 from the fp32 V in global memory), |q'|^2 ->
// qn, |kappa_skip|^2 -> nsk, the slots into the query tile (m >= M: zero columns)
__device__ __forceinline__ void r3_query(int m, int M, int k, double v, const Col16Meta *meta,
                                         const float *__restrict__ rot, double *qn, double *nsk,
                                         half8 *q16, double *ds, double *red) {
    _Float16 *qt = reinterpret_cast<_Float16 *>(q16 + (long)(m >> 5) * R3_TILE);
    const int col = m & 31;
    auto put = [&](int slot, _Float16 x) { qt[r3_h8(slot, col) * 8 + (slot & 7)] = x; };
    if (m >= M) {
        if (k < R3_SLOTS) put(k, (_Float16)0.f);
        return;
    }
    const double d = k < D3 ? v - meta->center[k] : 0.0;
    if (k < D3) ds[k] = d;
    double n = d * d;
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
    if ((k & 63) == 0) red[k >> 6] = n;
    __syncthreads();
    const double nq = (red[0] + red[1]) + (red[2] + red[3]);
    double kap = 0.0;
    if (k < D3) {
        double k0 = 0.0, k1 = 0.0, k2 = 0.0, k3 = 0.0;
        int i = 0;
        // unrolled: the loads of V (L2-resident) issue far ahead of their FMAs
#pragma unroll 10
        for (; i + 4 <= D3; i += 4) {
            k0 = fma((double)rot[(i + 0) * R3_LD + k], ds[i + 0], k0);
            k1 = fma((double)rot[(i + 1) * R3_LD + k], ds[i + 1], k1);
            k2 = fma((double)rot[(i + 2) * R3_LD + k], ds[i + 2], k2);
            k3 = fma((double)rot[(i + 3) * R3_LD + k], ds[i + 3], k3);
        }
        for (; i < D3; ++i) k0 = fma((double)rot[i * R3_LD + k], ds[i], k0);
        kap = (k0 + k1) + (k2 + k3);
    }
    double s2 = k >= R3_P && k < D3 ? kap * kap : 0.0;
    for (int o = 32; o > 0; o >>= 1) s2 += __shfl_xor(s2, o);
    __syncthreads();   // red reused
    if ((k & 63) == 0) red[k >> 6] = s2;
    __syncthreads();
    if (k == 0) {
        qn[m] = nq;
        nsk[m] = (red[0] + red[1]) + (red[2] + red[3]);
    }
    const Split16Db sc = split16_db_scale(__uint_as_float(meta->amax_bits));
    const int eq = split16_q_scale(nq, sc.R);
    if (k < D3) {
        _Float16 h, l;
        split16d(ldexp(-2.0 * kap, eq), h, l);
        put(R3_M0 + k, h);
        if (k < R3_P) {
            put(2 * k, h);
            put(2 * k + 1, l);
        }
    } else if (k == D3) {
        const _Float16 nn = (_Float16)ldexpf(1.f, eq + sc.R);
        put(R3_NL, nn);
        put(R3_NH, nn);
    } else if (R3_NH + (k - D3) < R3_SLOTS) {
        put(R3_NH + (k - D3), (_Float16)0.f);
    }
}

// queries of wave t for the R16c screen (as k_query3s; qin: caller-given rows, diagnostics):
// the body of k_query3r (one job, by-value arguments) and k_query3rb (a batch, job table)
__device__ __forceinline__ void query3r_body(const Img3 &Bsm, const Img3 &Blg, const Img3 &Bpsm,
                                             const Img3 &Bplg, int t, int y_lo, int M,
                                             const Col16Meta *__restrict__ meta,
                                             const float *__restrict__ rot, const double *__restrict__ qin,
                                             double *__restrict__ q3, double *__restrict__ qn,
                                             double *__restrict__ nsk, half8 *__restrict__ q16) {
    __shared__ double red[4];
    __shared__ double ds[D3];
    const int m = blockIdx.x, k = threadIdx.x;
    double v = 0.0;
    if (m < M) {
        if (qin) {
            v = k < D3 ? qin[(long)m * D3 + k] : 0.0;
        } else {
            const int y = y_lo + m, x = t - 3 * y;
            if (k < D3_FULL) v = feat3(Bsm, Blg, y, x, k);
            else if (k < D3) v = feat3(Bpsm, Bplg, y, x, k - D3_FULL);
            if (k < D3P) q3[(long)m * D3P + k] = v;
        }
    }
    r3_query(m, M, k, v, meta, rot, qn, nsk, q16, ds, red);
}
__global__ __launch_bounds__(256) void k_query3r(Img3 Bsm, Img3 Blg, Img3 Bpsm, Img3 Bplg, int t,
                                                 int y_lo, int M, const Col16Meta *__restrict__ meta,
                                                 const float *__restrict__ rot, const double *__restrict__ qin,
                                                 double *__restrict__ q3, double *__restrict__ qn,
                                                 double *__restrict__ nsk, half8 *__restrict__ q16) {
    query3r_body(Bsm, Blg, Bpsm, Bplg, t, y_lo, M, meta, rot, qin, q3, qn, nsk, q16);
}

// the R16c screen: as k_screen3 with 11 operand groups per tile and 11 MFMAs per (row tile,
// query tile); up to 8 query tiles staged per workgroup (a c3 wave's 213 queries: one group,
// each DB tile read once per wave)
// 7 query tiles per group (a c3 wave's <= 213 queries: one group; LDS 77 KiB, two workgroups
// per CU: the grid's ~450 workgroups in one round instead of two)
constexpr int S3R_QG = 7;
// The row-tile loop of the R16c screens: the workgroup's nq staged query tiles (qsh) against this
// wave's row tiles.  QS says whose queries the staged tiles are: q0(j), tile j's first query,
// and smin(j), the minima it writes to.  S3One: consecutive tiles of one job (k_screen3r, and
// k_screen3rb per job of a batch); S3Tab: tiles of several jobs passing one database, looked
// up per staged entry (k_screen3rs).  QS is passed by value and its members are the
// expressions the kernels had in place, term for term: k_screen3r's and k_screen3rb's
// instructions are those of the bodies written out (checked instruction by instruction on the
// gfx950 assembly, profiles/screen_loop_isa.txt; tests/test_gpu_color3_shared.py pins the registers)
struct S3One {
    int qt0;
    float *__restrict__ sm;
    __device__ __forceinline__ int q0(int j) const { return (qt0 + j) * 32; }
    __device__ __forceinline__ float *smin(int) const { return sm; }
};
struct S3Tab {
    const int *q0_sh;                // per staged entry: its first query
    const gptr<float> *smin_sh;      // and its job's minima (gptr: global accesses)
    __device__ __forceinline__ int q0(int j) const { return q0_sh[j]; }
    __device__ __forceinline__ float *smin(int j) const { return smin_sh[j].p; }
};
template <typename QS>
__device__ __forceinline__ void screen3r_rows(const half8 *__restrict__ db16, int ntiles, int M, int tpw,
                                              const half8 *qsh, int nq, const QS qs) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const floatx16 zero = {};
    int t = blockIdx.x * tpw * 4 + wv;
    if (t >= ntiles) return;   // (after the last barrier)
    half8 a[R3_MFMA], n[R3_MFMA];
#pragma unroll
    for (int c = 0; c < R3_MFMA; ++c) a[c] = db16[(long)t * R3_TILE + c * 64 + lane];
    for (int it = 0; it < tpw; ++it, t += 4) {
        const int tn = t + 4;
        const bool more = it + 1 < tpw && tn < ntiles;
        if (more)
#pragma unroll
            for (int c = 0; c < R3_MFMA; ++c) n[c] = db16[(long)tn * R3_TILE + c * 64 + lane];
        // two query tiles per pass: both tiles' 22 operand reads issued first, the two
        // accumulation chains interleaved (each MFMA's operand and the other chain's MFMA
        // cover one another's latency; one wave per SIMD here), then both folds
        for (int j = 0; j < nq; j += 2) {
            const int j1 = j + 1 < nq ? j + 1 : j;
            const half8 *qb0 = qsh + j * R3_TILE + lane, *qb1 = qsh + j1 * R3_TILE + lane;
            half8 b0[R3_MFMA], b1[R3_MFMA];
#pragma unroll
            for (int c = 0; c < R3_MFMA; ++c) {
                b0[c] = qb0[c * 64];
                b1[c] = qb1[c * 64];
            }
            floatx16 acc0 = zero, acc1 = zero;
#pragma unroll
            for (int c = 0; c < R3_MFMA; ++c) {
                acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[c], b0[c], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[c], b1[c], acc1, 0, 0, 0);
            }
            float mn0 = acc0[0], mn1 = acc1[0];
#pragma unroll
            for (int i = 1; i < 16; ++i) {
                mn0 = fminf(mn0, acc0[i]);
                mn1 = fminf(mn1, acc1[i]);
            }
            mn0 = fminf(mn0, __shfl_xor(mn0, 32));
            mn1 = fminf(mn1, __shfl_xor(mn1, 32));
            const int q0 = qs.q0(j) + lane, q1 = qs.q0(j1) + lane;
            if (lane < 32 && q0 < M) qs.smin(j)[(long)q0 * c3_stride(ntiles) + t] = mn0;
            if (lane < 32 && j1 != j && q1 < M) qs.smin(j1)[(long)q1 * c3_stride(ntiles) + t] = mn1;
        }
        if (!more) break;
#pragma unroll
        for (int c = 0; c < R3_MFMA; ++c) a[c] = n[c];
    }
}
// (screen3r_body: the body of k_screen3r, one job, and k_screen3rb, a batch)
__device__ __forceinline__ void screen3r_body(const half8 *__restrict__ db16, int ntiles,
                                              const half8 *__restrict__ q16, int M, int tpw,
                                              float *__restrict__ smin) {
    __shared__ half8 qsh[S3R_QG * R3_TILE];
    const int qt0 = blockIdx.y * S3R_QG;
    const int QT = (M + 31) / 32;
    const int nq = QT - qt0 < S3R_QG ? QT - qt0 : S3R_QG;
    for (int i = threadIdx.x; i < nq * R3_TILE; i += 256) qsh[i] = q16[(long)qt0 * R3_TILE + i];
    __syncthreads();   // (the only barrier)
    screen3r_rows(db16, ntiles, M, tpw, qsh, nq, S3One{qt0, smin});
}
__global__ __launch_bounds__(256, 2) void k_screen3r(const half8 *__restrict__ db16, int ntiles,
                                                     const half8 *__restrict__ q16, int M, int tpw,
                                                     float *__restrict__ smin) {
    screen3r_body(db16, ntiles, q16, M, tpw, smin);
}
// the grid: row tiles per wave (tpw) so that about 512 workgroups cover the (row tile, query
// group, job) triples of the whole launch (K jobs: grid z); the tile minima do not depend on tpw
static inline dim3 screen3r_grid(int ntiles, int M, int &tpw, int K = 1) {
    const int QG = ((M + 31) / 32 + S3R_QG - 1) / S3R_QG;
    tpw = (int)std::max(1L, ((long)ntiles * QG * K + 4L * 512 - 1) / (4L * 512));
    return dim3((unsigned)((ntiles + 4 * tpw - 1) / (4 * tpw)), (unsigned)QG, (unsigned)K);
}
// the grid of k_screen3rs: y covers the longest group's query groups (qg_max), z the G groups;
// tpw from the launch's qg_total (row tile, query group) pairs per row tile, the same aim
static inline dim3 screen3rs_grid(int ntiles, int qg_total, int qg_max, int G, int &tpw) {
    tpw = (int)std::max(1L, ((long)ntiles * qg_total + 4L * 512 - 1) / (4L * 512));
    return dim3((unsigned)((ntiles + 4 * tpw - 1) / (4 * tpw)), (unsigned)qg_max, (unsigned)G);
}

// eps of the R16c screen: u (850 A|q'| + 60 A^2) + 2^-9 1.01 A_skip |kappa_skip|
__device__ __forceinline__ double r3_eps(double A, double nqq, double askip, double nsk) {
    constexpr double U32 = 5.9604644775390625e-08;
    return U32 * (850.0 * A * sqrt(nqq) + 60.0 * A * A) + 0x1p-9 * 1.01 * askip * sqrt(nsk);
}
__device__ double r3_eps_m(const Rot3Meta *rm, double A, double nqq, double nsk) {
    return r3_eps(A, nqq, (double)__uint_as_float(rm->askip_bits), nsk);
}

// exhaustive fp64 search: a block takes 32 rows (staged in LDS) against every query, 8 at
// a time; thread (row tid / 8, query tid % 8) computes the oracle's distance; per query the
// block's lexicographic (distance, row) minimum -> part[query][block]
constexpr int M3_ROWS = 32, M3_Q = 8;
__global__ __launch_bounds__(256) void k_match3(const double *__restrict__ db3, long nrows, long row0,
                                                const double *__restrict__ q3, int M,
                                                Best *__restrict__ part) {
    __shared__ double rows[M3_ROWS * D3P];
    __shared__ double qs[M3_Q * D3P];
    __shared__ double cd[M3_Q][M3_ROWS];
    const long r0 = (long)blockIdx.x * M3_ROWS;
    const int nb = gridDim.x;
    for (int i = threadIdx.x; i < M3_ROWS * D3P; i += 256) {
        const long r = r0 + i / D3P;
        rows[i] = r < nrows ? db3[r0 * D3P + i] : 0.0;
    }
    const int rl = threadIdx.x >> 3, ql = threadIdx.x & 7;
    for (int q0 = 0; q0 < M; q0 += M3_Q) {
        __syncthreads();   // rows staged / the previous group's candidates consumed
        for (int i = threadIdx.x; i < M3_Q * D3P; i += 256) {
            const int q = q0 + i / D3P;
            qs[i] = q < M ? q3[(long)q0 * D3P + i] : 0.0;
        }
        __syncthreads();
        Pw165 pw;
        const double *a = rows + rl * D3P, *b = qs + ql * D3P;
#pragma unroll
        for (int k = 0; k < D3; ++k) {
            const double d = a[k] - b[k];
            pw.feed(k, d * d);
        }
        cd[ql][rl] = r0 + rl < nrows ? pw.result() : INFINITY;
        __syncthreads();
        if (threadIdx.x < M3_Q && q0 + threadIdx.x < M) {
            double bd = INFINITY;
            long long bi = 0x7fffffffffffffffLL;
            for (int r = 0; r < M3_ROWS; ++r) {
                const double d = cd[threadIdx.x][r];
                if (d < bd) { bd = d; bi = row0 + r0 + r; }   // rows ascending: first minimum
            }
            part[(long)(q0 + threadIdx.x) * nb + blockIdx.x] = Best{bd, bi};
        }
    }
}

// per query: the minimum over the blocks' partials (one block per query)
__global__ __launch_bounds__(256) void k_reduce3(const Best *__restrict__ part, int nb,
                                                 Best *__restrict__ best) {
    __shared__ double sd[4];
    __shared__ long long si[4];
    const Best b = block_best(part + (long)blockIdx.x * nb, nb, sd, si);
    if (threadIdx.x == 0) best[blockIdx.x] = b;
}

int comm_allgather(void *comm, const void *send, void *recv, size_t bytes, hipStream_t st);   // ia_comm.hip
int comm_nranks(void *comm);
PeerView comm_peer_wave(void *comm);
int comm_peer_mcap(void *comm);

struct Fin3 {
    const double *db3;       // this rank's rows of the level (local row 0 = global row0)
    const double *q3;
    const double *Ap_lg;     // nAp x Ah x Aw x 3
    int Ah, Aw;
    int t, y_lo, W;
    const double *weights;   // 165
    double kappa_factor;
    double *Bp_lg;           // H x W x 3
    int32_t *s, *im, *dbg_px;
    double *dbg_dist;
};

// The per-pixel tail of both colour tail kernels (k_exact3, k_finish3w) on the tail core of
// ia_finish.h.  Thread k < 15: window position k of pixel (y, x) into LDS (rix: its DB row,
// -1 none; rpos: row, col, A' image).
__device__ __forceinline__ void c3_window(int k, int y, int x, const Fin3 &f, long long *rix,
                                          int (*rpos)[3]) {
    const CohPos p = coh_pos(k, y, x, f.W, f.Ah, f.Aw, f.s, f.im);
    rix[k] = p.row;
    rpos[k][0] = p.r; rpos[k][1] = p.c; rpos[k][2] = p.im;
}
// One whole wave, once the window rows' distances are in LDS (sump: sqrt of the plain sum,
// +inf where rix < 0; sumw: weighted) and the exact winner app with its weighted distance
// d_app is known: the coherence pick, the kappa test, s / im and the debug record.  Returns
// the offset in Ap_lg of the chosen pixel's three channels (the B' store is the caller's).
__device__ __forceinline__ long c3_decide(const Fin3 &f, int y, int x, int lane, long long app,
                                          double d_app, const double *sump, const double *sumw,
                                          const long long *rix, const int (*rpos)[3]) {
    int win;
    const bool valid = coh_first_min(lane < 15 ? sump[lane] : INFINITY, lane, win);
    const CohSel c = coh_sel(CohPos{rix[win], rpos[win][0], rpos[win][1], rpos[win][2]}, win, valid,
                             y, x, sumw[win]);
    const long hw = (long)f.Ah * f.Aw;
    const TailSel p = kappa_pick(app, hw, f.Aw, d_app, c, f.kappa_factor);
    if (lane == 0) tail_record((long)y * f.W + x, p, c, d_app, f.s, f.im, f.dbg_px, f.dbg_dist);
    return (p.img * hw + (long)p.pr * f.Aw + p.pc) * 3;
}

// the exact stage's inputs on the split-f16 screen: per (query, row tile) minima, |q'|^2
struct Scr3 {
    const float *smin;       // M x ntiles
    int ntiles;
    long nrows;
    const double *qn;
    const Col16Meta *meta;
    unsigned long long *stats;   // [candidate tiles, full scans] (diagnostic, may be null)
    const double *nsk;           // R16c: |kappa_skip|^2 per query (null: the split-f16 screen)
    const Rot3Meta *rmeta;       // R16c: A_skip
};

// Thresholds of the colour exact stage: Tseg = e* + 2 eps3 in screen units,
// eps3 = u (900 A|q'| + 450 A^2); full scan when the norm slot nears the f16 floor
// (R16c, nsk >= 0: eps3 = r3_eps)
__device__ __forceinline__ double c3_tseg(float emin, float amax0, double nqq, bool &force_full,
                                          float askip = 0.f, double nsk = -1.0) {
    constexpr double U32 = 5.9604644775390625e-08;
    const double A = (double)amax0;
    const Split16Db sc = split16_db_scale(amax0);
    const int eq = split16_q_scale(nqq, sc.R);
    const int e2 = sc.ea + eq;
    const double em = ldexp((double)emin, -e2);
    const double eps3 = nsk >= 0.0 ? r3_eps(A, nqq, (double)askip, nsk)
                                   : U32 * (900.0 * A * sqrt(nqq) + 450.0 * A * A);
    const double slack = 1e-12 * (fabs(em) + nqq + A * A);
    force_full = eq + sc.R < -10 || split16_db_clamped(amax0);
    return ldexp(em + 2.0 * eps3 + slack, e2);
}

// ---- the exact stage + tail of the screened colour paths (k_exact3) ----------------------
// 8 threads per row: thread part j of a row holds features k = j + 8 i (i < 21), i.e. exactly
// Pw165's accumulator j of both halves (i < 10: k < 80; 10 <= i < 20: 80 <= k < 160) and,
// for j < 5, the tail term k = 160 + j.  All 21 loads issue before any use (one round trip),
// the accumulators are summed in Pw165's order in registers, and the row's part 0 finishes the
// two trees and the tail from LDS: the same value as pw165_sum, with no 165-term
// serial sum and no (row, feature) term array.
constexpr int R8_N = 21;
struct Acc8 {
    double p1, p2, pt, w1, w2, wt;   // plain / weighted: half 1, half 2, tail term
};
// thread part j's accumulators of row `row` (global fp64 rows, D3P stride) against qs / ws (LDS)
__device__ __forceinline__ Acc8 acc8_row(const double *__restrict__ row, int j, const double *qs,
                                         const double *ws) {
    double x[R8_N];
#pragma unroll
    for (int i = 0; i < R8_N; ++i) {
        const int k = j + 8 * i;
        x[i] = row[k < D3 ? k : 0];   // unconditional: every load before any use
    }
    Acc8 a{};
#pragma unroll
    for (int i = 0; i < R8_N; ++i) {
        const int k = j + 8 * i;
        const double d = x[i] - qs[k < D3 ? k : 0];
        const double dw = d * ws[k < D3 ? k : 0];
        const double tp = d * d, tw = dw * dw;
        if (i == 0) { a.p1 = tp; a.w1 = tw; }
        else if (i < 10) { a.p1 += tp; a.w1 += tw; }
        else if (i == 10) { a.p2 = tp; a.w2 = tw; }
        else if (i < 20) { a.p2 += tp; a.w2 += tw; }
        else if (k < D3) { a.pt = tp; a.wt = tw; }
    }
    return a;
}
// part 0 of a row: Pw165's value from the 8 parts' accumulators (LDS, acc[0..7])
__device__ __forceinline__ double acc8_sum(const Acc8 *acc, bool weighted) {
    double r1[8], r2[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        r1[j] = weighted ? acc[j].w1 : acc[j].p1;
        r2[j] = weighted ? acc[j].w2 : acc[j].p2;
    }
    const double h1 = Pw165::tree(r1);
    double h2 = Pw165::tree(r2);
#pragma unroll
    for (int j = 0; j < D3 - 160; ++j) h2 += weighted ? acc[j].wt : acc[j].pt;
    return h1 + h2;
}

// The exact stage of the screened paths (k_screen3 / k_screen3r) and the per-pixel tail, one
// 256-thread workgroup per pixel: the query, weights, the coherence window's s / im and the
// query's tile minima (float4s in registers) in one round trip; e* and the tiles within the
// threshold; then per candidate tile its 32 rows, 8 threads each (acc8_row: plain and weighted
// sums, so the winner's weighted distance needs no second read), with the 15 coherence rows
// in the first tile's round trip; the lexicographic (distance, row) minimum carries its
// weighted distance; coherence pick, kappa test and the record by c3_decide, then B'.
// FUSE (the R16c path, IA_C3_FUSE): the same launch also writes the query rows of wave t + 1
// (as k_query3r / r3_query; k_xwave's scheme): the workgroup of pixel (y, x)
// builds the row of (y, x + 1).  Of its 165 features only the B' samples of two pixels can
// come from wave t: this pixel (its new value, from LDS) and the upper neighbour (y - 1,
// x + 3) (its three new channels from six tagged 8-byte decision granules, dbox[8 (y - 1)
// ...]); the rest are loaded at the start.  Pixels take their index from a ticket counter, so a
// workgroup waits only for a lower ticket (dispatched earlier); extra workgroups (index >= M)
// build the first row of the rows that enter wave t + 1.  Query buffers alternate by wave parity.
struct Nx3 {
    Img3 Bsm, Blg, Bpsm, Bplg;
    int M, y_lo_n, M_n, H;
    const Col16Meta *meta;
    const float *rot;
    double *q3n, *qnn, *nskn;
    half8 *q16n;
    unsigned *tickets;            // [2]; tickets[t & 1] is this launch's
    unsigned *err;                // a decision wait timed out
    unsigned long long *dbox;     // 8 granules per row: channel c's bits at 2c (lo), 2c + 1 (hi)
};
constexpr unsigned long long C3_WAIT_TICKS = 1000000000ULL;   // 10 s of s_memrealtime
__device__ __forceinline__ unsigned long long c3_gran(unsigned tag, unsigned bits) {
    return ((unsigned long long)tag << 32) | bits;
}

//
// A batch of K identical-shape jobs (k_exact3b, grid (pixels, jobs)) runs the same body
// per job: the ticket counters, the error word and the decision granules live in each job's
// own workspace, so a workgroup of job k takes its pixel from job k's counter and waits only
// for job k's ticket m - 1, which a workgroup that is already resident took.  The single
// job's forward-progress argument therefore holds for any dispatch order of the (pixels x
// jobs) grid: in every job the resident workgroup with the lowest unfinished ticket waits for
// nothing that is not resident.  A wait that times out sets that job's error word
// (ia_synth3_status reads every job's).  The batch form also zeroes the padding columns
// [M_n, roundup32(M_n)) of the next wave's query tiles (the workgroup of its first row).
// The body is ia_color3_exact.inc, included by both kernels (C3X_M, C3X_YN, C3X_MN: the wave's
// M, y_lo_n, M_n: nx's own in the single job's kernel, launch arguments in the batch's, whose
// nx is read in place from the job table).
template <bool FUSE>
__global__ __launch_bounds__(256) void k_exact3(Fin3 f, Scr3 sc, Nx3 nx) {
#define C3X_BATCH 0
#define C3X_PUB 0
#define C3X_M nx.M
#define C3X_YN nx.y_lo_n
#define C3X_MN nx.M_n
#include "ia_color3_exact.inc"
#undef C3X_BATCH
#undef C3X_PUB
#undef C3X_M
#undef C3X_YN
#undef C3X_MN
}

// ---- a batch of K identical-shape jobs (ia_synth_levels3_batch) --------------------------
// One launch of k_query3rb / k_screen3rb / k_exact3b serves K jobs: the block's job is a grid
// dimension (query, exact: y; screen: z, y being its query group), and job k's pointers and
// scalars come from entry k of a device job table (one per level, in job 0's workspace).  The
// wave's scalars stay launch arguments.  Query sets alternate by wave parity on the fused
// path (set 0 otherwise).  Jobs may pass the same database (db, dbr, rot, src: a DB group, the
// multi_script batch's runs of one A / A' pair); no wave kernel writes into those buffers or
// their Col16Meta / Rot3Meta (the counters are g_c3_stats), and everything written stays per
// job.  When some do (G groups < K), the screen is k_screen3rs: one pass over a group's row
// tiles for its jobs' query tiles together; otherwise k_screen3rb.
constexpr int C3_CTL_ERR = 2;      // the error word's index in ctl
struct C3Job {
    Fin3 f;                        // t, y_lo: the launch's; q3: q3[parity]
    Scr3 sc;                       // qn, nsk: by parity
    Nx3 nx[2];                     // by parity (M, y_lo_n, M_n: the launch's); read in place
    const half8 *dbr;
    float *smin;
    double *q3[2], *qn[2], *nsk[2];
    half8 *q16[2];
    // the batch's DB groups (jobs passing one dbr, ia_batch3_groups), read by k_screen3rs; these
    // belong to the table's entry i, not to job i: the i-th job in group order, and group i's
    // first position in that order, job count and rotated DB
    int sjob, gfirst, gcount;
    const half8 *gdbr;
};
__global__ __launch_bounds__(256) void k_query3rb(const C3Job *__restrict__ jobs, int t, int y_lo, int M) {
    const C3Job &J = jobs[blockIdx.y];
    const Nx3 &nx = J.nx[0];
    query3r_body(nx.Bsm, nx.Blg, nx.Bpsm, nx.Bplg, t, y_lo, M, nx.meta, nx.rot, nullptr, J.q3[0], J.qn[0],
                 J.nsk[0], J.q16[0]);
}
__global__ __launch_bounds__(256, 2) void k_screen3rb(const C3Job *__restrict__ jobs, int ntiles, int M,
                                                      int tpw, int parity) {
    const C3Job &J = jobs[blockIdx.z];
    screen3r_body(J.dbr, ntiles, J.q16[parity], M, tpw, J.smin);
}
// The screen of a batch whose jobs share databases (G groups < K jobs): block (x, y, group z)
// stages up to S3R_QG consecutive entries of the group's list of n_g QT query tiles (entry e: tile
// e % QT of the group's job e / QT, each from its own job's q16) and walks the group's row
// tiles once for all of them, as screen3r_body does for one job's tiles: the same row-tile loop
// (screen3r_rows) after a staging of its own (per-entry sources, two barriers); every entry's
// minima go to its own job's smin.  It waits for nothing.
// entries per workgroup of a list of ne: its ceil(ne / S3R_QG) query groups, evenly filled
__host__ __device__ constexpr int s3rs_per(int ne) {
    return (ne + (ne + S3R_QG - 1) / S3R_QG - 1) / ((ne + S3R_QG - 1) / S3R_QG);
}
static_assert(s3rs_per(1) == 1 && s3rs_per(7) == 7 && s3rs_per(8) == 4 && s3rs_per(15) == 5 && s3rs_per(28) == 7,
              "k_screen3rs: query groups");
__global__ __launch_bounds__(256, 2) void k_screen3rs(const C3Job *__restrict__ jobs, int ntiles, int M,
                                                      int tpw, int parity) {
    __shared__ half8 qsh[S3R_QG * R3_TILE];
    __shared__ gptr<const half8> src_sh[S3R_QG];   // per staged entry: its query tile,
    __shared__ gptr<float> smin_sh[S3R_QG];        // its job's minima (gptr: global accesses)
    __shared__ int q0_sh[S3R_QG];             // and its first query
    const C3Job &G = jobs[blockIdx.z];
    const int QT = (M + 31) / 32;
    // the list's ceil(ne / S3R_QG) query groups in equal parts (8 entries: 4 + 4, not 7 + 1: the
    // launch is as long as its longest workgroup)
    const int ne = G.gcount * QT, per = s3rs_per(ne), e0 = blockIdx.y * per;
    if (e0 >= ne) return;   // (the whole workgroup, before any barrier: a smaller group's list ends here)
    const int nq = ne - e0 < per ? ne - e0 : per;
    if (threadIdx.x < nq) {
        const int e = e0 + threadIdx.x, jb = e / QT, qt = e - jb * QT;
        const C3Job &J = jobs[jobs[G.gfirst + jb].sjob];
        src_sh[threadIdx.x] = J.q16[parity] + (long)qt * R3_TILE;
        smin_sh[threadIdx.x] = J.smin;
        q0_sh[threadIdx.x] = qt * 32;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nq * R3_TILE; i += 256) {
        const int j = i / R3_TILE;
        qsh[i] = src_sh[j].p[i - j * R3_TILE];
    }
    __syncthreads();
    const gptr<const half8> db16g = G.gdbr;
    screen3r_rows(db16g.p, ntiles, M, tpw, qsh, nq, S3Tab{q0_sh, smin_sh});
}
template <bool FUSE>
__global__ __launch_bounds__(256) void k_exact3b(const C3Job *__restrict__ jobs, int t, int y_lo, int M,
                                                 int y_lo_n, int M_n) {
    const C3Job &J = jobs[blockIdx.y];
    const int b = FUSE ? t & 1 : 0;
    Fin3 f = J.f;
    f.t = t;
    f.y_lo = y_lo;
    f.q3 = J.q3[b];
    Scr3 sc = J.sc;
    sc.qn = J.qn[b];
    sc.nsk = J.nsk[b];
    const Nx3 &nx = J.nx[b];
#define C3X_BATCH 1
#define C3X_PUB 0
#define C3X_M M
#define C3X_YN y_lo_n
#define C3X_MN M_n
#include "ia_color3_exact.inc"
#undef C3X_BATCH
#undef C3X_PUB
#undef C3X_M
#undef C3X_YN
#undef C3X_MN
}

// ---- a level whose rows are sharded over ranks (IaSynthArgs.comm) -----------
// Each rank holds ia_db3_build(src, row0, nrows) of its contiguous row range (tiles, centre,
// bound and A_skip its own) and runs the wave in four launches: the query rows, the screen over
// its tiles, k_exact3p and k_peer_finish3.  k_exact3p is the exact stage above without the tail
// (ia_color3_exact.inc, C3X_PUB): it leaves this shard's (distance, global row = row0 + local
// row, weighted distance) in rec[m] and, on the device-side exchange (px.nranks > 0), publishes
// it to every rank's box.  It waits for nothing.
struct C3Pub {
    PeerView px;             // nranks 0: RCCL (the records are all-gathered from rec)
    ShardRec *rec;           // this rank's records of the wave (M)
    long row0;
};
template <bool FUSE>   // (false: the text's FUSE branches are discarded)
__global__ __launch_bounds__(256) void k_exact3p(Fin3 f, Scr3 sc, C3Pub pub) {
    static_assert(!FUSE, "a sharded level runs the four-launch form");
    const Nx3 nx{};
#define C3X_BATCH 0
#define C3X_PUB 1
#define C3X_M nx.M
#define C3X_YN nx.y_lo_n
#define C3X_MN nx.M_n
#include "ia_color3_exact.inc"
#undef C3X_BATCH
#undef C3X_PUB
#undef C3X_M
#undef C3X_YN
#undef C3X_MN
}

// ---- the LSH matcher for 165-dim rows (c.matcher = 'lsh' with convert=False) ---------------
// The definition of ia_lsh.hip with D = 165 over the materialised fp64 rows: tables from
// ia_lsh3_build (Lsh3View), centred value fl32(q_k - c_k), hash floorf(d / w) with d from
// p[165] through fmaf(p[e], q'[e], d), e = 0..164 in order, key = the masked sum of lsh_mix.
// One 256-thread workgroup per pixel of the wave (the shape of k_exact3<false>): the query row,
// weights and coherence window in one round trip; the L k hashes, one lane each (the 672-B
// projection rows as float4s, 16-B aligned); per table the bucket range (an empty bucket: the 4
// sorted entries around its position) and a prefix of the candidate counts (<= LSH_CAP per
// table); then the candidates in passes of 32 rows, 8 threads per row through acc8_row (plain
// and weighted sums from one read), the 15 coherence rows in the first pass, each pass's row
// numbers loaded during the pass before; the block's lexicographic (distance, row) minimum
// (no valid candidate: row 0, as k_lsh_query's row0), c3_decide and the 3-channel B' store.
// It waits for nothing and builds no query rows: a wave is k_query3, then this kernel.
// TAIL false: the stand-alone query (ia_lsh3_match_batch): query m from f.q3 + m qstride, the
// winner to idx / dist, no window, weights or tail.
template <bool TAIL>
__global__ __launch_bounds__(256) void k_lsh3_pixel(Fin3 f, Lsh3View lv, const double *__restrict__ center,
                                                    long nrows, int qstride, int64_t *__restrict__ idx,
                                                    double *__restrict__ dist) {
#include "ia_color3_lsh.inc"
}

// ---- a batch of K identical-shape LSH jobs (ia_synth_levels3_lsh_batch) --------------------
// One launch of k_query3b and one of k_lsh3_pixelb serve K jobs: the block's job is blockIdx.y,
// and everything of job k comes from entry k of a device job table (one per level, in job 0's
// workspace, where an exact batch keeps its C3Job table); the wave's scalars stay launch
// arguments.  Jobs of one DB group pass the same rows, tables, projections and centre; neither
// kernel writes into those, and everything written (q3, B', s, im, debug) stays per job.  Both
// kernels wait for nothing, so the job dimension needs no forward-progress argument.
struct L3Job {
    Fin3 f;                        // t, y_lo: the launch's; q3: the job's query rows, read
    double *q3;                    // the same rows, written by k_query3b
    Lsh3View lv;
    const double *center;
    long nrows;
    Img3 Bsm, Blg, Bpsm, Bplg;
};
__global__ __launch_bounds__(256) void k_query3b(const L3Job *__restrict__ jobs, int t, int y_lo) {
    const L3Job &J = jobs[blockIdx.y];
    const int m = blockIdx.x, k = threadIdx.x;
    const int y = y_lo + m, x = t - 3 * y;
    if (k >= D3P) return;
    double v = 0.0;
    if (k < D3_FULL) v = feat3(J.Bsm, J.Blg, y, x, k);
    else if (k < D3) v = feat3(J.Bpsm, J.Bplg, y, x, k - D3_FULL);
    J.q3[(long)m * D3P + k] = v;
}
__global__ __launch_bounds__(256) void k_lsh3_pixelb(const L3Job *__restrict__ jobs, int t, int y_lo) {
    constexpr bool TAIL = true;
    const L3Job &J = jobs[blockIdx.y];
    Fin3 f = J.f;
    f.t = t;
    f.y_lo = y_lo;
    const Lsh3View lv = J.lv;
    const double *__restrict__ center = J.center;
    const long nrows = J.nrows;
    constexpr int qstride = D3P;
    int64_t *const idx = nullptr;
    double *const dist = nullptr;
#include "ia_color3_lsh.inc"
}

// the replicated fp64 pyramids of a level's A side (feat3's inputs, as k_db3_build's)
struct Src3 {
    Img3 Asm, Alg;
    const double *Ap_sm, *Ap_lg;
    int pairs;         // training pairs: A image i goes with A' image i (0: one A for every A' image)
};
// acc8_row for a row that is not materialised here: features k = j + 8 i of DB pixel (r, c)
// of A' image img gathered from the pyramids, exactly the values k_db3_build writes, and the
// same sums in the same order (an accumulator that starts at +0 and adds its first term, a
// square, holds that term's bits).  Five gathers in flight at a time, not acc8_row's 21: the
// waiting kernel's VGPRs stay small.
__device__ __forceinline__ Acc8 acc8_feat(const Src3 &s, int img, int r, int c, int j, const double *qs,
                                          const double *ws) {
    // (the A half of the row: image img of training pairs, stacked as the A' images are)
    const long osm = (long)s.Asm.h * s.Asm.w * 3, olg = (long)s.Alg.h * s.Alg.w * 3;
    const int aimg = s.pairs ? img : 0;
    const double *psm = s.Ap_sm + img * osm, *plg = s.Ap_lg + img * olg;
    const long asm_ = aimg * osm, alg_ = aimg * olg;   // (offsets: a select of four per-lane pointers
                                                       // compiled to a table in scratch memory)
    // feat3's sample of the pair (A | A' of image img; one shape) with every choice a select of
    // scalars (feat3's own branches over two Img3 temporaries put them in scratch here)
    auto ld = [&](int k) __attribute__((always_inline)) {
        const bool ap = k >= D3_FULL;
        const int kk = ap ? k - D3_FULL : k;
        const bool co = kk < 27;                     // the coarse 3x3x3 window, else the fine 5x5x3
        const int e = co ? kk : kk - 27;
        const int t = e / 3, ch = e - 3 * t;
        const int dr = co ? t / 3 - 1 : t / 5 - 2, dc = co ? t % 3 - 1 : t % 5 - 2;
        const int h = co ? s.Asm.h : s.Alg.h, w = co ? s.Asm.w : s.Alg.w;
        const double *p = co ? (ap ? psm : s.Asm.p) : (ap ? plg : s.Alg.p);
        return p[(ap ? 0 : (co ? asm_ : alg_)) + ((long)symi2((co ? r >> 1 : r) + dr, h) * w + symi2((co ? c >> 1 : c) + dc, w)) * 3 + ch];
    };
    constexpr int G = 5;   // gathers in flight
    double hp[2], hw[2];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        double p = 0.0, w = 0.0;
#pragma unroll 1
        for (int g = 0; g < 10; g += G) {
            const int k0 = j + 8 * (10 * half + g);
            const double x0 = ld(k0), x1 = ld(k0 + 8), x2 = ld(k0 + 16), x3 = ld(k0 + 24), x4 = ld(k0 + 32);
            auto add = [&](double xv, int k) __attribute__((always_inline)) {
                const double d = xv - qs[k];
                const double dw = d * ws[k];
                p += d * d;
                w += dw * dw;
            };
            add(x0, k0); add(x1, k0 + 8); add(x2, k0 + 16); add(x3, k0 + 24); add(x4, k0 + 32);
        }
        hp[half] = p;
        hw[half] = w;
    }
    Acc8 a{hp[0], hp[1], 0.0, hw[0], hw[1], 0.0};
    if (j < D3 - 160) {
        const double d = ld(160 + j) - qs[160 + j];
        const double dw = d * ws[160 + j];
        a.pt = d * d;
        a.wt = dw * dw;
    }
    return a;
}

// The tail of a sharded level, one 128-thread workgroup per pixel (modelled on k_peer_finish,
// ia_synth.hip).  Wave 0 takes the lexicographic (distance, row) minimum of every rank's record
// of query m: from this rank's receive box (peer_collect_rec: the ONLY inter-rank wait of the
// colour path, with its timeout and error word; on timeout this shard's own record stands) or,
// over RCCL (px.nranks == 0), from the gathered records rec[g * M + m].  Wave 1 meanwhile
// computes the plain and weighted distances of the <= 15 coherence window rows, which may lie
// in any rank's shard, from the replicated pyramids (acc8_feat: the materialised rows' bits).
// Then c3_decide and the three-channel B' store, on replicated state: every rank ends with the
// same B', s and im.  The wait sits here, in a small workgroup (~9 KB of LDS), never in the
// exact stage's 256-thread, 21-23 KB ones: the screens and exact stages the awaited records
// depend on keep room to run beside any number of these.
__global__ __launch_bounds__(128) void k_peer_finish3(Fin3 f, Src3 src, PeerView px,
                                                      const ShardRec *__restrict__ rec, int nranks, int M) {
    __shared__ double qs[D3P], wsh[D3P];
    __shared__ Acc8 cacc[15 * 8];
    __shared__ double sump[15], sumw[15];
    __shared__ long long rix[15];
    __shared__ int rpos[15][3];
    const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int y = f.y_lo + m, x = f.t - 3 * y;
    for (int k = tid; k < D3P; k += 128) {
        qs[k] = f.q3[(long)m * D3P + k];
        wsh[k] = k < D3 ? f.weights[k] : 0.0;
    }
    if (tid < 15) c3_window(tid, y, x, f, rix, rpos);
    XRec win{INFINITY, 0x7fffffffffffffffLL, 0.0, 0.0};
    if (wv == 0 && px.nranks > 0) {
        const ShardRec own = rec[m];
        win = XRec{own.d, own.idx, own.wd, 0.0};
    }
    __syncthreads();
    if (wv == 0) {
        if (px.nranks > 0) {
            peer_collect_rec(px, m, lane, win);
        } else {
            if (lane < nranks) {
                const ShardRec r = rec[(long)lane * M + m];
                win = XRec{r.d, r.idx, r.wd, 0.0};
            }
            win = xrec_wave_min(win);
        }
    } else {
#pragma unroll 1
        for (int e = lane; e < 15 * 8; e += 64) {
            const int ro = e >> 3;
            if (rix[ro] >= 0) cacc[e] = acc8_feat(src, rpos[ro][2], rpos[ro][0], rpos[ro][1], e & 7, qs, wsh);
        }
    }
    __syncthreads();
    if (tid < 15) {
        if (rix[tid] >= 0) {
            sump[tid] = sqrt(acc8_sum(cacc + 8 * tid, false));
            const double sq = sqrt(acc8_sum(cacc + 8 * tid, true));
            sumw[tid] = sq * sq;
        } else {
            sump[tid] = INFINITY;
            sumw[tid] = 0.0;
        }
    }
    __syncthreads();
    if (wv != 0) return;
    const long from = c3_decide(f, y, x, lane, win.i, win.wd, sump, sumw, rix, rpos);
    if (lane < 3) f.Bp_lg[((long)y * f.W + x) * 3 + lane] = f.Ap_lg[from + lane];
}

// The per-pixel tail of the exhaustive fp64 search (IA_COLOR16=0), one 256-thread workgroup
// per pixel: the winner is the lexicographic minimum of k_match3's partials (order free); the
// 15 coherence candidates' and the winner's rows are read once, lane-parallel over (row,
// feature); their plain and weighted squared terms go to LDS, and 31 threads sum one row each
// (Pw165); then c3_decide and the B' store as k_exact3.
__global__ __launch_bounds__(256) void k_finish3w(Fin3 f, const Best *__restrict__ part, int nb) {
    __shared__ double qs[D3P], wsh[D3P];
    __shared__ double tp[15][D3], tw[16][D3];   // coherence rows: plain, weighted (+ winner)
    __shared__ double sump[15], sumw[16];
    __shared__ long long rix[16];               // rows: candidates 0..14, winner 15 (-1: none)
    __shared__ int rpos[15][3];
    __shared__ double rd[4];
    __shared__ long long ri[4];
    const int m = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int y = f.y_lo + m, x = f.t - 3 * y;
    // the query, the weights, the coherence candidates' rows (from s / im) and the partials'
    // minimum: one round trip
    if (tid < D3P) {
        qs[tid] = f.q3[(long)m * D3P + tid];
        wsh[tid] = tid < D3 ? f.weights[tid] : 0.0;
    }
    if (tid < 15) c3_window(tid, y, x, f, rix, rpos);
    const long long app = block_best(part + (long)m * nb, nb, rd, ri).idx;
    if (tid == 0) rix[15] = app;
    __syncthreads();
    // the terms: (row j, feature k) pairs spread over the block, each row read once
    for (int e = tid; e < 16 * D3; e += 256) {
        const int j = e / D3, k = e - j * D3;
        const long long ix = rix[j];
        if (ix < 0) continue;
        const double d = f.db3[ix * D3P + k] - qs[k];
        const double dw = d * wsh[k];
        if (j < 15) tp[j][k] = d * d;
        tw[j][k] = dw * dw;
    }
    __syncthreads();
    if (tid < 31) {   // one row per thread, numpy's pairwise order
        const bool pl = tid < 15;
        const int j = pl ? tid : tid - 15;
        const double *t = pl ? tp[j] : tw[j];
        if (rix[j] >= 0) {
            const double sq = sqrt(pw165_sum(t));
            if (pl) sump[j] = sq; else sumw[j] = sq * sq;
        } else {
            if (pl) sump[j] = INFINITY; else sumw[j] = 0.0;
        }
    }
    __syncthreads();
    if (wv != 0) return;
    const long src = c3_decide(f, y, x, lane, app, sumw[15], sump, sumw, rix, rpos);
    if (lane < 3) f.Bp_lg[((long)y * f.W + x) * 3 + lane] = f.Ap_lg[src + lane];
}

// per-pixel API helpers (algorithms.py:92-135) for 165-dim rows: the coherence argmin over n
// candidate rows (first minimum of sqrt(pairwise((a - q)^2))) and weighted distances
__global__ void k_coherence_pick3(const double *__restrict__ rows, int n, const double *__restrict__ q,
                                  int32_t *out) {
    __shared__ double sd[64];
    const int i = threadIdx.x;
    double d = INFINITY;
    if (i < n) {
        Pw165 pw;
        for (int k = 0; k < D3; ++k) {
            const double x = rows[(long)i * D3 + k] - q[k];
            pw.feed(k, x * x);
        }
        d = sqrt(pw.result());
    }
    sd[i] = d;
    __syncthreads();
    if (i == 0) {
        int b = 0;
        for (int j = 1; j < n; ++j)
            if (sd[j] < sd[b]) b = j;
        out[0] = b;
    }
}

__global__ void k_wdist3(const double *__restrict__ a, const double *__restrict__ q,
                         const double *__restrict__ w, int n, double *__restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Pw165 pw;
    for (int k = 0; k < D3; ++k) {
        const double x = (a[(long)i * D3 + k] - q[(long)i * D3 + k]) * w[k];
        pw.feed(k, x * x);
    }
    const double s = sqrt(pw.result());
    out[i] = s * s;
}

__global__ void k_split_best3(const Best *__restrict__ b, int M, int64_t *idx, double *dist) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M) return;
    if (idx) idx[i] = b[i].idx;
    if (dist) dist[i] = b[i].d;
}

static inline int match3_blocks(long nrows) { return (int)((nrows + M3_ROWS - 1) / M3_ROWS); }

// IA_COLOR16 (ia_diag_set_color16): 1 the split-f16 screen + exact stage, 0 the exhaustive
// fp64 search (k_match3)
static std::atomic<int> g_color16{env_int("IA_COLOR16", 1)};
static unsigned long long *g_c3_stats = nullptr;   // diagnostic counters (ia_diag_color16_stats)
// IA_C3_SHARED_SCREEN (ia_diag_set_c3_shared_screen): 1 a batch whose jobs share databases
// screens each DB group in one k_screen3rs pass, 0 every job through k_screen3rb (same minima)
static std::atomic<int> g_c3_shared_screen{env_int("IA_C3_SHARED_SCREEN", 1)};

// the DB groups of one level's K jobs (ia_batch3_groups): jobs passing the same non-null dbr
// form a group, numbered in order of first appearance; returns their number
static int batch3_groups(const IaSynthArgs *jobs, int K, int *group_of_job) {
    int G = 0, first[IA_BATCH_MAX];
    for (int k = 0; k < K; ++k) {
        int g = 0;
        while (g < G && !(jobs[k].dbr && jobs[first[g]].dbr == jobs[k].dbr)) ++g;
        if (g == G) first[G++] = k;
        group_of_job[k] = g;
    }
    return G;
}

// the synthesis workspace: q3 | partials (fp64 search) | q16 | qn | tile minima, and for
// the fused R16c tail (k_exact3<true>) the odd waves' query set, the control words and the
// decision granules
struct Ws3 {
    double *q3;
    Best *part;
    half8 *q16;              // the query tiles of either screen (C16_TILE >= R3_TILE)
    double *qn, *nsk;
    float *smin;
    double *q3b, *qnb, *nskb;
    half8 *q16b;
    unsigned *ctl;           // tickets[2], error word
    unsigned long long *dbox;
    C3Job *jtab;             // a batch's job table (ia_synth_levels3_batch, job 0's workspace)
    ShardRec *rec, *rec_all; // a sharded level: this rank's records, all ranks' (RCCL gather)
};
// the fused colour tail (k_exact3<true>: the next wave's query rows from the exact stage's
// launch; IA_C3_FUSE, default 1) on R16c levels; read per level (Level3::init)
static inline bool c3_fuse() { return env_int("IA_C3_FUSE", 1) != 0; }
static_assert(C16_TILE >= R3_TILE, "query tiles");
// (nranks > 0: a sharded level's workspace, the records after everything else, so the
// unsharded layout and ia_synth3_workspace_bytes keep their values)
static inline size_t ws3_layout(int H, int W, long nrows, char *base, Ws3 *w, int nranks = 0) {
    const size_t M = (size_t)wave_max_queries(H, W), Mp = (M + 31) / 32 * 32;
    size_t o = 0;
    auto take = [&](size_t bytes) { char *p = base ? base + o : nullptr; o += align_up(bytes, 256); return p; };
    char *q3 = take(Mp * D3P * sizeof(double));
    char *part = take(M * (size_t)match3_blocks(nrows) * sizeof(Best));
    char *q16 = take(Mp / 32 * C16_TILE * sizeof(half8));
    char *qn = take(Mp * sizeof(double));
    char *nsk = take(Mp * sizeof(double));
    char *smin = take(M * (size_t)c3_stride((int)db3_tiles(nrows)) * sizeof(float));
    char *q3b = take(Mp * D3P * sizeof(double));
    char *q16b = take(Mp / 32 * C16_TILE * sizeof(half8));
    char *qnb = take(Mp * sizeof(double));
    char *nskb = take(Mp * sizeof(double));
    char *ctl = take(256);
    char *dbox = take((size_t)H * 8 * sizeof(unsigned long long));
    char *jtab = take((size_t)IA_BATCH_MAX * sizeof(C3Job));
    char *rec = nranks > 0 ? take(Mp * sizeof(ShardRec)) : nullptr;
    char *rec_all = nranks > 0 ? take(Mp * (size_t)nranks * sizeof(ShardRec)) : nullptr;
    if (w) {
        w->rec = reinterpret_cast<ShardRec *>(rec);
        w->rec_all = reinterpret_cast<ShardRec *>(rec_all);
        w->jtab = reinterpret_cast<C3Job *>(jtab);
        w->q3b = reinterpret_cast<double *>(q3b);
        w->q16b = reinterpret_cast<half8 *>(q16b);
        w->qnb = reinterpret_cast<double *>(qnb);
        w->nskb = reinterpret_cast<double *>(nskb);
        w->ctl = reinterpret_cast<unsigned *>(ctl);
        w->dbox = reinterpret_cast<unsigned long long *>(dbox);
        w->q3 = reinterpret_cast<double *>(q3);
        w->part = reinterpret_cast<Best *>(part);
        w->q16 = reinterpret_cast<half8 *>(q16);
        w->qn = reinterpret_cast<double *>(qn);
        w->nsk = reinterpret_cast<double *>(nsk);
        w->smin = reinterpret_cast<float *>(smin);
    }
    return o;
}

// a level's lsh (NULL: fine): only on an unsharded level, with its centre and usable tables
static int lsh3_level_check(const IaSynthArgs &a, const char *who) {
    if (!a.lsh) return IA_OK;
    IA_ARG(!a.comm, std::string(who) + ": a sharded level runs the exact matcher (comm with lsh)");
    IA_ARG(a.center, std::string(who) + ": lsh needs center (165 doubles)");
    return lsh3_check(a.lsh, who);
}

// one 3-channel level (all its rows, or this rank's shard): the wave loop of ia_synth_level3
// (per wave: the query rows and split operand, the screen, the exact stage + tail; or the
// exhaustive fp64 search; an LSH level: the query rows, k_lsh3_pixel; a sharded level:
// wave_sharded)
struct Level3 {
    const IaSynthArgs *a = nullptr;
    Ws3 w{};
    Db3View v{};
    Fin3 f{};
    Scr3 sc{};
    Img3 Bsm{}, Blg{}, Bpsm{}, Bplg{};
    int H = 0, W = 0, nw = 0, nb = 0, ntiles = 0;
    bool split = true, rot = false;   // rot: the R16c screen (a->dbr, a->rot: ia_db3_build_rot)
    bool fuse = false;                // rot with the fused tail (k_exact3<true>)
    bool lsh = false;                 // the LSH matcher (a->lsh, a->center): k_lsh3_pixel
    Lsh3View lv{};
    const half8 *dbr = nullptr;
    // a sharded level (a->comm): rows [row0, row0 + nrows) of N_total, one exchange per wave
    bool sharded = false, peer = false;
    int nranks = 1;
    Src3 src3{};
    int init(const IaSynthArgs *a_, hipStream_t st) {
        a = a_;
        IA_ARG(a && a->db && a->B_sm && a->B_lg && a->Bp_sm && a->Bp_lg && a->weights && a->s && a->im &&
                   a->workspace && a->H > 0 && a->W > 0,
               "ia_synth_level3: bad args");
        IA_SRC_NA(a->src, "ia_synth_level3");
        {
            const int rc = lsh3_level_check(*a, "ia_synth_level3");
            if (rc) return rc;
        }
        lsh = a->lsh != nullptr;
        const long N = (long)a->src.nAp * a->src.Ah * a->src.Aw;
        sharded = a->comm != nullptr;
        if (!sharded) {
            IA_ARG(a->row0 == 0 && a->nrows == N,
                   "ia_synth_level3: a partial row range (row0, nrows) needs a comm");
        } else {
            nranks = comm_nranks(a->comm);
            peer = comm_peer_mcap(a->comm) > 0;
            IA_ARG(nranks >= 1 && nranks <= 64, "ia_synth_level3: bad communicator");
            IA_ARG(a->nrows > 0 && a->row0 >= 0 && a->row0 + a->nrows <= N && a->N_total == N,
                   "ia_synth_level3: bad shard (row0, nrows, N_total)");
            IA_ARG(N < (1L << 32), "ia_synth_level3: the exchange carries 32-bit rows (N_total >= 2^32)");
            IA_ARG(g_color16.load(std::memory_order_relaxed) != 0,
                   "ia_synth_level3: a sharded level runs the screened matcher (IA_COLOR16=0 is unsharded only)");
            IA_ARG(!peer || comm_peer_mcap(a->comm) >= wave_max_queries(a->H, a->W),
                   "ia_synth_level3: the peer exchange's box holds fewer queries than a wave");
        }
        IA_ARG(!a->dbg_px == !a->dbg_dist, "ia_synth_level3: debug outputs come in pairs");
        H = a->H;
        W = a->W;
        ws3_layout(H, W, a->nrows, reinterpret_cast<char *>(a->workspace), &w, sharded ? nranks : 0);
        src3 = Src3{Img3{a->src.A_sm, a->src.A_hs, a->src.A_ws}, Img3{a->src.A_lg, a->src.Ah, a->src.Aw},
                    a->src.Ap_sm, a->src.Ap_lg, src_pairs(a->src) ? 1 : 0};
        nb = match3_blocks(a->nrows);
        Bsm = Img3{a->B_sm, a->B_hs, a->B_ws};
        Blg = Img3{a->B_lg, H, W};
        Bpsm = Img3{a->Bp_sm, a->B_hs, a->B_ws};
        Bplg = Img3{a->Bp_lg, H, W};
        v = db3_view(const_cast<void *>(a->db), a->nrows);
        f = Fin3{v.rows, w.q3, a->src.Ap_lg, a->src.Ah, a->src.Aw,
                 0, 0, W, a->weights, a->kappa_factor, a->Bp_lg, a->s, a->im, a->dbg_px, a->dbg_dist};
        split = g_color16.load(std::memory_order_relaxed) != 0;
        ntiles = (int)v.ntiles;
        if (lsh) lv = lsh3_view(a->lsh, a->nrows);
        rot = split && a->dbr && a->rot && !lsh;   // (an LSH level reads no screen operand)
        dbr = reinterpret_cast<const half8 *>(a->dbr);
        sc = Scr3{w.smin, ntiles, a->nrows, w.qn, v.meta, g_c3_stats, rot ? w.nsk : nullptr,
                  rot ? db3r_meta(const_cast<void *>(a->dbr), a->nrows) : nullptr};
        nw = wave_count(H, W);
        fuse = rot && c3_fuse() && !sharded;   // (a sharded level: the four-launch form)
        IA_HIP(hipMemsetAsync(w.ctl, 0, 256, st));
        if (fuse) IA_HIP(hipMemsetAsync(w.dbox, 0, (size_t)H * 8 * sizeof(unsigned long long), st));
        return IA_OK;
    }

    // a batch of K identical-shape jobs (ia_synth_levels3_batch): this run is job 0 and owns
    // the job table; part holds jobs 1 .. K-1 (their own control words and granules, set up by
    // their own init)
    int K = 1;
    std::vector<Level3> part;
    C3Job job_entry() const {
        C3Job J{};
        J.f = f;
        J.sc = sc;
        J.dbr = dbr;
        J.smin = w.smin;
        J.q3[0] = w.q3; J.q3[1] = w.q3b;
        J.qn[0] = w.qn; J.qn[1] = w.qnb;
        J.nsk[0] = w.nsk; J.nsk[1] = w.nskb;
        J.q16[0] = w.q16; J.q16[1] = w.q16b;
        for (int b = 0; b < 2; ++b)   // wave parity b writes the next wave's set b ^ 1
            J.nx[b] = Nx3{Bsm, Blg, Bpsm, Bplg, 0, 0, 0, H, v.meta, a->rot, J.q3[b ^ 1], J.qn[b ^ 1],
                          J.nsk[b ^ 1], J.q16[b ^ 1], w.ctl, w.ctl + C3_CTL_ERR, w.dbox};
        return J;
    }
    // a batch of K > 1 LSH jobs (ia_synth_levels3_lsh_batch, which has validated args[0..nj)):
    // as init_batch, with the L3Job table in the place of the C3Job one (w.jtab's area)
    bool lshb = false;
    L3Job lsh_entry() const { return L3Job{f, w.q3, lv, a->center, a->nrows, Bsm, Blg, Bpsm, Bplg}; }
    int init_lsh_batch(const IaSynthArgs *args, int nj, hipStream_t st, L3Job *pinned) {
        static_assert(sizeof(L3Job) <= sizeof(C3Job), "the LSH job table lives in the jtab area");
        int rc = init(&args[0], st);
        if (rc) return rc;
        IA_ARG(lsh && nj > 1 && nj <= IA_BATCH_MAX, "ia_synth_levels3_lsh_batch: bad batch");
        K = nj;
        lshb = true;
        part.resize(K - 1);
        pinned[0] = lsh_entry();
        for (int k = 1; k < K; ++k) {
            if ((rc = part[k - 1].init(&args[k], st))) return rc;
            IA_ARG(part[k - 1].lsh, "ia_synth_levels3_lsh_batch: a job without lsh");
            pinned[k] = part[k - 1].lsh_entry();
        }
        IA_HIP(hipMemcpyAsync(w.jtab, pinned, (size_t)K * sizeof(L3Job), hipMemcpyHostToDevice, st));
        return IA_OK;
    }
    // args[0..nj): the jobs' levels (validated by ia_synth_levels3_batch); the job table is
    // staged through `pinned` (kept alive by the caller until the copy has run)
    int init_batch(const IaSynthArgs *args, int nj, hipStream_t st, C3Job *pinned) {
        int rc = init(&args[0], st);
        if (rc || nj == 1) return rc;
        IA_ARG(rot, "ia_synth_levels3_batch: a batch of K > 1 jobs runs the rotated screen (dbr, rot; IA_COLOR16=1)");
        K = nj;
        part.resize(K - 1);
        for (int k = 1; k < K; ++k) {
            if ((rc = part[k - 1].init(&args[k], st))) return rc;
            IA_ARG(part[k - 1].rot && part[k - 1].ntiles == ntiles, "ia_synth_levels3_batch: jobs of different forms");
        }
        pinned[0] = job_entry();
        for (int k = 1; k < K; ++k) pinned[k] = part[k - 1].job_entry();
        // the DB groups (the caller has checked that jobs of one dbr agree in db, rot, nrows and
        // src): the jobs in group order and each group's range of that order, in the table too
        int grp[IA_BATCH_MAX];
        const int G = batch3_groups(args, K, grp);
        gcount.assign(G, 0);
        for (int k = 0; k < K; ++k) ++gcount[grp[k]];
        for (int g = 0, pos = 0; g < G; pos += gcount[g++]) {
            pinned[g].gfirst = pos;
            pinned[g].gcount = gcount[g];
            int i = pos;
            for (int k = 0; k < K; ++k)
                if (grp[k] == g) {
                    if (i == pos) pinned[g].gdbr = pinned[k].dbr;
                    pinned[i++].sjob = k;
                }
        }
        shared_screen = G < K && g_c3_shared_screen.load(std::memory_order_relaxed) != 0;
        IA_HIP(hipMemcpyAsync(w.jtab, pinned, (size_t)K * sizeof(C3Job), hipMemcpyHostToDevice, st));
        return IA_OK;
    }
    // a batch's DB groups: jobs per group (G = gcount.size()); shared_screen: some jobs share a
    // database and the wave's screen is k_screen3rs (else k_screen3rb, every job for itself)
    std::vector<int> gcount;
    bool shared_screen = false;
    void screen_batch(int M, int parity, hipStream_t st) {
        int tpw;
        if (!shared_screen) {
            const dim3 grid = screen3r_grid(ntiles, M, tpw, K);
            k_screen3rb<<<grid, 256, 0, st>>>(w.jtab, ntiles, M, tpw, parity);
            return;
        }
        const int QT = (M + 31) / 32;
        int total = 0, most = 0;
        for (int n : gcount) {
            const int qg = (n * QT + S3R_QG - 1) / S3R_QG;
            total += qg;
            most = std::max(most, qg);
        }
        const dim3 grid = screen3rs_grid(ntiles, total, most, (int)gcount.size(), tpw);
        k_screen3rs<<<grid, 256, 0, st>>>(w.jtab, ntiles, M, tpw, parity);
    }
    // wave t of a batch: the single job's launches with the job as a grid dimension
    int wave_batch(int t, int y_lo, int M, hipStream_t st) {
        const int QT = (M + 31) / 32;
        if (fuse) {
            if (t == 0) k_query3rb<<<dim3(QT * 32, K), 256, 0, st>>>(w.jtab, t, y_lo, M);
            screen_batch(M, t & 1, st);
            int y_lo_n = 0, M_n = 0;
            if (t + 1 < nw) wave_rows(H, W, t + 1, y_lo_n, M_n);
            const int R = std::max(M, M_n > 0 ? y_lo_n + M_n - y_lo : 0);
            k_exact3b<true><<<dim3(R, K), 256, 0, st>>>(w.jtab, t, y_lo, M, y_lo_n, M_n);
        } else {
            k_query3rb<<<dim3(QT * 32, K), 256, 0, st>>>(w.jtab, t, y_lo, M);
            screen_batch(M, 0, st);
            k_exact3b<false><<<dim3(M, K), 256, 0, st>>>(w.jtab, t, y_lo, M, 0, 0);
        }
        IA_LAUNCH_CHECK("ia_synth_levels3_batch wave");
        return IA_OK;
    }

    int wave(int t, hipStream_t st) {
        int y_lo, M;
        wave_rows(H, W, t, y_lo, M);
        if (M <= 0) return IA_OK;
        if (lshb) {   // the single LSH job's two launches with the job as a grid dimension
            const L3Job *jt = reinterpret_cast<const L3Job *>(w.jtab);
            k_query3b<<<dim3(M, K), 256, 0, st>>>(jt, t, y_lo);
            k_lsh3_pixelb<<<dim3(M, K), 256, 0, st>>>(jt, t, y_lo);
            IA_LAUNCH_CHECK("ia_synth_levels3_lsh_batch wave");
            return IA_OK;
        }
        if (K > 1) return wave_batch(t, y_lo, M, st);
        f.t = t;
        f.y_lo = y_lo;
        if (sharded) return wave_sharded(M, st);
        if (lsh) {
            k_query3<<<M, 256, 0, st>>>(Bsm, Blg, Bpsm, Bplg, t, y_lo, w.q3);
            k_lsh3_pixel<true><<<M, 256, 0, st>>>(f, lv, a->center, a->nrows, D3P, nullptr, nullptr);
        } else if (fuse) {
            // wave t's query set b (wave 0's built here, the later ones by the previous wave's
            // k_exact3<true>), wave t + 1's into set b ^ 1
            const int b = t & 1;
            double *q3s[2] = {w.q3, w.q3b}, *qns[2] = {w.qn, w.qnb}, *nsks[2] = {w.nsk, w.nskb};
            half8 *q16s[2] = {w.q16, w.q16b};
            int tpw;
            const dim3 grid = screen3r_grid(ntiles, M, tpw);
            if (t == 0)
                k_query3r<<<(M + 31) / 32 * 32, 256, 0, st>>>(Bsm, Blg, Bpsm, Bplg, t, y_lo, M, v.meta, a->rot, nullptr,
                                                              q3s[0], qns[0], nsks[0], q16s[0]);
            k_screen3r<<<grid, 256, 0, st>>>(dbr, ntiles, q16s[b], M, tpw, w.smin);
            int y_lo_n = 0, M_n = 0;
            if (t + 1 < nw) wave_rows(H, W, t + 1, y_lo_n, M_n);
            const Nx3 nx{Bsm, Blg, Bpsm, Bplg, M, y_lo_n, M_n, H, v.meta, a->rot, q3s[b ^ 1], qns[b ^ 1],
                         nsks[b ^ 1], q16s[b ^ 1], w.ctl, w.ctl + C3_CTL_ERR, w.dbox};
            Fin3 fb = f;
            fb.q3 = q3s[b];
            Scr3 sb = sc;
            sb.qn = qns[b];
            sb.nsk = nsks[b];
            const int R = std::max(M, M_n > 0 ? y_lo_n + M_n - y_lo : 0);
            k_exact3<true><<<R, 256, 0, st>>>(fb, sb, nx);
        } else if (rot) {
            const int QT = (M + 31) / 32;
            int tpw;
            const dim3 grid = screen3r_grid(ntiles, M, tpw);
            k_query3r<<<QT * 32, 256, 0, st>>>(Bsm, Blg, Bpsm, Bplg, t, y_lo, M, v.meta, a->rot, nullptr, w.q3,
                                               w.qn, w.nsk, w.q16);
            k_screen3r<<<grid, 256, 0, st>>>(dbr, ntiles, w.q16, M, tpw, w.smin);
            k_exact3<false><<<M, 256, 0, st>>>(f, sc, Nx3{});
        } else if (split) {
            const int QT = (M + 31) / 32;
            int tpw;
            const dim3 grid = screen3_grid(ntiles, M, tpw);
            k_query3s<<<QT * 32, 256, 0, st>>>(Bsm, Blg, Bpsm, Bplg, t, y_lo, M, v.meta, w.q3, w.qn,
                                               reinterpret_cast<_Float16 *>(w.q16));
            k_screen3<<<grid, 256, 0, st>>>(v.db16, ntiles, w.q16, M, tpw, w.smin);
            k_exact3<false><<<M, 256, 0, st>>>(f, sc, Nx3{});
        } else {
            k_query3<<<M, 256, 0, st>>>(Bsm, Blg, Bpsm, Bplg, t, y_lo, w.q3);
            k_match3<<<nb, 256, 0, st>>>(f.db3, a->nrows, 0, w.q3, M, w.part);
            k_finish3w<<<M, 256, 0, st>>>(f, w.part, nb);
        }
        IA_LAUNCH_CHECK("ia_synth_level3 wave");
        return IA_OK;
    }
    // wave t of a sharded level: the query rows and the screen of this shard's tiles as on one
    // GPU, the publishing exact stage, [RCCL: one all-gather of the M records,] the finish
    int wave_sharded(int M, hipStream_t st) {
        const int QT = (M + 31) / 32;
        int tpw;
        if (rot) {
            const dim3 grid = screen3r_grid(ntiles, M, tpw);
            k_query3r<<<QT * 32, 256, 0, st>>>(Bsm, Blg, Bpsm, Bplg, f.t, f.y_lo, M, v.meta, a->rot, nullptr, w.q3,
                                               w.qn, w.nsk, w.q16);
            k_screen3r<<<grid, 256, 0, st>>>(dbr, ntiles, w.q16, M, tpw, w.smin);
        } else {
            const dim3 grid = screen3_grid(ntiles, M, tpw);
            k_query3s<<<QT * 32, 256, 0, st>>>(Bsm, Blg, Bpsm, Bplg, f.t, f.y_lo, M, v.meta, w.q3, w.qn,
                                               reinterpret_cast<_Float16 *>(w.q16));
            k_screen3<<<grid, 256, 0, st>>>(v.db16, ntiles, w.q16, M, tpw, w.smin);
        }
        const PeerView px = peer ? comm_peer_wave(a->comm) : PeerView{};
        k_exact3p<false><<<M, 256, 0, st>>>(f, sc, C3Pub{px, w.rec, a->row0});
        IA_LAUNCH_CHECK("ia_synth_level3 sharded wave");
        if (!peer) {
            const int rc = comm_allgather(a->comm, w.rec, w.rec_all, (size_t)M * sizeof(ShardRec), st);
            if (rc) return rc;
        }
        k_peer_finish3<<<M, 128, 0, st>>>(f, src3, px, peer ? w.rec : w.rec_all, nranks, M);
        IA_LAUNCH_CHECK("k_peer_finish3");
        return IA_OK;
    }
    int done(hipStream_t) { return IA_OK; }
};

}  // namespace ia

using namespace ia;

extern "C" {

size_t ia_db3_bytes(long nrows) {
    return nrows > 0 ? db3_rows_bytes(nrows) + db3_split_bytes(nrows) + sizeof(Col16Meta) : 0;
}

int ia_db3_build(const IaSrcLevel *src, long row0, long nrows, double *db3, void *stream) {
    IA_ARG(src && db3 && nrows > 0 && row0 >= 0, "ia_db3_build: bad args");
    IA_SRC_NA(*src, "ia_db3_build");
    IA_ARG(row0 + nrows <= (long)src->nAp * src->Ah * src->Aw, "ia_db3_build: rows out of range");
    const Img3 Asm{src->A_sm, src->A_hs, src->A_ws}, Alg{src->A_lg, src->Ah, src->Aw};
    const long n = nrows * D3P;
    hipStream_t st = S(stream);
    const bool pairs = src_pairs(*src);
    k_db3_build<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(
        Asm, Alg, pairs ? (long)src->A_hs * src->A_ws * 3 : 0, pairs ? (long)src->Ah * src->Aw * 3 : 0,
        src->Ap_sm, src->Ap_lg, row0, nrows, db3);
    // the split-f16 rows of the screen: range -> centre and bound -> split
    const Db3View v = db3_view(db3, nrows);
    IA_HIP(hipMemsetAsync(v.meta->rng, 0xff, sizeof(v.meta->rng), st));
    IA_HIP(hipMemsetAsync(&v.meta->amax_bits, 0, sizeof(unsigned int), st));
    k_db3_range<<<(unsigned)((nrows + C3_RB - 1) / C3_RB), D3P, 0, st>>>(v.rows, nrows, v.meta);
    k_db3_bound<<<(unsigned)((nrows + 255) / 256), 256, 0, st>>>(v.rows, nrows, v.meta);
    k_db3_split<<<(unsigned)((v.ntiles * 32 + 255) / 256), 256, 0, st>>>(v.rows, nrows, v.meta, v.db16);
    IA_LAUNCH_CHECK("ia_db3_build");
    return IA_OK;
}

int ia_level_features3_f64(const double *sm, int hs, int ws, const double *lg, int h, int w,
                           int full, double *out, void *stream) {
    IA_ARG(sm && lg && out && hs > 0 && ws > 0 && h > 0 && w > 0, "ia_level_features3_f64: bad args");
    const int nf = full ? D3_FULL : D3_HALF;
    const long n = (long)h * w * nf;
    k_level_features3<<<(unsigned)((n + 255) / 256), 256, 0, S(stream)>>>(Img3{sm, hs, ws},
                                                                         Img3{lg, h, w}, nf, out);
    IA_LAUNCH_CHECK("k_level_features3");
    return IA_OK;
}

int ia_coherence_pick3(const double *rows, int n, const double *q, int32_t *out, void *stream) {
    IA_ARG(rows && q && out && n > 0 && n <= 64, "ia_coherence_pick3: bad args");
    k_coherence_pick3<<<1, 64, 0, S(stream)>>>(rows, n, q, out);
    IA_LAUNCH_CHECK("k_coherence_pick3");
    return IA_OK;
}

int ia_wdist3_batch(const double *a, const double *q, const double *w, int n, double *out,
                    void *stream) {
    IA_ARG(a && q && w && out && n > 0, "ia_wdist3_batch: bad args");
    k_wdist3<<<(n + 63) / 64, 64, 0, S(stream)>>>(a, q, w, n, out);
    IA_LAUNCH_CHECK("k_wdist3");
    return IA_OK;
}

size_t ia_match3_workspace_bytes(int M, long nrows) {
    return align_up((size_t)M * D3P * sizeof(double), 256) + align_up((size_t)M * sizeof(Best), 256) +
           align_up((size_t)M * match3_blocks(nrows) * sizeof(Best), 256);
}

int ia_match3_batch(const double *db3, long nrows, const double *q165, int M, int64_t *idx,
                    double *dist, void *workspace, void *stream) {
    IA_ARG(db3 && q165 && workspace && M > 0 && nrows > 0, "ia_match3_batch: bad args");
    hipStream_t st = S(stream);
    char *ws = reinterpret_cast<char *>(workspace);
    double *q3 = reinterpret_cast<double *>(ws);
    Best *best = reinterpret_cast<Best *>(ws + align_up((size_t)M * D3P * sizeof(double), 256));
    Best *part = reinterpret_cast<Best *>(reinterpret_cast<char *>(best) + align_up((size_t)M * sizeof(Best), 256));
    IA_HIP(hipMemsetAsync(q3, 0, (size_t)M * D3P * sizeof(double), st));
    IA_HIP(hipMemcpy2DAsync(q3, D3P * sizeof(double), q165, D3 * sizeof(double), D3 * sizeof(double),
                            M, hipMemcpyDeviceToDevice, st));
    const int nb = match3_blocks(nrows);
    k_match3<<<nb, 256, 0, st>>>(db3, nrows, 0, q3, M, part);
    k_reduce3<<<M, 256, 0, st>>>(part, nb, best);
    k_split_best3<<<(M + 255) / 256, 256, 0, st>>>(best, M, idx, dist);
    IA_LAUNCH_CHECK("ia_match3_batch");
    return IA_OK;
}

int ia_lsh3_match_batch(const double *db3, long nrows, const double *center, const IaLsh *lsh,
                        const double *q165, int M, int64_t *idx, double *dist, void *stream) {
    IA_ARG(db3 && center && lsh && q165 && M > 0 && nrows > 0, "ia_lsh3_match_batch: bad args");
    {
        const int rc = lsh3_check(lsh, "ia_lsh3_match_batch");
        if (rc) return rc;
    }
    Fin3 f{};
    f.db3 = db3;
    f.q3 = q165;
    k_lsh3_pixel<false><<<M, 256, 0, S(stream)>>>(f, lsh3_view(lsh, nrows), center, nrows, D3, idx, dist);
    IA_LAUNCH_CHECK("k_lsh3_pixel");
    return IA_OK;
}

size_t ia_synth3_workspace_bytes(int H, int W, long nrows) { return ws3_layout(H, W, nrows, nullptr, nullptr); }

size_t ia_synth3_shard_workspace_bytes(int H, int W, long nrows, int nranks) {
    if (H <= 0 || W <= 0 || nrows <= 0 || nranks <= 0) return 0;
    return ws3_layout(H, W, nrows, nullptr, nullptr, nranks);
}

int ia_level3_resources(const IaSynthArgs *a, int *out) {
    IA_ARG(a && out && a->nrows > 0, "ia_level3_resources: bad args");
    IA_SRC_NA(a->src, "ia_level3_resources");
    const bool rot = g_color16.load(std::memory_order_relaxed) != 0 && a->dbr && a->rot;
    hipFuncAttributes f{}, sc{};
    IA_HIP(hipFuncGetAttributes(&f, reinterpret_cast<const void *>(&k_peer_finish3)));
    IA_HIP(hipFuncGetAttributes(&sc, rot ? reinterpret_cast<const void *>(&k_screen3r)
                                         : reinterpret_cast<const void *>(&k_screen3)));
    out[0] = (int)f.sharedSizeBytes;
    out[1] = f.numRegs;
    out[2] = (int)sc.sharedSizeBytes;
    out[3] = sc.numRegs;
    return IA_OK;
}

size_t ia_db3_rot_bytes(long nrows) { return nrows > 0 ? db3r_tiles_bytes(nrows) + sizeof(Rot3Meta) : 0; }

size_t ia_db3_cov_bytes(void) {
    return (size_t)(D3 * D3P + D3P + C3C_SPLIT * D3P + (size_t)C3C_SPLIT * D3 * D3P) * sizeof(double);
}

int ia_db3_cov(const double *db3, long nrows, double *cov, void *stream) {
    IA_ARG(db3 && cov && nrows > 0, "ia_db3_cov: bad args");
    hipStream_t st = S(stream);
    const long step = nrows / 65536 > 1 ? nrows / 65536 : 1;
    const long nsamp = (nrows + step - 1) / step;
    double *mean = cov + D3 * D3P, *cpart = mean + D3P, *vpart = cpart + C3C_SPLIT * D3P;
    k_db3_colsum<<<C3C_SPLIT, 256, 0, st>>>(db3, step, nsamp, cpart);
    k_db3_mean<<<1, 256, 0, st>>>(cpart, nsamp, mean);
    k_db3_cov<<<dim3(C3C_NA, C3C_SPLIT), 256, 0, st>>>(db3, step, nsamp, mean, vpart);
    k_db3_cov_reduce<<<D3, 256, 0, st>>>(vpart, cov);
    IA_LAUNCH_CHECK("ia_db3_cov");
    return IA_OK;
}
int ia_db3_rot_components(void) { return R3_P; }
int ia_db3_rot_floats(void) { return R3_ROT_FLOATS; }

int ia_db3_build_rot(const double *db3, long nrows, const float *rot, void *dbr, void *stream) {
    IA_ARG(db3 && rot && dbr && nrows > 0, "ia_db3_build_rot: bad args");
    hipStream_t st = S(stream);
    {
        const int rc = rot_check_orthonormal(rot, D3, R3_LD, st, "ia_db3_build_rot");
        if (rc) return rc;
    }
    const Db3View v = db3_view(const_cast<double *>(db3), nrows);
    Rot3Meta *rm = db3r_meta(dbr, nrows);
    IA_HIP(hipMemsetAsync(rm, 0, sizeof(Rot3Meta), st));
    k_db3_rot<<<(unsigned)v.ntiles, 256, 0, st>>>(v.rows, nrows, v.meta, rot, reinterpret_cast<half8 *>(dbr), rm);
    IA_LAUNCH_CHECK("ia_db3_build_rot");
    return IA_OK;
}

/* diagnostics: A_skip of a rotated 3-channel DB and the R16c screen of M given query rows
 * (M x 165): tile minima in unscaled units e[M][ntiles], eps (r3_eps) and |q'|^2 per query */
int ia_diag_db3_askip(const void *dbr, long nrows, float *out) {
    IA_ARG(dbr && out && nrows > 0, "ia_diag_db3_askip: bad args");
    unsigned int b = 0;
    IA_HIP(hipMemcpy(&b, &db3r_meta(const_cast<void *>(dbr), nrows)->askip_bits, 4, hipMemcpyDeviceToHost));
    std::memcpy(out, &b, 4);
    return IA_OK;
}

int ia_synth3_status(const IaSynthArgs *levels, int n, void *stream) {
    return levels_status(
        "ia_synth3_status", levels, n, stream,
        [](const IaSynthArgs &a) {
            Ws3 w{};
            ws3_layout(a.H, a.W, a.nrows, reinterpret_cast<char *>(a.workspace), &w);
            return w.ctl + C3_CTL_ERR;
        },
        // a sharded level's peer waits (k_peer_finish3) report through the exchange's error word
        [](const IaSynthArgs &a) { return comm_peer_mcap(a.comm) > 0 ? ia_peer_status(a.comm) : IA_OK; });
}

int ia_synth_level3(const IaSynthArgs *a, void *stream) {
    hipStream_t st = S(stream);
    Level3 run;
    int rc = run.init(a, st);
    if (rc) return rc;
    for (int t = 0; t < run.nw; ++t)
        if ((rc = run.wave(t, st))) return rc;
    return IA_OK;
}

/* n consecutive 3-channel levels through the level pipeline of ia_synth_levels (ia_pipe.h),
 * every level enqueued whole, coarse to fine (order 1): a level's waits name events already
 * recorded.  Finest-first as the luminance path (IA_PIPE_ORDER 0) is a speed change yet to be
 * measured here.
 * K > 1 (ia_synth_levels3_batch): levels[j * K + k] is level j of job k; every level's run is
 * job 0's Level3 with the other jobs as its parts and one job table, and every wave is one
 * set of launches for the K jobs. */
static int synth_levels3(const IaSynthArgs *levels, int n, int K, void *stream) {
    const std::string who = K > 1 ? "ia_synth_levels3_batch" : "ia_synth_levels3";
    IA_ARG(levels && n >= 1 && n <= 64, who + ": bad level count");
    for (int j = 1; j < n; ++j)
        for (int k = 0; k < K; ++k) {
            const IaSynthArgs &c = levels[(size_t)(j - 1) * K + k], &l = levels[(size_t)j * K + k];
            IA_ARG(l.Bp_sm == c.Bp_lg && l.B_hs == c.H && l.B_ws == c.W,
                   who + ": levels must be consecutive (level j's coarse B' = level j-1's B')");
        }
    // (an lsh that cannot run is refused before anything is enqueued)
    for (size_t i = 0; i < (size_t)n * K; ++i) {
        const int rc = lsh3_level_check(levels[i], who.c_str());
        if (rc) return rc;
    }
    // a batch: every job of a level in the same shapes and forms (checked before anything is
    // enqueued; the message names the field)
    if (K > 1) {
        IA_ARG(g_color16.load(std::memory_order_relaxed) != 0,
               who + ": K > 1 needs the screened matcher (IA_COLOR16=1)");
        for (int j = 0; j < n; ++j) {
            const IaSynthArgs &a = levels[(size_t)j * K];
            for (int k = 0; k < K; ++k) {
                const IaSynthArgs &b = levels[(size_t)j * K + k];
#define IA_SAME(field) IA_ARG(b.field == a.field, who + ": the jobs of a batch differ in " #field)
                IA_SAME(H); IA_SAME(W); IA_SAME(B_hs); IA_SAME(B_ws);
                IA_SAME(src.Ah); IA_SAME(src.Aw); IA_SAME(src.A_hs); IA_SAME(src.A_ws); IA_SAME(src.nAp); IA_SAME(src.nA);
                IA_SAME(nrows);
#undef IA_SAME
                // jobs passing one rotated DB are one DB group (ia_batch3_groups): it stands for
                // one database, so everything read with it is the same memory too
                for (int p = 0; p < k && b.dbr; ++p) {
                    const IaSynthArgs &c = levels[(size_t)j * K + p];
                    if (c.dbr != b.dbr) continue;
#define IA_SAME(field) IA_ARG(b.field == c.field, who + ": jobs sharing a dbr differ in " #field)
                    IA_SAME(db); IA_SAME(rot); IA_SAME(nrows);
                    IA_SAME(src.A_sm); IA_SAME(src.A_lg); IA_SAME(src.Ap_sm); IA_SAME(src.Ap_lg); IA_SAME(src.nA);
#undef IA_SAME
                    break;   // (p agrees with the group's earlier jobs already)
                }
                IA_ARG(!b.dbg_px == !a.dbg_px && !b.dbg_dist == !a.dbg_dist,
                       who + ": the jobs of a batch differ in having debug outputs (dbg_px, dbg_dist)");
                IA_ARG(!b.dbr == !a.dbr && !b.rot == !a.rot,
                       who + ": the jobs of a batch differ in having a rotated DB (dbr, rot)");
                IA_ARG(!b.comm, who + ": a batch takes no comm");
                IA_ARG(!b.lsh, who + ": a batch takes no lsh");
                IA_ARG(b.row0 == 0 && b.nrows == (long)b.src.nAp * b.src.Ah * b.src.Aw,
                       who + ": a batch takes no partial row range (row0, nrows)");
                IA_ARG(b.dbr && b.rot,
                       who + ": K > 1 needs the rotated DB (dbr, rot): the batch form exists for the R16c screen");
            }
        }
    }
    hipStream_t st = S(stream);
    int rc = g_pipe.begin(n, st);
    if (rc) return rc;
    // the job tables go through this thread's pinned staging buffer (ia_pipe.h)
    C3Job *pinned = nullptr;
    if (K > 1) IA_HIP(g_pipe.staging((size_t)n * K * sizeof(C3Job), reinterpret_cast<void **>(&pinned)));
    // Sharded levels (one exchange each) overlap over the device-side exchange, whose only
    // waits sit in k_peer_finish3's small workgroups; over RCCL, and between ranks sharing one
    // GPU (IA_SHARE_GPU=1), each one's first wave waits for the previous one's last, as for
    // luminance (ia_synth.hip synth_levels)
    static const int overlap = env_int("IA_SHARD_OVERLAP", 1) && !env_int("IA_SHARE_GPU", 0);
    auto multi_rank = [&](const IaSynthArgs &l) {
        if (l.comm == nullptr || l.nrows >= l.N_total) return false;
        return !(overlap && comm_peer_mcap(l.comm) > 0);
    };
    std::vector<Level3> run(n);
    std::vector<PipeLevel> pl(n);
    for (int j = 0; j < n; ++j) {
        if ((rc = g_pipe.level_begin(j)) ||
            (rc = run[j].init_batch(&levels[(size_t)j * K], K, g_pipe.stream(j), pinned ? pinned + (size_t)j * K : nullptr)))
            return rc;
        // (the fused tail's launch of wave t also builds wave t + 1's query rows)
        pl[j] = PipeLevel{run[j].H, run[j].W, run[j].fuse, multi_rank(levels[(size_t)j * K])};
    }
    return pipe_execute(run, pl, 1, 0, st);
}

int ia_synth_levels3(const IaSynthArgs *levels, int n, void *stream) { return synth_levels3(levels, n, 1, stream); }

int ia_synth_levels3_batch(const IaSynthArgs *levels, int n, int K, void *stream) {
    IA_ARG(K >= 1 && K <= IA_BATCH_MAX, "ia_synth_levels3_batch: K out of range (1 .. 128)");
    IA_ARG(levels && n >= 1 && n <= 64, "ia_synth_levels3_batch: bad level count");
    for (size_t i = 0; i < (size_t)n * K; ++i)   // (batches shard by job, not by rows)
        IA_ARG(!levels[i].comm, "ia_synth_levels3_batch: a batch takes no comm (sharded levels: ia_synth_levels3)");
    for (size_t i = 0; i < (size_t)n * K; ++i)   // (for any K: LSH jobs have an entry of their own)
        IA_ARG(!levels[i].lsh, "ia_synth_levels3_batch: a batch takes no lsh (LSH batches: ia_synth_levels3_lsh_batch)");
    return synth_levels3(levels, n, K, stream);
}

/* K LSH jobs per set of launches (k_query3b, k_lsh3_pixelb; K = 1: the single job's launches).
 * Everything that cannot run is refused here, before anything is enqueued; the message names
 * the field. */
int ia_synth_levels3_lsh_batch(const IaSynthArgs *levels, int n, int K, void *stream) {
    const std::string who = "ia_synth_levels3_lsh_batch";
    IA_ARG(K >= 1 && K <= IA_BATCH_MAX, who + ": K out of range (1 .. 128)");
    IA_ARG(levels && n >= 1 && n <= 64, who + ": bad level count");
    for (int j = 0; j < n; ++j) {
        const IaSynthArgs &a = levels[(size_t)j * K];
        for (int k = 0; k < K; ++k) {
            const IaSynthArgs &b = levels[(size_t)j * K + k];
            IA_ARG(b.db && b.B_sm && b.B_lg && b.Bp_sm && b.Bp_lg && b.weights && b.s && b.im && b.workspace &&
                       b.H > 0 && b.W > 0,
                   who + ": bad args");
            IA_ARG(b.lsh, who + ": every job of every level needs lsh (exact batches: ia_synth_levels3_batch)");
            IA_ARG(!b.comm, who + ": an lsh batch takes no comm (the LSH matcher runs unsharded)");
            IA_ARG(!b.dbg_px == !b.dbg_dist, who + ": debug outputs come in pairs (dbg_px, dbg_dist)");
            {
                const int rc = lsh3_level_check(b, who.c_str());   // center, tables
                if (rc) return rc;
            }
            if (j > 0) {
                const IaSynthArgs &c = levels[(size_t)(j - 1) * K + k];
                IA_ARG(b.Bp_sm == c.Bp_lg && b.B_hs == c.H && b.B_ws == c.W,
                       who + ": levels must be consecutive (level j's coarse B' = level j-1's B')");
            }
#define IA_SAME(field) IA_ARG(b.field == a.field, who + ": the jobs of an lsh batch differ in " #field)
            IA_SAME(H); IA_SAME(W); IA_SAME(B_hs); IA_SAME(B_ws);
            IA_SAME(src.Ah); IA_SAME(src.Aw); IA_SAME(src.A_hs); IA_SAME(src.A_ws); IA_SAME(src.nAp); IA_SAME(src.nA);
            IA_SAME(nrows); IA_SAME(lsh->L); IA_SAME(lsh->k);
#undef IA_SAME
            IA_ARG(b.row0 == 0 && b.nrows == (long)b.src.nAp * b.src.Ah * b.src.Aw,
                   who + ": an lsh batch takes no partial row range (row0, nrows)");
            IA_ARG(!b.dbg_px == !a.dbg_px,
                   who + ": the jobs of an lsh batch differ in having debug outputs (dbg_px, dbg_dist)");
            // jobs passing one table set are one DB group: it stands for one database, so
            // everything read with it is the same memory too
            for (int p = 0; p < k; ++p) {
                const IaSynthArgs &c = levels[(size_t)j * K + p];
                if (c.lsh->mem != b.lsh->mem) continue;
#define IA_SAME(field) IA_ARG(b.field == c.field, who + ": jobs sharing lsh->mem differ in " #field)
                IA_SAME(lsh->proj); IA_SAME(lsh->w); IA_SAME(center); IA_SAME(db);
                IA_SAME(src.A_sm); IA_SAME(src.A_lg); IA_SAME(src.Ap_sm); IA_SAME(src.Ap_lg); IA_SAME(src.nA);
#undef IA_SAME
                break;   // (p agrees with the group's earlier jobs already)
            }
        }
    }
    if (K == 1) return synth_levels3(levels, n, 1, stream);
    hipStream_t st = S(stream);
    int rc = g_pipe.begin(n, st);
    if (rc) return rc;
    // one job table per level, staged once through this thread's pinned buffer (ia_pipe.h)
    L3Job *pinned = nullptr;
    IA_HIP(g_pipe.staging((size_t)n * K * sizeof(L3Job), reinterpret_cast<void **>(&pinned)));
    std::vector<Level3> run(n);
    std::vector<PipeLevel> pl(n);
    for (int j = 0; j < n; ++j) {
        if ((rc = g_pipe.level_begin(j)) ||
            (rc = run[j].init_lsh_batch(&levels[(size_t)j * K], K, g_pipe.stream(j), pinned + (size_t)j * K)))
            return rc;
        pl[j] = PipeLevel{run[j].H, run[j].W, false, false};
    }
    return pipe_execute(run, pl, 1, 0, st);
}

int ia_batch3_groups(const IaSynthArgs *level_jobs, int K, int *group_of_job) {
    IA_ARG(level_jobs && group_of_job, "ia_batch3_groups: bad args");
    IA_ARG(K >= 1 && K <= IA_BATCH_MAX, "ia_batch3_groups: K out of range (1 .. 128)");
    for (int k = 0; k < K; ++k) IA_SRC_NA(level_jobs[k].src, "ia_batch3_groups");
    return batch3_groups(level_jobs, K, group_of_job);
}

int ia_diag_screen3(const void *db3, long nrows, const double *q165, int M, double *e, double *eps,
                    double *qn) {
    IA_ARG(db3 && q165 && e && eps && qn && nrows > 0 && M > 0, "ia_diag_screen3: bad args");
    const Db3View v = db3_view(const_cast<void *>(db3), nrows);
    const int QT = (M + 31) / 32, ntiles = (int)v.ntiles;
    half8 *q16 = nullptr;
    float *smin = nullptr;
    IA_HIP(hipMalloc(&q16, (size_t)QT * C16_TILE * sizeof(half8)));
    IA_HIP(hipMalloc(&smin, (size_t)M * c3_stride(ntiles) * sizeof(float)));
    k_qsplit3<<<QT * 32, 256>>>(q165, M, v.meta, qn, reinterpret_cast<_Float16 *>(q16));
    int tpw;
    k_screen3<<<screen3_grid(ntiles, M, tpw), 256>>>(v.db16, ntiles, q16, M, tpw, smin);
    const long n = (long)M * ntiles;
    k_screen3_unscale<<<(unsigned)((n + 255) / 256), 256>>>(smin, M, ntiles, qn, v.meta, e, eps);
    IA_LAUNCH_CHECK("ia_diag_screen3");
    IA_HIP(hipDeviceSynchronize());
    IA_HIP(hipFree(q16));
    IA_HIP(hipFree(smin));
    return IA_OK;
}

int ia_diag_screen3r(const void *db3, const void *dbr, const float *rot, long nrows, const double *q165, int M,
                     double *e, double *eps, double *qn) {
    IA_ARG(db3 && dbr && rot && q165 && e && eps && qn && nrows > 0 && M > 0, "ia_diag_screen3r: bad args");
    const Db3View v = db3_view(const_cast<void *>(db3), nrows);
    const int QT = (M + 31) / 32, ntiles = (int)v.ntiles;
    half8 *q16 = nullptr;
    float *smin = nullptr;
    double *nsk = nullptr;
    IA_HIP(hipMalloc(&q16, (size_t)QT * R3_TILE * sizeof(half8)));
    IA_HIP(hipMalloc(&smin, (size_t)M * c3_stride(ntiles) * sizeof(float)));
    IA_HIP(hipMalloc(&nsk, (size_t)QT * 32 * sizeof(double)));
    const Img3 z{nullptr, 0, 0};
    k_query3r<<<QT * 32, 256>>>(z, z, z, z, 0, 0, M, v.meta, rot, q165, nullptr, qn, nsk, q16);
    int tpw;
    k_screen3r<<<screen3r_grid(ntiles, M, tpw), 256>>>(reinterpret_cast<const half8 *>(dbr), ntiles, q16, M, tpw,
                                                        smin);
    const long n = (long)M * ntiles;
    k_screen3_unscale<<<(unsigned)((n + 255) / 256), 256>>>(smin, M, ntiles, qn, v.meta, e, eps, nsk,
                                                            db3r_meta(const_cast<void *>(dbr), nrows));
    IA_LAUNCH_CHECK("ia_diag_screen3r");
    IA_HIP(hipDeviceSynchronize());
    IA_HIP(hipFree(q16));
    IA_HIP(hipFree(smin));
    IA_HIP(hipFree(nsk));
    return IA_OK;
}

int ia_diag_set_color16(int on) {
    const int prev = g_color16.load();
    if (on == 0 || on == 1) g_color16.store(on);
    return prev;
}

int ia_diag_set_c3_shared_screen(int on) {
    const int prev = g_c3_shared_screen.load();
    if (on == 0 || on == 1) g_c3_shared_screen.store(on);
    return prev;
}

// the colour exact stage's counters since the last call: [candidate tiles rescored, queries
// that scanned every tile]; the first call allocates them (and returns zeros)
int ia_diag_color16_stats(unsigned long long *out) {
    IA_ARG(out, "ia_diag_color16_stats: bad args");
    if (!g_c3_stats) {
        IA_HIP(hipMalloc(&g_c3_stats, 2 * sizeof(unsigned long long)));
        IA_HIP(hipMemset(g_c3_stats, 0, 2 * sizeof(unsigned long long)));
        out[0] = out[1] = 0;
        return IA_OK;
    }
    IA_HIP(hipDeviceSynchronize());
    IA_HIP(hipMemcpy(out, g_c3_stats, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    IA_HIP(hipMemset(g_c3_stats, 0, 2 * sizeof(unsigned long long)));
    return IA_OK;
}

}  // extern "C"
