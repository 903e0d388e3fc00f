// ia_lsh.hip — LSH matcher (config c2 "LSH vs GPU brute force").
//
// The reference snapshot has no LSH code (only the artefact output/freud-crop-filt-lsh.jpg),
// so this is the build's own definition: E2LSH over the same centred rows a' = a - c the
// exact matcher screens.  L tables, each k concatenated hashes
//     h_i(x) = floor((p_i . x + b_i) / w),   p_i ~ N(0, I_55),  b_i ~ U[0, w)
// (projections drawn on the host with a seeded RandomState), combined into a 32-bit key
// per table and masked to B = lsh_bits(nrows) bits (2^B >= 2 nrows buckets).  Build: one
// pass over the fp32 DB computes L keys per row, one hipCUB radix sort of (key, row)
// pairs per table, and a bucket directory start[t][0..2^B] (counting-sort offsets).
// The rows' centred fp32 values are gathered from the pyramids like the DB build's.
// Query (one wave per query): L keys, two directory loads per table, and the exact fp64
// distance (the oracle's pairwise-8 value) of up to LSH_CAP rows per bucket, spread over
// the wave's lanes; the lexicographic (distance, row) minimum is returned.
// Approximate by construction: the exact matcher is the default.
// 3-channel matching (165-dim rows) keeps the definition with D = 165: ia_lsh3_build makes the
// same tables from the materialised fp64 rows of ia_db3_build (k_lsh3_keys, then the shared
// sort and directory); its queries are ia_color3.hip's k_lsh3_pixel.
#include "ia_internal.h"

#include <hipcub/hipcub.hpp>

namespace ia {

// (LSH_MAXH, LSH_CAP, lsh_bits, lsh_mix: ia_internal.h, shared with the 165-dim tables)

// keys_in[t][r] for the local rows r of [row0, row0 + nrows): the centred fp32 values
// fl32(a_k - c_k) gathered from the pyramids (the rows the exact matcher screens)
__global__ __launch_bounds__(256) void k_lsh_keys(DbSrc src, long row0, long nrows, long npad,
                                                  const double *__restrict__ center,
                                                  const float *__restrict__ proj,
                                                  int L, int k, float w, int bits,
                                                  unsigned int *__restrict__ keys,
                                                  int *__restrict__ rows) {
    __shared__ float P[LSH_MAXH * IA_DP];
    for (int i = threadIdx.x; i < L * k * IA_DP; i += 256) P[i] = proj[i];
    __syncthreads();
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r >= npad) return;
    float a[IA_DP];
    {
        ImgPair ai, ap; int rr, cc;
        src.locate(row0 + (r < nrows ? r : nrows - 1), ai, ap, rr, cc);
        emit_feature(ai, ap, rr, cc, [&](int kk, double v) { a[kk] = (float)(v - center[kk]); });
    }
    for (int t = 0; t < L; ++t) {
        unsigned int key = 0;
        for (int i = 0; i < k; ++i) {
            const float *p = P + (t * k + i) * IA_DP;
            float d = p[55];
#pragma unroll
            for (int e = 0; e < IA_D; ++e) d = fmaf(p[e], a[e], d);
            key += lsh_mix((int)floorf(d / w), i);
        }
        // rows past nrows (sentinels) get the key 2^bits, beyond every bucket
        const unsigned int mask = (1u << bits) - 1u;
        keys[(long)t * npad + r] = r < nrows ? (key & mask) : mask + 1u;
        rows[(long)t * npad + r] = (int)r;
    }
}

// bucket directory: start[t][b] = first sorted position with key >= b, b in [0, 2^bits]
__global__ __launch_bounds__(256) void k_lsh_dir(const unsigned int *__restrict__ keys, long npad,
                                                 int bits, int *__restrict__ start) {
    const int t = blockIdx.y;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= npad) return;
    const unsigned int *kt = keys + (long)t * npad;
    int *st = start + (long)t * ((1L << bits) + 1);
    const long kp = i > 0 ? (long)kt[i - 1] : -1;
    const long kc = kt[i];
    for (long b = kp + 1; b <= kc; ++b) st[b] = (int)i;
    if (i == npad - 1)   // sentinels hold key 2^bits: nothing beyond
        for (long b = kc + 1; b <= (1L << bits); ++b) st[b] = (int)npad;
}

// ---- keys of 165-dim rows (3-channel matching: the materialised fp64 rows of ia_db3_build,
// LSH3_PD doubles apart).  The luminance kernel's whole row per thread would spill at 165
// floats, so a workgroup stages the projections (odd LDS stride: lanes of consecutive hashes
// on distinct banks) and a tile of K3_ROWS centred fp32 rows (coalesced reads of the 1,344-B
// rows) in LDS; threads then take (row, hash) pairs, each the 165-term fmaf chain in the
// definition's order, and (row, table) pairs sum the k mixed hashes into the key.  A workgroup
// walks tiles blockIdx.x, + gridDim.x, ...: the projections are staged once per workgroup.
constexpr int K3_ROWS = 16, K3_PS = LSH3_PD + 1;
__global__ __launch_bounds__(256) void k_lsh3_keys(const double *__restrict__ db3, long nrows, long npad,
                                                   const double *__restrict__ center,
                                                   const float *__restrict__ proj, int L, int k,
                                                   float w, int bits, unsigned int *__restrict__ keys,
                                                   int *__restrict__ rows) {
    __shared__ float P[LSH_MAXH * K3_PS];          // 43,264 B
    __shared__ float X[K3_ROWS * LSH3_PD];         // 10,752 B
    __shared__ double cs[LSH3_PD];
    __shared__ unsigned int hk[K3_ROWS * LSH_MAXH];
    const int tid = threadIdx.x, nh = L * k;
    for (int i = tid; i < nh * LSH3_PD; i += 256) {
        const int h = i / LSH3_PD, e = i - h * LSH3_PD;
        P[h * K3_PS + e] = proj[i];
    }
    for (int e = tid; e < LSH3_PD; e += 256) cs[e] = e < LSH3_D ? center[e] : 0.0;
    const unsigned int mask = (1u << bits) - 1u;
    for (long r0 = (long)blockIdx.x * K3_ROWS; r0 < npad; r0 += (long)gridDim.x * K3_ROWS) {
        __syncthreads();   // cs and P staged; the previous tile's X and hk consumed
        for (int i = tid; i < K3_ROWS * LSH3_PD; i += 256) {
            const int rr = i / LSH3_PD, e = i - rr * LSH3_PD;
            const long r = r0 + rr < nrows ? r0 + rr : nrows - 1;   // (sentinel rows: key unused)
            X[i] = e < LSH3_D ? (float)(db3[r * LSH3_PD + e] - cs[e]) : 0.f;
        }
        __syncthreads();
        for (int i = tid; i < K3_ROWS * nh; i += 256) {
            const int rr = i / nh, h = i - rr * nh;
            const float *p = P + h * K3_PS, *a = X + rr * LSH3_PD;
            float d = p[LSH3_D];
#pragma unroll 5
            for (int e = 0; e < LSH3_D; ++e) d = fmaf(p[e], a[e], d);
            hk[rr * LSH_MAXH + h] = lsh_mix((int)floorf(d / w), h % k);
        }
        __syncthreads();
        for (int i = tid; i < K3_ROWS * L; i += 256) {
            const int t = i / K3_ROWS, rr = i - t * K3_ROWS;
            const long r = r0 + rr;
            unsigned int key = 0;
            for (int j = 0; j < k; ++j) key += hk[rr * LSH_MAXH + t * k + j];
            // rows past nrows (sentinels) get the key 2^bits, beyond every bucket
            keys[(long)t * npad + r] = r < nrows ? (key & mask) : mask + 1u;
            rows[(long)t * npad + r] = (int)r;
        }
    }
}

__device__ __forceinline__ void lbest(double &bd, long long &bi, double d, long long i) {
    if (d < bd || (d == bd && i < bi)) { bd = d; bi = i; }
}

// one 64-lane wave per query
__global__ __launch_bounds__(64) void k_lsh_query(DbSrc src, long row0, long nrows, long npad,
                                                  const int *__restrict__ start, int bits,
                                                  const int *__restrict__ rows,
                                                  const float *__restrict__ proj, int L, int k,
                                                  float w, const double *__restrict__ q64,
                                                  const double *__restrict__ center,
                                                  Best *__restrict__ best,
                                                  unsigned long long *stats) {
#include "ia_lsh_query.inc"
}

// a batch of K LSH jobs (ia_synth_levels_lsh_batch): the same query with the job as
// blockIdx.y, everything of job k from entry k of the device job table
__global__ __launch_bounds__(64) void k_lsh_query_b(const LJob *__restrict__ jobs) {
    const LJob &J = jobs[blockIdx.y];
    const DbSrc src = J.src();
    const long row0 = J.row0, nrows = J.nrows, npad = J.npad;
    const int bits = J.bits, L = J.L, k = J.k;
    const float w = J.w;
    const auto *__restrict__ start = J.start.p;
    const auto *__restrict__ rows = J.rows.p;
    const auto *__restrict__ proj = J.proj.p;
    const auto *__restrict__ q64 = J.q64.p;
    const auto *__restrict__ center = J.center.p;
    auto *__restrict__ best = J.best.p;
    unsigned long long *stats = J.stats;
#include "ia_lsh_query.inc"
}

// device layout of IaLsh::mem: rows[L][npad] | start[L][2^bits + 1] | keys[L][npad] |
// keys_in[L][npad] | rows_in[L][npad] | sort temp (the last four only used by the build)
struct LshLayout {
    size_t rows, start, keys, keys_in, rows_in, tmp, total;
};
static size_t sort_temp_bytes(long npad, int bits);
// (npad: the padded row count, db_rows_padded(nrows) for the luminance tables,
// lsh3_rows_padded(nrows) for the 165-dim ones)
static LshLayout lsh_layout_n(long nrows, long npad, int L) {
    const int bits = lsh_bits(nrows);
    const size_t tab = align_up((size_t)L * npad * 4, 256);
    LshLayout y;
    y.rows = 0;
    y.start = tab;
    y.keys = y.start + align_up((size_t)L * ((1L << bits) + 1) * 4, 256);
    y.keys_in = y.keys + tab;
    y.rows_in = y.keys_in + tab;
    y.tmp = y.rows_in + tab;
    y.total = y.tmp + align_up(sort_temp_bytes(npad, bits), 256);
    return y;
}
static LshLayout lsh_layout(long nrows, int L) { return lsh_layout_n(nrows, db_rows_padded(nrows), L); }

// the tables of npad padded rows from their unsorted (key, row) pairs in keys_in / rows_in: one
// stable radix sort per table, then the bucket directory
static int lsh_sort_tables(char *m, const LshLayout &y, long npad, int bits, int L, hipStream_t st,
                           const char *who) {
    int *rows = reinterpret_cast<int *>(m + y.rows);
    int *start = reinterpret_cast<int *>(m + y.start);
    unsigned int *keys = reinterpret_cast<unsigned int *>(m + y.keys);
    unsigned int *keys_in = reinterpret_cast<unsigned int *>(m + y.keys_in);
    int *rows_in = reinterpret_cast<int *>(m + y.rows_in);
    void *tmp = m + y.tmp;
    size_t tb = sort_temp_bytes(npad, bits);
    IA_ARG(tb > 0, std::string(who) + ": radix-sort size query failed");
    for (int t = 0; t < L; ++t) {
        IA_HIP(hipcub::DeviceRadixSort::SortPairs(tmp, tb, keys_in + (long)t * npad,
                                                  keys + (long)t * npad, rows_in + (long)t * npad,
                                                  rows + (long)t * npad, (int)npad, 0, bits + 1,
                                                  st));
    }
    k_lsh_dir<<<dim3((unsigned)((npad + 255) / 256), L), 256, 0, st>>>(keys, npad, bits, start);
    IA_LAUNCH_CHECK("k_lsh_dir");
    return IA_OK;
}

int lsh3_check(const IaLsh *lsh, const char *who) {
    IA_ARG(lsh->mem && lsh->proj, std::string(who) + ": lsh without tables (mem, proj)");
    IA_ARG((reinterpret_cast<uintptr_t>(lsh->proj) & 15) == 0,
           std::string(who) + ": lsh proj must be 16-byte aligned");
    IA_ARG(lsh->L >= 1 && lsh->k >= 1 && lsh->L * lsh->k <= LSH_MAXH && lsh->w > 0.f,
           std::string(who) + ": lsh needs 1 <= L*k <= 64 and w > 0");
    return IA_OK;
}

Lsh3View lsh3_view(const IaLsh *lsh, long nrows) {
    const long npad = lsh3_rows_padded(nrows);
    const LshLayout y = lsh_layout_n(nrows, npad, lsh->L);
    const char *m = reinterpret_cast<const char *>(lsh->mem);
    return Lsh3View{reinterpret_cast<const int *>(m + y.rows), reinterpret_cast<const int *>(m + y.start),
                    lsh->proj, lsh->L, lsh->k, lsh_bits(nrows), lsh->w, npad};
}

int launch_lsh_match(const IaLsh *lsh, const DbSrc &src, long row0, long nrows, int M,
                     const double *q64, const double *center, Best *best,
                     unsigned long long *stats, hipStream_t st) {
    const long npad = db_rows_padded(nrows);
    const LshLayout y = lsh_layout(nrows, lsh->L);
    const char *m = reinterpret_cast<const char *>(lsh->mem);
    k_lsh_query<<<M, 64, 0, st>>>(src, row0, nrows, npad,
                                  reinterpret_cast<const int *>(m + y.start), lsh_bits(nrows),
                                  reinterpret_cast<const int *>(m + y.rows), lsh->proj, lsh->L,
                                  lsh->k, lsh->w, q64, center, best, stats);
    IA_LAUNCH_CHECK("k_lsh_query");
    return IA_OK;
}

int lsh_check(const IaLsh *lsh, const char *who) {
    IA_ARG(lsh->mem && lsh->proj, std::string(who) + ": lsh without tables (mem, proj)");
    IA_ARG(lsh->L >= 1 && lsh->k >= 1 && lsh->L * lsh->k <= LSH_MAXH && lsh->w > 0.f,
           std::string(who) + ": lsh needs 1 <= L*k <= 64 and w > 0");
    return IA_OK;
}

// what a query reads of an ia_lsh_build table set, into a batch's job entry
void lsh_job_tables(const IaLsh *lsh, long nrows, LJob *J) {
    const LshLayout y = lsh_layout(nrows, lsh->L);
    const char *m = reinterpret_cast<const char *>(lsh->mem);
    J->start = reinterpret_cast<const int *>(m + y.start);
    J->rows = reinterpret_cast<const int *>(m + y.rows);
    J->proj = lsh->proj;
    J->L = lsh->L;
    J->k = lsh->k;
    J->bits = lsh_bits(nrows);
    J->w = lsh->w;
    J->npad = db_rows_padded(nrows);
}

int launch_lsh_match_batch(const LJob *jobs, int K, int M, hipStream_t st) {
    k_lsh_query_b<<<dim3(M, K), 64, 0, st>>>(jobs);
    IA_LAUNCH_CHECK("k_lsh_query_b");
    return IA_OK;
}

static size_t sort_temp_bytes(long npad, int bits) {
    size_t tb = 0;
    if (hipcub::DeviceRadixSort::SortPairs(nullptr, tb, (unsigned int *)nullptr,
                                           (unsigned int *)nullptr, (int *)nullptr,
                                           (int *)nullptr, (int)npad, 0, bits + 1) != hipSuccess)
        return 0;
    return tb;
}

}  // namespace ia

using namespace ia;

extern "C" {

size_t ia_lsh_bytes(long nrows, int L) {
    if (nrows <= 0 || L <= 0) return 0;
    return lsh_layout(nrows, L).total;
}

int ia_lsh_bits(long nrows) { return nrows > 0 ? lsh_bits(nrows) : 0; }

int ia_lsh_build(const IaSrcLevel *src, long row0, long nrows, const double *center,
                 const IaLsh *lsh, void *stream) {
    IA_ARG(src && center && lsh && lsh->mem && lsh->proj && nrows > 0 && row0 >= 0,
           "ia_lsh_build: bad args");
    IA_SRC_NA(*src, "ia_lsh_build");
    IA_ARG(lsh->L >= 1 && lsh->k >= 1 && lsh->L * lsh->k <= LSH_MAXH && lsh->w > 0.f,
           "ia_lsh_build: need 1 <= L*k <= 64 and w > 0");
    IA_ARG(nrows < (1L << 31), "ia_lsh_build: too many rows");
    hipStream_t st = S(stream);
    const long npad = db_rows_padded(nrows);
    const int bits = lsh_bits(nrows);
    const LshLayout y = lsh_layout(nrows, lsh->L);
    char *m = reinterpret_cast<char *>(lsh->mem);
    IA_ARG(sort_temp_bytes(npad, bits) > 0, "ia_lsh_build: radix-sort size query failed");
    const unsigned nb = (unsigned)((npad + 255) / 256);
    k_lsh_keys<<<nb, 256, 0, st>>>(make_dbsrc(*src), row0, nrows, npad, center, lsh->proj,
                                   lsh->L, lsh->k, lsh->w, bits,
                                   reinterpret_cast<unsigned int *>(m + y.keys_in),
                                   reinterpret_cast<int *>(m + y.rows_in));
    IA_LAUNCH_CHECK("k_lsh_keys");
    return lsh_sort_tables(m, y, npad, bits, lsh->L, st, "ia_lsh_build");
}

size_t ia_lsh3_bytes(long nrows, int L) {
    if (nrows <= 0 || L <= 0) return 0;
    return lsh_layout_n(nrows, lsh3_rows_padded(nrows), L).total;
}

int ia_lsh3_build(const double *db3, long nrows, const double *center, const IaLsh *lsh, void *stream) {
    IA_ARG(db3 && center && lsh && nrows > 0, "ia_lsh3_build: bad args");
    {
        const int rc = lsh3_check(lsh, "ia_lsh3_build");
        if (rc) return rc;
    }
    IA_ARG(nrows < (1L << 31) - 256, "ia_lsh3_build: too many rows");
    hipStream_t st = S(stream);
    const long npad = lsh3_rows_padded(nrows);
    const int bits = lsh_bits(nrows);
    const LshLayout y = lsh_layout_n(nrows, npad, lsh->L);
    char *m = reinterpret_cast<char *>(lsh->mem);
    IA_ARG(sort_temp_bytes(npad, bits) > 0, "ia_lsh3_build: radix-sort size query failed");
    // (at most 1,024 workgroups walk the tiles: the projections are staged once per workgroup)
    const long tiles = npad / K3_ROWS;
    k_lsh3_keys<<<(unsigned)(tiles < 1024 ? tiles : 1024), 256, 0, st>>>(
        db3, nrows, npad, center, lsh->proj, lsh->L, lsh->k, lsh->w, bits,
        reinterpret_cast<unsigned int *>(m + y.keys_in), reinterpret_cast<int *>(m + y.rows_in));
    IA_LAUNCH_CHECK("k_lsh3_keys");
    return lsh_sort_tables(m, y, npad, bits, lsh->L, st, "ia_lsh3_build");
}

}  // extern "C"
