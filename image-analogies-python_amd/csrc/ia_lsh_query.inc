// The body of k_lsh_query (one job, by-value arguments) and k_lsh_query_b (a batch, job table):
// included once in each, so both kernels are compiled from this one text.  In scope: src, row0,
// nrows, npad, start, bits, rows, proj, L, k, w, q64, center, best, stats; the query is
// blockIdx.x.  (ia_lsh.hip has the description.)
    __shared__ double qs[IA_DP];
    __shared__ float qc[IA_DP];
    __shared__ unsigned int hk[LSH_MAXH];
    __shared__ int lo_s[LSH_MAXH + 1], n_s[LSH_MAXH + 1];
    const int q = blockIdx.x, lane = threadIdx.x;
    if (lane < IA_DP) {
        qs[lane] = q64[(long)q * IA_DP + lane];
        qc[lane] = lane < IA_D ? (float)(qs[lane] - center[lane]) : 0.f;
    }
    __syncthreads();
    if (lane < L * k) {
        const auto *p = proj + lane * IA_DP;
        float d = p[55];
        for (int e = 0; e < IA_D; ++e) d = fmaf(p[e], qc[e], d);
        hk[lane] = lsh_mix((int)floorf(d / w), lane % k);
    }
    __syncthreads();
    if (lane < L) {
        unsigned int key = 0;
        for (int i = 0; i < k; ++i) key += hk[lane * k + i];
        key &= (1u << bits) - 1u;
        const auto *st = start + (long)lane * ((1L << bits) + 1);
        long lo = st[key], hi = st[key + 1];
        if (lo == hi) {   // empty bucket: take the neighbouring entries of the sorted table
            lo = lo >= 2 ? lo - 2 : 0;
            hi = lo + 4 < nrows ? lo + 4 : nrows;
        }
        lo_s[lane] = (int)lo;
        n_s[lane] = (int)(hi - lo > LSH_CAP ? LSH_CAP : hi - lo);
    }
    __syncthreads();
    if (lane == 0) {   // exclusive prefix of the per-table counts in n_s (in place)
        int acc = 0;
        for (int t = 0; t < L; ++t) { const int c = n_s[t]; n_s[t] = acc; acc += c; }
        n_s[L] = acc;
    }
    __syncthreads();
    const int total = n_s[L];
    double bd = INFINITY;
    long long bi = 0x7fffffffffffffffLL;
    int ncand = 0;
    int t = 0;
    for (int c = lane; c < total; c += 64) {   // candidates of all tables over the lanes
        while (n_s[t + 1] <= c) ++t;
        const int lr = rows[(long)t * npad + lo_s[t] + (c - n_s[t])];
        if (lr < nrows) {
            lbest(bd, bi, row_dist2(src, row0 + lr, qs), row0 + lr);
            ++ncand;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double od = __shfl_xor(bd, o);
        const long long oi = __shfl_xor(bi, o);
        lbest(bd, bi, od, oi);
        ncand += __shfl_xor(ncand, o);
    }
    if (lane == 0) {
        best[q] = Best{bd, bi == 0x7fffffffffffffffLL ? row0 : bi};
        if (stats) atomicAdd(&stats_slot(stats, q)[0], (unsigned long long)ncand);
    }
