// The body of k_lsh3_pixel (one job, by-value arguments) and k_lsh3_pixelb (a batch, job table):
// included once in each, so both kernels are compiled from this one text.  In scope: TAIL, f
// (Fin3; t, y_lo: the wave's), lv (Lsh3View), center, nrows, qstride, idx, dist; the pixel is
// m = blockIdx.x.  (ia_color3.hip has the description.)
    __shared__ double qs[D3P], wsh[D3P];
    __shared__ __attribute__((aligned(16))) float qc[D3P];
    __shared__ unsigned int hk[LSH_MAXH];
    __shared__ int lo_s[LSH_MAXH + 1], n_s[LSH_MAXH + 1];
    __shared__ Acc8 acc[32 * 8];                // a pass's rows (32 x 8 parts)
    __shared__ Acc8 cacc[15 * 8];               // the coherence rows
    __shared__ double sump[15], sumw[15];
    __shared__ long long rix[15];
    __shared__ int rpos[15][3];
    __shared__ double rd[4], rw[4];
    __shared__ long long ri[4];
    constexpr long long NONE = 0x7fffffffffffffffLL;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int m = blockIdx.x;
    const int ro = tid >> 3, j = tid & 7;
    const int y = f.y_lo + m, x = f.t - 3 * y;
    // ---- one round trip: query, weights, coherence s / im
    if (tid < D3P) {
        const double q = tid < D3 ? f.q3[(long)m * qstride + tid] : 0.0;
        qs[tid] = q;
        wsh[tid] = TAIL && tid < D3 ? f.weights[tid] : 0.0;
        qc[tid] = tid < D3 ? (float)(q - center[tid]) : 0.f;
    }
    if (TAIL && tid < 15) c3_window(tid, y, x, f, rix, rpos);
    __syncthreads();
    // ---- the hashes, one lane each
    if (tid < lv.L * lv.k) {
        const float4 *p4 = reinterpret_cast<const float4 *>(lv.proj + (long)tid * LSH3_PD);
        const float4 *q4 = reinterpret_cast<const float4 *>(qc);
        const float4 last = p4[D3 / 4];         // {p[164], b, 0, 0}
        float d = last.y;
#pragma unroll 8
        for (int i = 0; i < D3 / 4; ++i) {
            const float4 p = p4[i], a = q4[i];
            d = fmaf(p.x, a.x, d);
            d = fmaf(p.y, a.y, d);
            d = fmaf(p.z, a.z, d);
            d = fmaf(p.w, a.w, d);
        }
        d = fmaf(last.x, qc[D3 - 1], d);
        hk[tid] = lsh_mix((int)floorf(d / lv.w), tid % lv.k);
    }
    __syncthreads();
    // ---- per table: the bucket range, and the exclusive prefix of the candidate counts
    if (wv == 0) {
        int lo = 0, cnt = 0;
        if (lane < lv.L) {
            unsigned int key = 0;
            for (int i = 0; i < lv.k; ++i) key += hk[lane * lv.k + i];
            key &= (1u << lv.bits) - 1u;
            const int *st = lv.start + (long)lane * ((1L << lv.bits) + 1);
            long l = st[key], h = st[key + 1];
            if (l == h) {   // empty bucket: take the neighbouring entries of the sorted table
                l = l >= 2 ? l - 2 : 0;
                h = l + 4 < nrows ? l + 4 : nrows;
            }
            lo = (int)l;
            cnt = (int)(h - l > LSH_CAP ? LSH_CAP : h - l);
        }
        int inc = cnt;
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(inc, o);
            if (lane >= o) inc += v;
        }
        lo_s[lane] = lo;
        n_s[lane] = inc - cnt;                  // (lanes >= L: the total)
        if (lane == 63) n_s[LSH_MAXH] = inc;
    }
    __syncthreads();
    const int total = n_s[LSH_MAXH];
    const int npass = total > 32 ? (total + 31) / 32 : 1;
    // ---- the candidates, 32 rows per pass (and, with the first, the coherence rows)
    int tb = 0;
    auto cand = [&](int c) -> long {            // the row of candidate c (-1: none)
        if (c >= total) return -1;
        while (n_s[tb + 1] <= c) ++tb;
        const int lr = lv.rows[(long)tb * lv.npad + lo_s[tb] + (c - n_s[tb])];
        return lr < nrows ? (long)lr : -1;
    };
    double bd = INFINITY, bw = 0.0;
    long long bi = NONE;
    long r = cand(ro);
    for (int b = 0; b < npass; ++b) {
        const long rn = b + 1 < npass ? cand(32 * (b + 1) + ro) : -1;
        Acc8 ta{}, ca{};
        if (r >= 0) ta = acc8_row(f.db3 + r * D3P, j, qs, wsh);
        if (TAIL && b == 0 && tid < 15 * 8) {
            const long long ix = rix[ro];
            ca = acc8_row(f.db3 + (ix >= 0 ? ix : 0) * D3P, j, qs, wsh);
        }
        acc[tid] = ta;
        if (TAIL && b == 0 && tid < 15 * 8) cacc[tid] = ca;
        __syncthreads();
        if (j == 0 && r >= 0) {
            const double d = acc8_sum(acc + 8 * ro, false);
            if (d < bd || (d == bd && r < bi)) {
                bd = d;
                bi = r;
                const double sq = sqrt(acc8_sum(acc + 8 * ro, true));
                bw = sq * sq;
            }
        }
        if (TAIL && b == 0 && j == 0 && tid < 15 * 8) {
            if (rix[ro] >= 0) {
                sump[ro] = sqrt(acc8_sum(cacc + 8 * ro, false));
                const double sq = sqrt(acc8_sum(cacc + 8 * ro, true));
                sumw[ro] = sq * sq;
            } else {
                sump[ro] = INFINITY;
                sumw[ro] = 0.0;
            }
        }
        __syncthreads();   // acc is refilled by the next pass
        r = rn;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double od = __shfl_xor(bd, o), ow = __shfl_xor(bw, o);
        const long long oi = __shfl_xor(bi, o);
        if (od < bd || (od == bd && oi < bi)) { bd = od; bi = oi; bw = ow; }
    }
    if (lane == 0) { rd[wv] = bd; ri[wv] = bi; rw[wv] = bw; }
    __syncthreads();
    double wd = rd[0], ww = rw[0];
    long long wi = ri[0];
#pragma unroll
    for (int w = 1; w < 4; ++w)
        if (rd[w] < wd || (rd[w] == wd && ri[w] < wi)) { wd = rd[w]; wi = ri[w]; ww = rw[w]; }
    if (wi == NONE) {   // (workgroup-uniform) no valid candidate: row 0
        if (tid < 8) acc[tid] = acc8_row(f.db3, tid, qs, wsh);
        __syncthreads();
        wi = 0;
        wd = acc8_sum(acc, false);
        const double sq = sqrt(acc8_sum(acc, true));
        ww = sq * sq;
    }
    if constexpr (TAIL) {
        if (wv != 0) return;
        const long src = c3_decide(f, y, x, lane, wi, ww, sump, sumw, rix, rpos);
        if (lane < 3) f.Bp_lg[((long)y * f.W + x) * 3 + lane] = f.Ap_lg[src + lane];
    } else {
        if (tid == 0) {
            if (idx) idx[m] = wi;
            if (dist) dist[m] = wd;
        }
    }
