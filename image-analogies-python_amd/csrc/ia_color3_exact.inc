// ia_color3_exact.inc -- the body of the colour exact stage + tail (ia_color3.hip: k_exact3, one
// job, by-value arguments; k_exact3b, a batch, arguments from the job table).  Included inside
// a kernel template <bool FUSE> with f (Fin3), sc (Scr3) and nx (Nx3) in scope and C3X_M,
// C3X_YN, C3X_MN (the wave's M, y_lo_n, M_n) and C3X_BATCH (0 / 1) defined.  One text for both,
// so the single job's kernel compiles exactly as it did before the batch form existed.
// C3X_PUB (0 in those two; 1 in k_exact3p, the exact stage of a sharded level, with pub (C3Pub)
// in scope): the coherence rows, which may lie in another rank's shard, and the tail are left
// to k_peer_finish3; wave 0 instead stores this shard's (distance, global row, weighted
// distance) and publishes it to every rank's box.  Nothing here waits for another rank.
    __shared__ double qs[D3P], wsh[D3P];
    __shared__ double ownv[3], nbv[3], qred[4], qds[D3];
    __shared__ int tks, anydep;
    __shared__ Acc8 acc[32 * 8];                // a tile's rows (32 x 8 parts)
#if !C3X_PUB
    __shared__ Acc8 cacc[15 * 8];               // the coherence rows
    __shared__ double sump[15], sumw[15];
    __shared__ long long rix[15];
    __shared__ int rpos[15][3];
#endif
    __shared__ double rd[4], rw[4];
    __shared__ long long ri[4];
    __shared__ float fmn[4];
    __shared__ int clist[C3_CAND], ccount;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int m = blockIdx.x;
    if constexpr (FUSE) {
        if (tid == 0) {
            tks = (int)atomicAdd(&nx.tickets[f.t & 1], 1u);
            anydep = 0;
        }
        __syncthreads();
        m = tks;
        if (m == 0 && tid == 0) __hip_atomic_store(&nx.tickets[(f.t + 1) & 1], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const int ro = tid >> 3, j = tid & 7;
    const int y = f.y_lo + m, x = f.t - 3 * y;
    const int W = f.W;
    const bool cur = !FUSE || m < C3X_M;
    const bool nxt = FUSE && y >= C3X_YN && y < C3X_YN + C3X_MN;
    // FUSE: feature tid of the next query (y, x + 1): loaded now unless it is a wave-t sample
    double nv = 0.0;
    int dep = 0, dch = 0;
    if (FUSE && nxt && tid < D3) {
        const int X = x + 1;
        if (tid < D3_FULL) {
            nv = feat3(nx.Bsm, nx.Blg, y, X, tid);
        } else if (tid < D3_FULL + 27) {
            nv = feat3(nx.Bpsm, nx.Bplg, y, X, tid - D3_FULL);
        } else {
            const int t2 = (tid - D3_FULL - 27) / 3;
            dch = (tid - D3_FULL - 27) - 3 * t2;
            const int rr = symi2(y + t2 / 5 - 2, nx.H), cc = symi2(X + t2 % 5 - 2, W);
            dep = (rr == y && cc == x) ? 1 : (rr == y - 1 && cc == x + 3) ? 2 : 0;
            if (dep == 0) nv = nx.Bplg.p[((long)rr * W + cc) * 3 + dch];
        }
        if (dep == 2) anydep = 1;
    }
    if (cur) {
    // ---- one round trip: query, weights, coherence s / im, tile minima
    if (tid < D3P) {
        qs[tid] = f.q3[(long)m * D3P + tid];
        wsh[tid] = tid < D3 ? f.weights[tid] : 0.0;
    }
#if !C3X_PUB
    if (tid < 15) c3_window(tid, y, x, f, rix, rpos);
#endif
    const int stride = c3_stride(sc.ntiles);
    const float4 *sm4 = reinterpret_cast<const float4 *>(sc.smin + (long)m * stride);
    const int n4 = stride / 4;
    float4 v[C3_REG];
#pragma unroll
    for (int q = 0; q < C3_REG; ++q) {
        const int i = tid + 256 * q;
        v[q] = sm4[i < n4 ? i : 0];
    }
    auto masked = [&](float4 xx, int i) {   // +inf past the tiles (and the float4 pad)
        const int b = 4 * i;
        xx.x = b + 0 < sc.ntiles && i < n4 ? xx.x : INFINITY;
        xx.y = b + 1 < sc.ntiles && i < n4 ? xx.y : INFINITY;
        xx.z = b + 2 < sc.ntiles && i < n4 ? xx.z : INFINITY;
        xx.w = b + 3 < sc.ntiles && i < n4 ? xx.w : INFINITY;
        return xx;
    };
    float mn = INFINITY;
#pragma unroll
    for (int q = 0; q < C3_REG; ++q) {
        v[q] = masked(v[q], tid + 256 * q);
        mn = fminf(mn, fminf(fminf(v[q].x, v[q].y), fminf(v[q].z, v[q].w)));
    }
    for (int i = tid + 256 * C3_REG; i < n4; i += 256) {
        const float4 xx = masked(sm4[i], i);
        mn = fminf(mn, fminf(fminf(xx.x, xx.y), fminf(xx.z, xx.w)));
    }
    for (int o = 32; o > 0; o >>= 1) mn = fminf(mn, __shfl_xor(mn, o));
    if (lane == 0) fmn[wv] = mn;
    if (tid == 0) ccount = 0;
    __syncthreads();
    // ---- the candidate tiles
    mn = fminf(fminf(fmn[0], fmn[1]), fminf(fmn[2], fmn[3]));
    bool full;
    const float amax = __uint_as_float(sc.meta->amax_bits);
    const double Tseg = sc.nsk ? c3_tseg(mn, amax, sc.qn[m], full, __uint_as_float(sc.rmeta->askip_bits), sc.nsk[m])
                               : c3_tseg(mn, amax, sc.qn[m], full);
    if (!full) {
        auto pick = [&](float4 xx, int i) {
            const float e4[4] = {xx.x, xx.y, xx.z, xx.w};
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if ((double)e4[e] <= Tseg) {
                    const int c = atomicAdd(&ccount, 1);
                    if (c < C3_CAND) clist[c] = 4 * i + e;
                }
        };
#pragma unroll
        for (int q = 0; q < C3_REG; ++q) pick(v[q], tid + 256 * q);
        for (int i = tid + 256 * C3_REG; i < n4; i += 256) pick(masked(sm4[i], i), i);
    }
    __syncthreads();
    const int nc = ccount;
    full = full || nc > C3_CAND;
    const int ntl = full ? sc.ntiles : nc;
    if (tid == 0 && sc.stats) {
        atomicAdd(&sc.stats[0], (unsigned long long)ntl);
        if (full) atomicAdd(&sc.stats[1], 1ull);
    }
    // ---- every row of the candidate tiles (and, with the first, the coherence rows)
    double bd = INFINITY, bw = 0.0;
    long long bi = 0x7fffffffffffffffLL;
    const int nit = ntl > 0 ? ntl : 1;
    for (int b = 0; b < nit; ++b) {
        Acc8 ta{}, ca{};
        const long r0 = ntl > 0 ? (long)(full ? b : clist[b]) * 32 : 0;
        const long r = r0 + ro < sc.nrows ? r0 + ro : sc.nrows - 1;   // (rows past nrows: not taken)
        if (ntl > 0) ta = acc8_row(f.db3 + r * D3P, j, qs, wsh);
#if !C3X_PUB
        if (b == 0 && tid < 15 * 8) {
            const long long ix = rix[ro];
            ca = acc8_row(f.db3 + (ix >= 0 ? ix : 0) * D3P, j, qs, wsh);
        }
#endif
        acc[tid] = ta;
#if !C3X_PUB
        if (b == 0 && tid < 15 * 8) cacc[tid] = ca;
#else
        (void)ca;
#endif
        __syncthreads();
        if (j == 0 && ntl > 0 && r0 + ro < sc.nrows) {
            const double d = acc8_sum(acc + 8 * ro, false);
            if (d < bd || (d == bd && r0 + ro < bi)) {
                bd = d;
                bi = r0 + ro;
                const double sq = sqrt(acc8_sum(acc + 8 * ro, true));
                bw = sq * sq;
            }
        }
#if !C3X_PUB
        if (b == 0 && j == 0 && tid < 15 * 8) {
            if (rix[ro] >= 0) {
                sump[ro] = sqrt(acc8_sum(cacc + 8 * ro, false));
                const double sq = sqrt(acc8_sum(cacc + 8 * ro, true));
                sumw[ro] = sq * sq;
            } else {
                sump[ro] = INFINITY;
                sumw[ro] = 0.0;
            }
        }
#endif
        __syncthreads();   // acc is refilled by the next tile
    }
    for (int o = 32; o > 0; o >>= 1) {
        const double od = __shfl_xor(bd, o), ow = __shfl_xor(bw, o);
        const long long oi = __shfl_xor(bi, o);
        if (od < bd || (od == bd && oi < bi)) { bd = od; bi = oi; bw = ow; }
    }
    if (lane == 0) { rd[wv] = bd; ri[wv] = bi; rw[wv] = bw; }
    __syncthreads();
    if (wv == 0) {
    double wd = rd[0], ww = rw[0];
    long long wi = ri[0];
#pragma unroll
    for (int w = 1; w < 4; ++w)
        if (rd[w] < wd || (rd[w] == wd && ri[w] < wi)) { wd = rd[w]; wi = ri[w]; ww = rw[w]; }
#if C3X_PUB
    // this shard's record: kept for this rank's own finish (and the RCCL gather), and sent
    const XRec rec{wd, pub.row0 + wi, ww, 0.0};
    if (lane == 0) pub.rec[m] = ShardRec{rec.d, rec.i, rec.wd, 0.0};
    if (pub.px.nranks > 0) peer_publish_rec(pub.px, m, rec, lane);
#else
    const long src = c3_decide(f, y, x, lane, wi, ww, sump, sumw, rix, rpos);
    if (lane < 3) {
        const double val = f.Ap_lg[src + lane];
        f.Bp_lg[((long)y * W + x) * 3 + lane] = val;
        if constexpr (FUSE) {
            // the decision for the lower neighbour's next query, and this pixel's own
            ownv[lane] = val;
            const unsigned long long bits = (unsigned long long)__double_as_longlong(val);
            unsigned long long *d = nx.dbox + 8 * (long)y + 2 * lane;
            __hip_atomic_store(d, c3_gran(f.t + 1, (unsigned)bits), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(d + 1, c3_gran(f.t + 1, (unsigned)(bits >> 32)), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        }
    }
#endif
    }   // wave 0
    }   // cur
    if constexpr (FUSE) {
        __syncthreads();   // ownv, anydep
        if (nxt) {
            if (anydep && tid == 0) {   // the upper neighbour (ticket m - 1) decided (y - 1, x + 3)
                const unsigned long long *d = nx.dbox + 8 * (long)(y - 1);
                const unsigned tag = (unsigned)(f.t + 1);
                const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
                for (;;) {
                    bool ok = true;
                    unsigned long long g[6];
#pragma unroll
                    for (int c = 0; c < 6; ++c) {
                        g[c] = __hip_atomic_load(d + c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        ok = ok && (unsigned)(g[c] >> 32) == tag;
                    }
                    if (ok) {
#pragma unroll
                        for (int c = 0; c < 3; ++c)
                            nbv[c] = __longlong_as_double(
                                (long long)(((g[2 * c + 1] & 0xffffffffULL) << 32) | (g[2 * c] & 0xffffffffULL)));
                        break;
                    }
                    if (__builtin_amdgcn_s_memrealtime() - t0 > C3_WAIT_TICKS) {
                        atomicOr(nx.err, 1u);
                        nbv[0] = nbv[1] = nbv[2] = 0.0;
                        break;
                    }
                    __builtin_amdgcn_s_sleep(1);
                }
            }
            __syncthreads();
            const double v = dep == 1 ? ownv[dch] : dep == 2 ? nbv[dch] : nv;
            const int mq = y - C3X_YN;
            if (tid < D3P) nx.q3n[(long)mq * D3P + tid] = tid < D3 ? v : 0.0;
            r3_query(mq, C3X_MN, tid, v, nx.meta, nx.rot, nx.qnn, nx.nskn, nx.q16n, qds, qred);
#if C3X_BATCH
            if (mq == 0)   // the last query tile's padding columns (no barrier on this path)
                for (int c = C3X_MN; c < ((C3X_MN + 31) & ~31); ++c)
                    r3_query(c, C3X_MN, tid, 0.0, nx.meta, nx.rot, nx.qnn, nx.nskn, nx.q16n, qds, qred);
#endif
        }
    }
