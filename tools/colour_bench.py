"""Throughput of 3-channel matching (the reference's default convert=False on colour images:
config.py:29-42 num_ch = 3, 165-dim rows, algorithms.py:11-47) on one GPU, next to the
luminance path on the same images (their Y channel): B' pixels per second of whole
syntheses (device pyramids, B' reset, every level), inputs resident in HBM.

usage: python tools/colour_bench.py [H W] [steps] [jobs]   (default 180 117 (c1 size), 3 steps, 1 job)
       jobs = K > 1: a batch of K colour jobs of that size with distinct seeds in one
       synthesize_batch_dev call (ia_synth_levels3_batch): ms per step and per job, every
       step's time, the candidate tiles per query, under one rotation per batch and one per
       job (IA_ROT3_BATCH_SHARED both ways), and the peak device memory allocated
       python tools/colour_bench.py H W steps K --shared [G]
       the same batch with G distinct (A, A') pairs (default 1; job q takes pair q mod G) and K
       distinct B images and B' seeds: the jobs of a pair are given the same pyramid tensors, so
       they form one DB group (one database and one rotated database per level, screened
       together by k_screen3rs; IA_C3_SHARED_SCREEN=0: by k_screen3rb as an unshared batch)
       python tools/colour_bench.py H W steps --shards G [G ...]
       the per-rank cost of the sharded colour synthesis in the manner of tools/shard_sim.py: rank
       0 of G row shards (every level sharded: IA_SHARD_MIN_ROWS defaults to 0 here) over a 1-rank
       exchange (IA_EXCHANGE: peer [default] or rccl), so each wave runs the sharded path (query
       rows, the screen of the shard's tiles, k_exact3p, k_peer_finish3) without another rank's
       latency.  B' is the shard's own: timing only.  Per G: ms per level (levels one at a time,
       the median of `steps`) and ms per pipelined step
       python tools/colour_bench.py H W steps --lsh T,H,W [T,H,W ...] [--b BH BW] [--levels N]
       the colour LSH matcher (c.matcher = 'lsh': tables T, hashes H, width W each) against the
       colour exact matcher on the same images (A, A' of H x W; B of BH x BW, default H x W;
       N: the cap on pyramid halvings, with which a larger A keeps its finest level), in
       one call: per setting both warmed up, then `steps` pairs of whole syntheses, exact and LSH
       alternating (medians; px/s of each and exact / LSH time), and the quality of the LSH
       run's finest level on 4,096 sampled interior pixels: the share of LSH picks equal to the
       exact 1-NN of the same query, and the mean distance |a - q| of the LSH picks over that of
       the exact ones
       COLOUR_PIPE=0: the colour levels one at a time (default: pipelined, ia_synth_levels3)
       COLOUR_ONLY=1: the 3-channel run alone (kernel traces of it)
Also reports the colour exact stage's candidate tiles per query (ia_diag_color16_stats) and a
B' checksum (equal with and without the pipeline).
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import torch  # noqa: E402

ip, cfg, ia = bench.ip, bench.cfg, bench.ia


def batch_main(H, W, steps, K, pairs=None):
    """K colour jobs of H x W with distinct seeds as one batch; pairs = G: G distinct (A, A')
    among them, each pair's pyramids built once per step and given to all its jobs."""
    import ctypes
    import _ia
    from scipy.ndimage import gaussian_filter
    dev = 'cuda:0'
    w = torch.as_tensor(cfg.compute_weights(3, 5, 12, 3)).to(dev)
    nB = ip.num_layers(H, W, cfg.n_sm, None)
    L = nB + 1
    shapes = [(H, W, 3)]
    for _ in range(nB):
        shapes.append(((shapes[-1][0] + 1) // 2, (shapes[-1][1] + 1) // 2, 3))
    shapes.reverse()
    pixels = sum(s[0] * s[1] for s in shapes[1:L])
    srcs = []
    for q in range(K):
        A = np.dstack([bench.smooth_noise(7 + 17 * c + 101 * q, (H, W)) for c in range(3)])
        Ap = np.dstack([gaussian_filter(A[..., c], 1.5) for c in range(3)])
        B = np.dstack([bench.smooth_noise(8 + 17 * c + 101 * q, (H, W)) for c in range(3)])
        init = [torch.as_tensor(x).to(dev) for x in ip.initialize_Bp([np.empty(s) for s in shapes], True, 9 + q)]
        srcs.append(tuple(torch.as_tensor(x).to(dev) for x in (A, Ap, B)) + (init, [x.clone() for x in init]))
    out = {'size': [H, W], 'jobs': K, 'steps': steps, 'pixels_per_job': pixels, 'a_pairs': pairs or K}
    st = (ctypes.c_ulonglong * 2)()
    for name, shared in (('rotation_per_batch', True), ('rotation_per_job', False)):
        def step():
            jobs = []
            for q, (a, ap, b, init, Bp) in enumerate(srcs):
                for d, s in zip(Bp, init):
                    d.copy_(s)
                if pairs and q >= pairs:
                    A_pyr, Ap_list = jobs[q % pairs][:2]
                else:
                    A_pyr, Ap_list = ip.gaussian_pyramid_dev(a, cfg.n_sm), [ip.gaussian_pyramid_dev(ap, cfg.n_sm)]
                jobs.append((A_pyr, Ap_list, ip.gaussian_pyramid_dev(b, cfg.n_sm), Bp))
            ia.synthesize3_batch_dev(jobs, L, [0.5] * K, w, rot_shared=shared)

        _ia.check(_ia.lib().ia_diag_color16_stats(st), 'stats')   # (reads and clears)
        step()
        torch.cuda.synchronize()
        _ia.check(_ia.lib().ia_diag_color16_stats(st), 'stats')
        cand = (st[0] / (pixels * K), int(st[1]))
        step()                                                   # (second warm-up)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        times = []
        for _ in range(steps):
            t0 = time.perf_counter()
            step()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) * 1e3)
        med = float(np.median(times))
        out[name] = {'ms_per_step': med, 'ms_per_job': med / K, 'ms_steps': [round(t, 3) for t in times],
                     'px_per_s': pixels * K / (med * 1e-3), 'candidate_tiles_per_query': cand[0],
                     'full_scans': cand[1], 'peak_mb': round(torch.cuda.max_memory_allocated() / 2 ** 20, 1),
                     'bp_checksum': float(sum(float(x.sum()) for s in srcs for x in s[4][1:L]))}
    print(json.dumps(out))


def shards_main(H, W, steps, gs):
    """Rank 0 of G shards of every colour level over a 1-rank exchange, for each G."""
    import _ia
    from scipy.ndimage import gaussian_filter
    os.environ.setdefault('IA_SHARD_MIN_ROWS', '0')
    dev = 'cuda:0'
    A = np.dstack([bench.smooth_noise(7 + 17 * c, (H, W)) for c in range(3)])
    Ap = np.dstack([gaussian_filter(A[..., c], 1.5) for c in range(3)])
    B = np.dstack([bench.smooth_noise(8 + 17 * c, (H, W)) for c in range(3)])
    a, ap, b = (torch.as_tensor(x).to(dev) for x in (A, Ap, B))
    w = torch.as_tensor(cfg.compute_weights(3, 5, 12, 3)).to(dev)
    nB = ip.num_layers(H, W, cfg.n_sm, None)
    L = nB + 1
    shapes = [(H, W, 3)]
    for _ in range(nB):
        shapes.append(((shapes[-1][0] + 1) // 2, (shapes[-1][1] + 1) // 2, 3))
    shapes.reverse()
    init = [torch.as_tensor(x).to(dev) for x in ip.initialize_Bp([np.empty(s) for s in shapes], True, 9)]
    Bp = [x.clone() for x in init]
    A_pyr, Ap_pyr, B_pyr = (ip.gaussian_pyramid_dev(x, cfg.n_sm) for x in (a, ap, b))
    comms = [_ia.exchange(0, 1) for _ in range(1, L)]
    out = {'size': [H, W], 'steps': steps, 'exchange': _ia.exchange_kind(),
           'rows': {l: ia.level_rows([Ap_pyr], l) for l in range(1, L)}, 'shards': {}}

    def timed(**kw):
        for d, s in zip(Bp, init):
            d.copy_(s)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ia.synthesize_dev(A_pyr, [Ap_pyr], B_pyr, Bp, L, 0.5, w, rank=0, **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    try:
        for G in gs:
            timed(comm=comms, nranks=G, pipeline=True)        # warm-up
            levels = {l: float(np.median([timed(comm=comms[0], nranks=G, levels={l}, pipeline=False)
                                          for _ in range(steps)])) for l in range(1, L)}
            pipe = [timed(comm=comms, nranks=G, pipeline=True) for _ in range(steps)]
            out['shards'][G] = {'ms_per_level': {l: round(t, 3) for l, t in levels.items()},
                                'ms_levels_sum': round(sum(levels.values()), 3),
                                'ms_per_step_pipelined': round(float(np.median(pipe)), 3),
                                'ms_steps': [round(t, 3) for t in pipe]}
        for cm in comms:
            _ia.exchange_status(cm)
    finally:
        torch.cuda.synchronize()
        for cm in comms:
            _ia.lib().ia_comm_destroy(cm)
    print(json.dumps(out))


def lsh_main(H, W, steps, settings, BH, BW, levels=None, nq=4096):
    """Colour LSH against the colour exact matcher on the same images (A, A' of H x W, B of
    BH x BW), per LSH setting (tables, hashes, width): after a warm-up of both, `steps` pairs of
    whole syntheses, exact then LSH, alternating; the medians.  levels: the cap on pyramid
    halvings (config.levels; with it a larger A keeps its finest level against a smaller B)."""
    import algorithms
    from scipy.ndimage import gaussian_filter
    dev = 'cuda:0'
    A = np.dstack([bench.smooth_noise(7 + 17 * c, (H, W)) for c in range(3)])
    Ap = np.dstack([gaussian_filter(A[..., c], 1.5) for c in range(3)])
    B = np.dstack([bench.smooth_noise(8 + 17 * c, (BH, BW)) for c in range(3)])
    a, ap, b = (torch.as_tensor(x).to(dev) for x in (A, Ap, B))
    w = torch.as_tensor(cfg.compute_weights(3, 5, 12, 3)).to(dev)
    A_pyr, Ap_pyr, B_pyr = (ip.gaussian_pyramid_dev(x, cfg.n_sm, levels) for x in (a, ap, b))
    L = min(len(A_pyr), len(B_pyr))
    init = [torch.as_tensor(x).to(dev)
            for x in ip.initialize_Bp([np.empty(tuple(p.shape)) for p in B_pyr], True, 9)]
    Bp = [x.clone() for x in init]
    pixels = sum(int(p.shape[0] * p.shape[1]) for p in B_pyr[1:L])
    lv = L - 1
    out = {'A_size': [H, W], 'B_size': [BH, BW], 'level_cap': levels, 'levels': L - 1, 'pixels': pixels,
           'finest_rows': int(Ap_pyr[lv].shape[0] * Ap_pyr[lv].shape[1]), 'steps': steps, 'lsh': []}

    def step(lsh):
        pa, pap, pb = (ip.gaussian_pyramid_dev(x, cfg.n_sm, levels) for x in (a, ap, b))
        for d, s in zip(Bp, init):
            d.copy_(s)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ia.synthesize_dev(pa, [pap], pb, Bp, L, 0.5, w, lsh=lsh)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for T, K, width in settings:
        lsh = dict(tables=T, hashes=K, width=width, seed=0)
        step(None)
        step(lsh)
        te, tl = [], []
        for _ in range(steps):
            te.append(step(None))
            tl.append(step(lsh))
        # quality on the finest level of the LSH run just made: nq interior pixels (their causal
        # B' windows hold final values, so the rows below are the synthesis's own queries), the
        # LSH pick of the same tables against the exact 1-NN
        index = algorithms.LevelIndex3(A_pyr[lv - 1], A_pyr[lv], Ap_pyr[lv - 1][None], Ap_pyr[lv][None])
        index.build_lsh(**lsh)
        Hq, Wq = B_pyr[lv].shape[:2]
        Q = torch.cat([algorithms.level_features3_dev(B_pyr[lv - 1], B_pyr[lv], True),
                       algorithms.level_features3_dev(Bp[lv - 1], Bp[lv], False)], 1)
        rs = np.random.RandomState(1)
        ys, xs = rs.randint(2, Hq, nq), rs.randint(2, Wq, nq)
        Qs = Q[torch.as_tensor(ys * Wq + xs).to(dev)]
        li, ld = index.match(Qs)
        ei, ed = index.match(Qs, exact=True)
        me, ml = float(np.median(te)), float(np.median(tl))
        out['lsh'].append({'tables': T, 'hashes': K, 'width': width,
                           'exact_ms': round(me, 3), 'lsh_ms': round(ml, 3),
                           'exact_px_per_s': pixels / (me * 1e-3), 'lsh_px_per_s': pixels / (ml * 1e-3),
                           'speedup': me / ml,
                           'exact_ms_steps': [round(t, 3) for t in te], 'lsh_ms_steps': [round(t, 3) for t in tl],
                           'exact_pick_share': float((li == ei).double().mean()),
                           'dist_ratio': float(ld.sqrt().mean() / ed.sqrt().mean()),
                           'sampled_queries': nq})
        del index, Q, Qs
    print(json.dumps(out))


def main():
    H, W = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (180, 117)
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    if '--lsh' in sys.argv:
        rest = sys.argv[sys.argv.index('--lsh') + 1:]
        BH, BW, levels = H, W, None
        if '--levels' in rest:
            levels = int(rest[rest.index('--levels') + 1])
            del rest[rest.index('--levels'):rest.index('--levels') + 2]
        if '--b' in rest:
            BH, BW = int(rest[rest.index('--b') + 1]), int(rest[rest.index('--b') + 2])
            rest = rest[:rest.index('--b')]
        settings = [(int(t), int(k), float(wd)) for t, k, wd in (s.split(',') for s in rest)]
        return lsh_main(H, W, steps, settings or [(16, 4, 1.0)], BH, BW, levels)
    if '--shards' in sys.argv:
        return shards_main(H, W, steps, [int(g) for g in sys.argv[sys.argv.index('--shards') + 1:]] or [1, 2, 4, 8])
    if len(sys.argv) > 4 and int(sys.argv[4]) > 1:
        pairs = None
        if '--shared' in sys.argv:
            rest = sys.argv[sys.argv.index('--shared') + 1:]
            pairs = max(1, min(int(rest[0]), int(sys.argv[4]))) if rest else 1
        return batch_main(H, W, steps, int(sys.argv[4]), pairs)
    from scipy.ndimage import gaussian_filter
    dev = 'cuda:0'
    A = np.dstack([bench.smooth_noise(7 + 17 * c, (H, W)) for c in range(3)])
    Ap = np.dstack([gaussian_filter(A[..., c], 1.5) for c in range(3)])
    B = np.dstack([bench.smooth_noise(8 + 17 * c, (H, W)) for c in range(3)])
    w = torch.as_tensor(cfg.compute_weights(3, 5, 12, 3)).to(dev)
    w1 = torch.as_tensor(cfg.compute_weights(3, 5, 12, 1)).to(dev)
    import ctypes
    import _ia
    pipe = os.environ.get('COLOUR_PIPE', '1') != '0'
    out = {'size': [H, W], 'pipeline': pipe}
    runs = {'rgb': (A, Ap, B, w), 'luminance': (A[..., 0], Ap[..., 0], B[..., 0], w1)}
    if os.environ.get('COLOUR_ONLY', '0') != '0':
        del runs['luminance']
    for name, (a, ap, b, ww) in runs.items():
        a, ap, b = (torch.as_tensor(x).to(dev) for x in (a, ap, b))
        nB = ip.num_layers(H, W, cfg.n_sm, None)
        L = nB + 1
        shapes = [b.shape]
        for _ in range(nB):
            shapes.append(tuple([(shapes[-1][0] + 1) // 2, (shapes[-1][1] + 1) // 2] + list(b.shape[2:])))
        shapes.reverse()
        init = [torch.as_tensor(x).to(dev)
                for x in ip.initialize_Bp([np.empty(s) for s in shapes], True, 9)]
        Bp = [x.clone() for x in init]
        pixels = sum(s[0] * s[1] for s in shapes[1:L])

        def step():
            A_pyr = ip.gaussian_pyramid_dev(a, cfg.n_sm)
            Ap_pyr = ip.gaussian_pyramid_dev(ap, cfg.n_sm)
            B_pyr = ip.gaussian_pyramid_dev(b, cfg.n_sm)
            for d, s in zip(Bp, init):
                d.copy_(s)
            ia.synthesize_dev(A_pyr, [Ap_pyr], B_pyr, Bp, L, 0.5, ww, pipeline=pipe)

        st = (ctypes.c_ulonglong * 2)()
        _ia.check(_ia.lib().ia_diag_color16_stats(st), 'stats')   # (reads and clears)
        step()
        torch.cuda.synchronize()
        _ia.check(_ia.lib().ia_diag_color16_stats(st), 'stats')
        cand = (st[0] / pixels, int(st[1]))
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / steps
        out[name] = {'ms_per_step': dt * 1e3, 'px_per_s': pixels / dt, 'pixels': pixels,
                     'bp_checksum': float(sum(float(x.sum()) for x in Bp[1:L]))}
        if name == 'rgb':
            out[name]['candidate_tiles_per_query'], out[name]['full_scans'] = cand
    if 'luminance' in out:
        out['rgb_vs_luminance_slowdown'] = out['luminance']['px_per_s'] / out['rgb']['px_per_s']
    print(json.dumps(out))


if __name__ == '__main__':
    main()
