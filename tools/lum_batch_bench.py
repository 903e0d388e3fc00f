"""Throughput of a luminance batch (convert=True: 55-dim rows) whose jobs share (A, A') pairs,
on one GPU: whole syntheses from device pyramids (B' reset, every level), inputs resident in HBM.

usage: python tools/lum_batch_bench.py H W steps K [--shared G] [--levels N]
       K jobs of H x W with G distinct (A, A') pairs (default G = K: no sharing); job q takes
       pair q mod G, and the jobs of a pair are given the SAME pyramid tensors, so they form one
       DB group (image_analogies.db_groups): one level index per group and level, and on levels
       with a rotated database one k_screen16rs launch per wave (IA_SHARED_SCREEN=0: the K-job
       k_screen16r over the shared database).  Every job has its own B, B' seed and kappa.
       N: the cap on pyramid halvings (config.levels).
Prints one JSON line: the medians of ms per step and per job, every step's time, the peak device
memory allocated during the timed steps and a B' checksum per job.  Only calls that older
revisions have too, so the same file measures a revision without DB groups (where the aliased
jobs build K databases) when it is copied into that tree.
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


def main():
    args = sys.argv[1:]
    opt = {}
    for name in ('--shared', '--levels'):
        if name in args:
            i = args.index(name)
            opt[name] = int(args[i + 1])
            del args[i:i + 2]
    H, W, steps, K = (int(x) for x in args[:4])
    G = max(1, min(opt.get('--shared', K), K))
    levels = opt.get('--levels')
    from scipy.ndimage import gaussian_filter
    dev = 'cuda:0'
    w = torch.as_tensor(cfg.compute_weights(3, 5, 12, 1)).to(dev)
    up = lambda x: torch.as_tensor(x).to(dev)  # noqa: E731
    pairs = []
    for g in range(G):
        A = bench.smooth_noise(7 + 101 * g, (H, W))
        pairs.append((up(A), up(gaussian_filter(A, 1.5))))
    Bs = [up(bench.smooth_noise(8 + 101 * q, (H, W))) for q in range(K)]
    B0 = ip.gaussian_pyramid_dev(Bs[0], cfg.n_sm, levels)
    L = min(len(ip.gaussian_pyramid_dev(pairs[0][0], cfg.n_sm, levels)), len(B0))
    inits = [[up(x) for x in ip.initialize_Bp([np.empty(tuple(p.shape)) for p in B0], True, 9 + q)]
             for q in range(K)]
    Bps = [[x.clone() for x in init] for init in inits]
    ks = [0.5 + 0.75 * q for q in range(K)]
    pixels = sum(int(p.shape[0] * p.shape[1]) for p in B0[1:L])

    def step():
        sides = [(ip.gaussian_pyramid_dev(a, cfg.n_sm, levels), [ip.gaussian_pyramid_dev(ap, cfg.n_sm, levels)])
                 for a, ap in pairs]
        jobs = []
        for q in range(K):
            for d, s in zip(Bps[q], inits[q]):
                d.copy_(s)
            jobs.append(sides[q % G] + (ip.gaussian_pyramid_dev(Bs[q], cfg.n_sm, levels), Bps[q]))
        ia.synthesize_batch_dev(jobs, L, ks, w)

    for _ in range(2):      # warm-up
        step()
        torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    times = []
    for _ in range(steps):
        t0 = time.perf_counter()
        step()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    med = float(np.median(times))
    print(json.dumps({
        'size': [H, W], 'jobs': K, 'a_pairs': G, 'levels': L - 1, 'steps': steps, 'pixels_per_job': pixels,
        'shared_screen_env': os.environ.get('IA_SHARED_SCREEN'), 'chunks_env': os.environ.get('IA_BATCH_CHUNKS'),
        'ms_per_step': round(med, 3), 'ms_per_job': round(med / K, 3), 'ms_steps': [round(t, 3) for t in times],
        'px_per_s': pixels * K / (med * 1e-3),
        'peak_mb': round(torch.cuda.max_memory_allocated() / 2 ** 20, 1),
        'bp_checksums': [float(sum(float(x.sum()) for x in Bp[1:L])) for Bp in Bps]}))


if __name__ == '__main__':
    main()
