"""Throughput of K LSH jobs (c.matcher = 'lsh') of identical shapes on one GPU, batched or one by
one: whole syntheses from device pyramids (B' reset, every level), inputs resident in HBM.

usage: python tools/lsh_batch_bench.py H W steps K --lsh L,k,w [L,k,w ...] [--colour]
                                       [--shared 0|1|0,1] [--mode batch|single|exact] [--levels N]
       K jobs of H x W, each with its own B, B' seed and kappa; --shared 1: one (A, A') pair for
       all of them (the SAME pyramid tensors: one DB group), 0: a pair per job.  --colour: 3-channel
       rows (convert=False), else luminance.  Every step rebuilds the pyramids (once per pair),
       the level indexes and the LSH tables.
       --mode batch  [default] one synthesize_batch_dev(..., lsh=...) call per step
              single K synthesize_dev(..., lsh=...) calls per step: all that a revision without
                     LSH batches can do (this mode and `exact` make only calls such a revision
                     has too, so the same file measures it when copied into that tree)
              exact  one exact synthesize_batch_dev call per step (the --lsh settings are ignored)
Prints one JSON line per (setting, shared): the median of ms per step and per job, every step's
time, the peak device memory allocated during the timed steps and a B' checksum per job.
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


def image(seed, H, W, colour):
    if not colour:
        return bench.smooth_noise(seed, (H, W))
    return np.dstack([bench.smooth_noise(seed + 17 * c, (H, W)) for c in range(3)])


def blur(img, sigma=1.5):
    from scipy.ndimage import gaussian_filter
    if img.ndim == 2:
        return gaussian_filter(img, sigma)
    return np.dstack([gaussian_filter(img[..., c], sigma) for c in range(3)])


def run(H, W, steps, K, colour, shared, mode, lsh, levels):
    dev = 'cuda:0'
    up = lambda x: torch.as_tensor(x).to(dev)  # noqa: E731
    w = up(cfg.compute_weights(3, 5, 12, 3 if colour else 1))
    G = 1 if shared else K
    pairs = []
    for g in range(G):
        A = image(7 + 101 * g, H, W, colour)
        pairs.append((up(A), up(blur(A))))
    Bs = [up(image(8 + 101 * q, H, W, colour)) for q in range(K)]
    pyr = lambda x: ip.gaussian_pyramid_dev(x, cfg.n_sm, levels)  # noqa: E731
    B0 = pyr(Bs[0])
    L = min(len(pyr(pairs[0][0])), len(B0))
    inits = [[up(x) for x in ip.initialize_Bp([np.empty(tuple(p.shape)) for p in B0], True, 9 + q)]
             for q in range(K)]
    Bps = [[x.clone() for x in init] for init in inits]
    ks = [0.5 + 0.75 * q for q in range(K)]
    pixels = sum(int(p.shape[0] * p.shape[1]) for p in B0[1:L])

    def step():
        sides = [(pyr(a), [pyr(ap)]) for a, ap in pairs]
        jobs = []
        for q in range(K):
            for d, s in zip(Bps[q], inits[q]):
                d.copy_(s)
            jobs.append(sides[q % G] + (pyr(Bs[q]), Bps[q]))
        if mode == 'batch':
            ia.synthesize_batch_dev(jobs, L, ks, w, lsh=lsh)
        elif mode == 'exact':
            ia.synthesize_batch_dev(jobs, L, ks, w)
        else:
            for job, k in zip(jobs, ks):
                ia.synthesize_dev(*job, L, k, w, lsh=lsh)

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
        'size': [H, W], 'jobs': K, 'colour': colour, 'shared': int(shared), 'mode': mode,
        'lsh': None if mode == 'exact' else [lsh['tables'], lsh['hashes'], lsh['width']],
        'levels': L - 1, 'steps': steps, 'pixels_per_job': pixels,
        'ms_per_step': round(med, 3), 'ms_per_job': round(med / K, 3), 'ms_steps': [round(t, 3) for t in times],
        'peak_mb': round(torch.cuda.max_memory_allocated() / 2 ** 20, 1),
        'bp_checksums': [float(sum(float(x.sum()) for x in Bp[1:L])) for Bp in Bps]}), flush=True)


def main():
    args = sys.argv[1:]
    colour = '--colour' in args
    if colour:
        args.remove('--colour')
    opt = {'--shared': '0', '--mode': 'batch', '--levels': None}
    for name in ('--shared', '--mode', '--levels'):
        if name in args:
            i = args.index(name)
            opt[name] = args[i + 1]
            del args[i:i + 2]
    settings = []
    if '--lsh' in args:
        i = args.index('--lsh')
        j = i + 1
        while j < len(args) and not args[j].startswith('--'):
            L, k, w = args[j].split(',')
            settings.append(dict(tables=int(L), hashes=int(k), width=float(w), seed=0))
            j += 1
        del args[i:j]
    mode = opt['--mode']
    if mode not in ('batch', 'single', 'exact') or (mode != 'exact' and not settings):
        sys.exit(__doc__)
    H, W, steps, K = (int(x) for x in args[:4])
    levels = int(opt['--levels']) if opt['--levels'] else None
    for lsh in settings if mode != 'exact' else [None]:
        for shared in opt['--shared'].split(','):
            run(H, W, steps, K, colour, shared == '1', mode, lsh, levels)


if __name__ == '__main__':
    main()
