"""Time of a luminance synthesis from n training pairs (A_i, A'_i) against the run it should
cost the same as: one A with n A' images (the same row count, the same DB forms at widths that
are no multiple of 128), on one GPU, from device pyramids (B' reset every step).

usage: python tools/pairs_bench.py H W steps [--pairs 0|1] [--n N] [--warmup W]
       H x W: the size of every image (bench.py's c1 is 180 x 117).  --pairs 1 [default]: N
       pairs, A_pyr a list of N pyramids; --pairs 0: A_0 with the N A' images.  With --pairs 0
       it makes only calls that revisions without pairs have too, so the same file measures
       such a revision when it is copied into that tree.
Prints one JSON line: the median, the minimum and every step's time in ms, and a B' checksum.
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
    opt = {'--pairs': 1, '--n': 2, '--warmup': 3}
    for name in list(opt):
        if name in args:
            i = args.index(name)
            opt[name] = int(args[i + 1])
            del args[i:i + 2]
    H, W, steps = (int(x) for x in args[:3])
    n = opt['--n']
    from scipy.ndimage import gaussian_filter
    dev = 'cuda:0'
    up = lambda x: torch.as_tensor(x).to(dev)  # noqa: E731
    pyr = lambda x: ip.gaussian_pyramid_dev(up(x), cfg.n_sm, None)  # noqa: E731
    As = [bench.smooth_noise(7 + 10 * i, (H, W)) for i in range(n)]
    Aps = [gaussian_filter(A, 1.0 + 0.5 * i) for i, A in enumerate(As)]
    A_pyrs, Ap_list = [pyr(A) for A in As], [pyr(Ap) for Ap in Aps]
    B_pyr = pyr(bench.smooth_noise(8, (H, W)))
    L = min(len(A_pyrs[0]), len(B_pyr))
    init = [up(x) for x in ip.initialize_Bp([np.empty(tuple(p.shape)) for p in B_pyr], True, 9)]
    w = torch.as_tensor(cfg.compute_weights(3, 5, 12, 1)).to(dev)
    A_arg = A_pyrs if opt['--pairs'] else A_pyrs[0]
    times = []
    Bp = None
    for it in range(opt['--warmup'] + steps):
        Bp = [x.clone() for x in init]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ia.synthesize_dev(A_arg, Ap_list, B_pyr, Bp, L, 0.5, w)
        torch.cuda.synchronize()
        if it >= opt['--warmup']:
            times.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({'shape': [H, W], 'n': n, 'pairs': bool(opt['--pairs']), 'levels': L - 1,
                      'rows_finest': n * H * W, 'ms_median': float(np.median(times)),
                      'ms_min': float(np.min(times)), 'ms': [round(t, 3) for t in times],
                      'checksum': float(sum(float(b.sum().item()) for b in Bp[1:L]))}))


if __name__ == '__main__':
    main()
