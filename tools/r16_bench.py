"""Timing of the rotated screen (R16, k_screen16r<G>) on c4's finest level: the product's
dominant kernel over the 4,194,304-row rotated DB at M queries from
tests/golden/c4_queries.npz, HIP events around reps launches (IA_LIB_PATH selects a variant
build, tools/build_variant.sh).  Prints per M: mean us per launch, algorithmic frac of the
f16 peak (110 flop per pair), pipe frac (160 f16 flop issued per pair), DB GB/s.
--compact times the compact screen instead (k_screen16c over the compact DB,
ia_diag_screen16k; DB GB/s of its 64-B rows).  'minima' is a checksum of the segment minima's
bit patterns: builds whose minima agree bit for bit print the same value.

  python tools/r16_bench.py [--compact] [--M 342,256,128] [--reps 20] [--sleep CYCLES]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'image-analogies-python_amd'))
sys.path.insert(0, ROOT)

import _ia            # noqa: E402
import algorithms     # noqa: E402
import bench          # noqa: E402
import config as cfg  # noqa: E402
import img_preprocess as ip  # noqa: E402

F16_PEAK = 4096.0 * 256 * 2.4e9 / 1e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--M', default='342,256,128')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--sleep', default='0', help='GPU cycles of idle spin after each launch '
                    '(torch.cuda._sleep: the product\'s gaps between screens); not counted.  A comma '
                    'list times every M once per value')
    ap.add_argument('--compact', action='store_true', help='the compact screen (ia_diag_screen16k)')
    ap.add_argument('--stamps', action='store_true', help='with --compact and a library built with '
                    '-DIA_R16_STAMPS=1 (tools/build_variant.sh): one more launch per M whose stage stamps '
                    '(wave 0 of 8 blocks, s_memtime at 5 points per stage) are reduced to the median cycles '
                    'and share per phase.  The stamps cost cycles themselves: shares, not times')
    args = ap.parse_args()
    Ms = [int(x) for x in args.M.split(',')]
    dev = torch.device('cuda', 0)
    job = bench.Job(bench.CONFIGS['c4'], 0, dev)
    A_pyr = ip.gaussian_pyramid_dev(job.A, cfg.n_sm, job.levels)
    Ap_pyr = ip.gaussian_pyramid_dev(job.Ap, cfg.n_sm, job.levels)
    level = job.max_levels - 1
    idx = algorithms.level_index(A_pyr, [Ap_pyr], level, rot=True)
    assert idx.dbr is not None and (idx.dbk is not None or not args.compact)
    lib = _ia.lib()
    screen, db = (lib.ia_diag_screen16k, idx.dbk) if args.compact else (lib.ia_diag_screen16r, idx.dbr)
    N = idx.nrows
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'c4_queries.npz'))
    Mmax = max(Ms)
    qrows = lib.ia_diag_qp_rows(Mmax)
    q64 = torch.zeros((Mmax, _ia.IA_DP), dtype=torch.float64, device=dev)
    q64[:, :55] = torch.as_tensor(np.asarray(g['q'][:Mmax], dtype=np.float64)).to(dev)
    q16 = torch.zeros((qrows, 128), dtype=torch.float16, device=dev)
    nq = torch.zeros(qrows, dtype=torch.float64, device=dev)
    nsk = torch.zeros(qrows, dtype=torch.float64, device=dev)
    nseg = lib.ia_db_rows_padded(N) // min(lib.ia_db_chunk_rows(N), 512)
    segmin = torch.zeros((qrows, nseg), dtype=torch.float32, device=dev)
    st = _ia.stream()
    out = []
    for M in Ms:
        def run():
            _ia.check(screen(ctypes.byref(idx.src), idx.row0, N, _ia.ptr(db), _ia.ptr(idx.rot),
                             _ia.ptr(idx.amax), _ia.ptr(idx.center), _ia.ptr(q64), M, _ia.ptr(q16),
                             _ia.ptr(nq), _ia.ptr(nsk), _ia.ptr(segmin), st), 'screen16')
        for _ in range(3):
            run()
        torch.cuda.synchronize()
        for sleep in [int(x) for x in args.sleep.split(',')]:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            if sleep:
                ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                      for _ in range(args.reps)]
                for a, b in ev:
                    a.record()
                    run()
                    b.record()
                    torch.cuda._sleep(sleep)
                torch.cuda.synchronize()
                us = sum(a.elapsed_time(b) for a, b in ev) * 1e3 / args.reps
            else:
                e0.record()
                for _ in range(args.reps):
                    run()
                e1.record()
                torch.cuda.synchronize()
                us = e0.elapsed_time(e1) * 1e3 / args.reps
            pairs = M * N
            db_bytes = lib.ia_db_rotk_bytes(N) if args.compact else lib.ia_db_rot_bytes(N)
            minima = int(segmin[:M].view(torch.int32).to(torch.int64).sum().item())
            slots = 32 if args.compact else lib.ia_db_rot_slots()
            out.append({'M': M, 'us': round(us, 1), 'frac': 110 * pairs / (us * 1e-6) / 1e12 / F16_PEAK,
                        'pipe_frac': 2 * slots * pairs / (us * 1e-6) / 1e12 / F16_PEAK,
                        'P': lib.ia_db_rot_components(),
                        'db_gbs': db_bytes / (us * 1e-6) / 1e9, 'compact': args.compact,
                        'minima': minima, 'sleep': sleep, 'lib': os.environ.get('IA_LIB_PATH', 'libia.so')})
            print(json.dumps(out[-1]), flush=True)
        if args.stamps:
            print(json.dumps(stage_stamps(lib, run, M)), flush=True)


PHASES = ('issue+chains', 'close+flush', 'vmcnt wait', 'barrier', 'loop')


def stage_stamps(lib, run, M):
    """One launch's stage stamps (csrc/ia_screen16r.hip IA_R16_STAMPS): per phase the median cycles
    over the stamped (block, stage) pairs and its share of the stage (top to next top)."""
    assert hasattr(lib, 'ia_lab_r16_stamps'), 'a library built with -DIA_R16_STAMPS=1'
    fn = lib.ia_lab_r16_stamps
    fn.restype, fn.argtypes = ctypes.c_int, [ctypes.c_void_p]
    buf = np.zeros((8, 64, 5), dtype=np.uint64)
    _ia.check(fn(buf.ctypes.data), 'clear')
    run()
    _ia.check(fn(buf.ctypes.data), 'ia_lab_r16_stamps')
    t = buf.astype(np.int64)
    d = []
    for b in range(8):
        n = int((t[b, :, 0] != 0).sum())               # stages this block stamped
        for s in range(n - 1):                         # (the last stage has no next top)
            x = list(t[b, s]) + [t[b, s + 1, 0]]
            d.append([x[i + 1] - x[i] for i in range(5)])
    d = np.asarray(d, dtype=np.float64)
    med = np.median(d, axis=0)
    return {'M': M, 'stamped_stages': len(d), 'stage_cycles_median': float(np.median(d.sum(1))),
            'phase_median_cycles': dict(zip(PHASES, [float(x) for x in med])),
            'phase_share_of_sum': dict(zip(PHASES, [round(float(x), 4) for x in d.sum(0) / d.sum()])),
            'lib': os.environ.get('IA_LIB_PATH', 'libia.so')}


if __name__ == '__main__':
    main()
