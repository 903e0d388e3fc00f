"""One rank of a multi-process sharded synthesis (tests/test_gpu_exchange.py,
tests/test_gpu_shards.py).

Started by the test as a child process per rank (RANK, WORLD_SIZE, MASTER_ADDR/PORT in
the environment, gloo rendezvous); every rank runs on the device named by IA_TEST_DEVICE
(the test box has one GPU, so all ranks share cuda:0 — the device-side exchange's boxes
are then IPC-mapped between processes of one GPU, the same protocol as over xGMI).
Every level with a DB of >= IA_SHARD_MIN_ROWS rows is sharded.

usage: exchange_worker.py OUT SEED AH AW BH BW NAP KAPPA KIND PIPELINE
           smooth noise; each rank writes its per-level (B', s, im) to OUT/rank<r>.npz
       exchange_worker.py --cases OUT PIPELINE NAME...
           the named cases of test_gpu_shards.shard_spec, one after the other in this process
           group, over the device-side exchange; each rank writes OUT/rank<r>_<NAME>.npz
           (run_case)
"""
import ctypes
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import conftest  # noqa: E402  (import paths: package + oracle)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

import ia_oracle as o  # noqa: E402

CASE_ENV = ('IA_ROT_MIN_ROWS', 'IA_DB_ROT')     # a case's own settings, read when an index is built
PROF = ('full_scans', 'candidate_segments', 'rows_rescored', 'jobs')


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to('cuda', dtype=torch.float64)


def destroy(comms):
    import _ia
    torch.cuda.synchronize()
    for cm in comms:
        _ia.check(_ia.lib().ia_comm_destroy(cm), 'ia_comm_destroy')


def run_case(out_dir, name, rank, world, pipeline):
    """One named case: the pyramids from the generators the parent uses (no oracle run here),
    one device-side exchange per sharded level, a profiled debug synthesis.  The file holds per
    level l: s, im, bp (B'), dbgpx / dbgd (the debug record), prof (PROF), sharded, shard (row0,
    nrows of the index the product built), forms (whether index.db, .dbi, .dbr exist), stage_map
    (ia_diag_stage_map of the shard); and exchange_kind, xwave (the value given to
    ia_diag_set_xwave: IA_XWAVE, default 2)."""
    import _ia
    import algorithms
    import image_analogies as ia
    import test_gpu_fallback as fb
    from test_gpu_shards import shard_spec
    spec, env = shard_spec(name)
    for key in CASE_ENV:
        os.environ.pop(key, None)
    os.environ.update(env)
    xw = int(os.environ.get('IA_XWAVE', '2'))
    _ia.xwave(xw)
    A_pyr, Ap_list, B_pyr, Bp_pyr, L = fb.case_pyramids(spec['images'], spec['cap'], spec['seed'],
                                                        spec.get('bp_scale'), spec.get('setup'))
    w = o.compute_weights(3, 5, 12, 1)
    built = {}
    real = algorithms.level_index

    def recording(A, Ap, level, row_range=None, *args, **kw):
        built[level] = (real(A, Ap, level, row_range, *args, **kw), row_range is not None)
        return built[level][0]
    comms = [_ia.exchange(rank, world, 'peer')
             for _ in range(ia.sharded_level_count(Ap_list, L, world))]
    try:
        Bp_dev = [dev(b) for b in Bp_pyr]
        algorithms.level_index = recording
        _ia.prof_begin()
        try:
            out = ia.synthesize_dev([dev(p) for p in A_pyr], [[dev(p) for p in q] for q in Ap_list],
                                    [dev(p) for p in B_pyr], Bp_dev, L, spec['k'], w, comm=comms,
                                    rank=rank, nranks=world, pipeline=pipeline, prof=True, debug=True)
        finally:
            algorithms.level_index = real
            recs = _ia.prof_end()
        for cm in comms:
            _ia.exchange_status(cm)
        res = {'exchange_kind': _ia.exchange_kind(), 'xwave': xw}
        for l in out:
            rec = [r for r in recs if r['level'] == l]
            assert len(rec) == 1, (l, recs)
            index, sharded = built[l]
            m = (ctypes.c_int * 3)()
            _ia.check(_ia.lib().ia_diag_stage_map(index.row0, index.nrows, index.src.Aw, index.src.Ah, m),
                      'ia_diag_stage_map')
            res.update({'s%d' % l: out[l][0].cpu().numpy(), 'im%d' % l: out[l][1].cpu().numpy(),
                        'bp%d' % l: Bp_dev[l].cpu().numpy(), 'dbgpx%d' % l: out[l][2][0].cpu().numpy(),
                        'dbgd%d' % l: out[l][2][1].cpu().numpy(),
                        'prof%d' % l: np.array([rec[0][k] for k in PROF], dtype=np.int64),
                        'sharded%d' % l: sharded, 'shard%d' % l: np.array([index.row0, index.nrows]),
                        'forms%d' % l: np.array([x is not None for x in (index.db, index.dbi, index.dbr)]),
                        'stage_map%d' % l: np.array(list(m))})
        np.savez(os.path.join(out_dir, 'rank%d_%s.npz' % (rank, name)), **res)
    finally:
        built.clear()
        destroy(comms)


def run_noise(argv, rank, world):
    out_dir, seed, Ah, Aw, Bh, Bw, nap, kappa, kind, pipe = argv[:10]
    seed, Ah, Aw, Bh, Bw, nap = map(int, (seed, Ah, Aw, Bh, Bw, nap))
    kappa = float(kappa)
    import _ia
    import image_analogies as ia
    A, Aps, B = conftest.analogy_inputs(seed, (Ah, Aw), (Bh, Bw), n_ap=nap)
    A_pyr, Ap_list, B_pyr, Bp_pyr, L = o.setup_luminance(A, Aps, B, seed=seed)
    w = o.compute_weights(3, 5, 12, 1)
    comms = [_ia.exchange(rank, world, kind) for _ in range(1, L)]
    try:
        Bp_dev = [dev(b) for b in Bp_pyr]
        out = ia.synthesize_dev([dev(p) for p in A_pyr], [[dev(p) for p in q] for q in Ap_list],
                                [dev(p) for p in B_pyr], Bp_dev, L, kappa, w, comm=comms,
                                rank=rank, nranks=world, pipeline=(pipe == '1'))
        torch.cuda.synchronize()
        for cm in comms:
            _ia.exchange_status(cm)
        res = {}
        for l in out:
            res['s%d' % l] = out[l][0].cpu().numpy()
            res['im%d' % l] = out[l][1].cpu().numpy()
            res['bp%d' % l] = Bp_dev[l].cpu().numpy()
        np.savez(os.path.join(out_dir, 'rank%d.npz' % rank), **res)
    finally:
        destroy(comms)


def main():
    rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
    dist.init_process_group('gloo')
    torch.cuda.set_device(int(os.environ.get('IA_TEST_DEVICE', '0')))
    try:
        if sys.argv[1] == '--cases':
            out_dir, pipe = sys.argv[2:4]
            for name in sys.argv[4:]:
                t0 = time.time()
                run_case(out_dir, name, rank, world, pipe == '1')
                print('rank %d %s: %.1f s' % (rank, name, time.time() - t0), flush=True)
        else:
            run_noise(sys.argv[1:], rank, world)
        dist.barrier()
    finally:
        # (no barrier after a failure: the other ranks may be inside another collective, and
        # their next one fails at once when this rank is gone)
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
