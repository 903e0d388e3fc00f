"""One rank of a multi-process sharded 3-channel synthesis (tests/test_gpu_color3_shards.py):
exchange_worker.py's colour counterpart, started the same way (RANK, WORLD_SIZE,
MASTER_ADDR/PORT in the environment, gloo rendezvous, every rank on the device named by
IA_TEST_DEVICE: the ranks share the box's GPU, their receive boxes IPC-mapped between the
processes).  Every level with a DB of >= IA_SHARD_MIN_ROWS rows is sharded.

usage: exchange_worker3.py OUT PIPELINE NAME...
    the named inputs of colour_shards (a label case, or `noise`; a `-rot0` suffix runs it with
    IA_DB_ROT=0), one after the other in this process group over the device-side exchange, each
    a debug synthesis; each rank writes OUT/rank<r>_<NAME>.npz: per level l s, im, bp (B'),
    dbgpx / dbgd (the debug record), shard (row0, nrows of the database _db3_level built),
    sharded; and exchange_kind, stats ([candidate tiles, full scans] of this rank's exact stage,
    ia_diag_color16_stats).
"""
import ctypes
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import conftest  # noqa: E402,F401  (import paths: package + oracle)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

import colour_shards as cs  # noqa: E402
from exchange_worker import destroy, dev  # noqa: E402


def run_case(out_dir, name, rank, world, pipeline):
    import _ia
    import image_analogies as ia
    base, _, rot = name.partition('-rot')
    os.environ.pop('IA_DB_ROT', None)
    if rot:
        os.environ['IA_DB_ROT'] = rot
    (A_pyr, Ap_list, B_pyr, Bp_pyr, L), k = cs.pyramids(base)
    w = cs.o.compute_weights(3, 5, 12, 3)
    built = {}
    real = ia._db3_level

    def recording(A, Ap, level, row_range=None):
        built[level] = real(A, Ap, level, row_range)
        return built[level]
    comms = [_ia.exchange(rank, world, 'peer') for _ in range(ia.sharded_level_count(Ap_list, L, world))]
    st = (ctypes.c_ulonglong * 2)()
    try:
        Bp_dev = [dev(b) for b in Bp_pyr]
        ia._db3_level = recording
        _ia.check(_ia.lib().ia_diag_color16_stats(st), 'stats')       # (reading clears the counters)
        try:
            out = ia.synthesize_dev([dev(p) for p in A_pyr], [[dev(p) for p in q] for q in Ap_list],
                                    [dev(p) for p in B_pyr], Bp_dev, L, k, w, comm=comms,
                                    rank=rank, nranks=world, pipeline=pipeline, debug=True)
        finally:
            ia._db3_level = real
        _ia.check(_ia.lib().ia_diag_color16_stats(st), 'stats')
        for cm in comms:
            _ia.exchange_status(cm)
        res = {'exchange_kind': _ia.exchange_kind(), 'stats': np.array([st[0], st[1]], dtype=np.int64)}
        for l in out:
            N, (row0, nrows) = built[l][5], built[l][7]
            res.update({'s%d' % l: out[l][0].cpu().numpy(), 'im%d' % l: out[l][1].cpu().numpy(),
                        'bp%d' % l: Bp_dev[l].cpu().numpy(), 'dbgpx%d' % l: out[l][2][0].cpu().numpy(),
                        'dbgd%d' % l: out[l][2][1].cpu().numpy(), 'shard%d' % l: np.array([row0, nrows]),
                        'sharded%d' % l: nrows < N or world == 1})
        np.savez(os.path.join(out_dir, 'rank%d_%s.npz' % (rank, name)), **res)
    finally:
        built.clear()
        destroy(comms)


def main():
    rank, world = int(os.environ['RANK']), int(os.environ['WORLD_SIZE'])
    dist.init_process_group('gloo')
    torch.cuda.set_device(int(os.environ.get('IA_TEST_DEVICE', '0')))
    try:
        out_dir, pipe = sys.argv[1:3]
        for name in sys.argv[3:]:
            t0 = time.time()
            run_case(out_dir, name, rank, world, pipe == '1')
            print('rank %d %s: %.1f s' % (rank, name, time.time() - t0), flush=True)
        dist.barrier()
    finally:
        # (no barrier after a failure: the other ranks may be inside another collective)
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
