"""3-channel matching with the level databases sharded over ranks (ia_color3.hip k_exact3p /
k_peer_finish3) on the GPU against the C oracle (nch = 3): rank processes sharing
the box's GPU over the device-side exchange (colour label maps whose flat queries tie across
ranks, inside one late rank, and over more than C3_CAND tiles of every rank; and a smooth-noise
input with every level sharded), 1-rank exchanges in this process (device-side and RCCL), the
refusals of the C-ABI, and the resources the forward-progress rule takes.  Every rank must end
with the oracle's B' in all three channels, s, im and approximate picks, bit for bit.
test_color3_shard_cases.py asserts, from the oracle alone, what each label case exercises."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

import colour_shards as cs
import test_gpu_exchange as xg
from test_gpu_exchange import dev

pytestmark = pytest.mark.gpu

# one launch per world: its cases run one after the other in one process group
LAUNCHES = {2: (1, ['at2', 'over', 'over-rot0', 'noise']), 3: (0, ['at2', 'tie_late', 'noise'])}
_RESULTS = {}


def run_ranks3(world, argv, timeout=100):
    """test_gpu_exchange.run_ranks (all ranks on cuda:0, IA_SHARD_MIN_ROWS=0, IA_SHARE_GPU=1, a
    time limit per rank) with exchange_worker3.py as the rank program: run_ranks names
    exchange_worker.py itself, so its Popen is given the colour worker's path in its place."""
    old, new = os.path.join(xg.HERE, 'exchange_worker.py'), os.path.join(xg.HERE, 'exchange_worker3.py')
    real = xg.subprocess

    def popen(cmd, **kw):
        return real.Popen([new if c == old else c for c in cmd], **kw)
    xg.subprocess = types.SimpleNamespace(Popen=popen, PIPE=real.PIPE, STDOUT=real.STDOUT)
    try:
        return xg.run_ranks(world, argv, timeout=timeout)
    finally:
        xg.subprocess = real


def launch(world, tmp_path_factory):
    """The ranks' results of one world's launch: {(rank, case): npz}, run once per session."""
    if world not in _RESULTS:
        pipeline, names = LAUNCHES[world]
        td = str(tmp_path_factory.mktemp('colour_shards_w%d' % world))
        outs = run_ranks3(world, [td, pipeline] + names)
        print(''.join(outs))
        _RESULTS[world] = {(r, n): dict(np.load(os.path.join(td, 'rank%d_%s.npz' % (r, n))))
                           for r in range(world) for n in names}
    return _RESULTS[world]


def assert_rank_matches(ref, got, who):
    """One rank's outputs against the oracle's: B', s, im and the approximate pick and distance
    of the debug record, per level."""
    A_pyr, _, B_pyr, _, L = ref.pyr
    for l in sorted(ref.ref):
        Bp, s, im = ref.ref[l]
        assert np.array_equal(got['s%d' % l], s), (who, l)
        assert np.array_equal(got['im%d' % l], im), (who, l)
        assert np.array_equal(got['bp%d' % l], Bp), (who, l)
        sa, d = ref.app[l]
        assert [(int(r), int(c)) for r, c in got['dbgpx%d' % l][:, 0:2]] == sa, (who, l)
        assert np.array_equal(got['dbgd%d' % l][:, 0].reshape(Bp.shape[:2]), d), (who, l)


@pytest.mark.parametrize('world,name', [(w, n) for w in sorted(LAUNCHES) for n in LAUNCHES[w][1]])
def test_ranks_on_one_gpu_match_oracle(gpu, tmp_path_factory, world, name):
    """`world` rank processes on the box's one GPU, every level's rows sharded over them, the
    records exchanged through each other's IPC-mapped boxes: every rank reproduces the oracle,
    reports the device-side exchange, and built only its own rows of the finest level.  `over`:
    every rank scanned all its tiles for the queries tied over more than C3_CAND of them; the
    other label cases scan only on tie_late's rank 2, whose shard is one row repeated."""
    res = launch(world, tmp_path_factory)
    base = name.partition('-rot')[0]
    ref = cs.reference(base)
    for r in range(world):
        got = res[(r, name)]
        assert str(got['exchange_kind']) == 'peer', (r, got['exchange_kind'])
        assert_rank_matches(ref, got, (world, name, r))
        fin = ref.L - 1
        assert bool(got['sharded%d' % fin])
        assert tuple(got['shard%d' % fin]) == cs.shard_rows(ref.N, r, world), r
        full = int(got['stats'][1])
        print('%s world %d rank %d: candidate tiles %d, full scans %d' % (name, world, r, got['stats'][0], full))
        if base == 'over':
            assert full >= 360, (r, full)
        elif base == 'tie_late' and r == 2:     # a constant shard (A = 0): the clamp's full scan
            assert full == ref.nn.size, (r, full)
        elif base != 'noise':                   # no query ties over more than C3_CAND tiles
            assert full == 0, (r, full)


def one_rank(kind, pipeline):
    """The noise input with every level sharded over a 1-rank exchange, in this process."""
    import _ia
    import image_analogies as ia
    ref = cs.reference('noise')
    A_pyr, Ap_list, B_pyr, Bp_pyr, L = ref.pyr
    comms = [_ia.exchange(0, 1, kind) for _ in range(1, L)]
    try:
        Bp_dev = [dev(b) for b in Bp_pyr]
        out = ia.synthesize_dev([dev(p) for p in A_pyr], [[dev(p) for p in q] for q in Ap_list],
                                [dev(p) for p in B_pyr], Bp_dev, L, ref.k, ref.w, comm=comms,
                                rank=0, nranks=1, pipeline=pipeline, debug=True)
        torch.cuda.synchronize()
        for cm in comms:
            _ia.exchange_status(cm)
        got = {}
        for l in out:
            got.update({'s%d' % l: out[l][0].cpu().numpy(), 'im%d' % l: out[l][1].cpu().numpy(),
                        'bp%d' % l: Bp_dev[l].cpu().numpy(), 'dbgpx%d' % l: out[l][2][0].cpu().numpy(),
                        'dbgd%d' % l: out[l][2][1].cpu().numpy()})
        assert set(out) == set(ref.ref)
        assert_rank_matches(ref, got, (kind, pipeline))
    finally:
        torch.cuda.synchronize()
        for cm in comms:
            _ia.check(_ia.lib().ia_comm_destroy(cm), 'ia_comm_destroy')


@pytest.mark.parametrize('kind,pipeline', [('peer', False), ('peer', True), ('rccl', True)])
def test_one_rank_exchange_matches_oracle(gpu, kind, pipeline):
    """Every level sharded over a 1-rank exchange (one per level): the four-launch sharded wave
    (device-side: publish and collect through this rank's own box; RCCL: the all-gather form)
    gives the oracle's B', s, im and debug record."""
    one_rank(kind, pipeline)


class ShardedLevel:
    """IaSynthArgs of the at2 input's level as rank 0 of 2 would run it over a 1-rank exchange
    handle (nothing is launched with it but refusals), outputs filled with -7."""

    def __init__(self):
        import _ia
        import algorithms
        import image_analogies as ia
        A_pyr, Ap_list, B_pyr, Bp_pyr, L = cs.label_pyramids('at2')
        self.comm = _ia.exchange(0, 1, 'peer')
        A = [dev(p) for p in A_pyr]
        Ap = [[dev(p) for p in q] for q in Ap_list]
        self.B, self.Bp = [dev(p) for p in B_pyr], [dev(p) for p in Bp_pyr]
        level = L - 1
        N = ia.level_rows(Ap_list, level)
        self.built = ia._db3_level(A, Ap, level, ia.shard_rows(N, 0, 2))
        self.rot, self.dbr = algorithms.rot3_build(self.built[6], self.built[7][1])
        self.w = _ia.to_dev(cs.o.compute_weights(3, 5, 12, 3))
        self.args, (self.s, self.im, _), self.bufs = ia._level3_args(
            self.built, self.rot, self.dbr, self.B, self.Bp, level, L, 1.0, self.w, False, self.comm)
        self.s.fill_(-7)
        self.im.fill_(-7)
        self.bp0 = self.Bp[level].clone()
        self.level = level

    def untouched(self):
        torch.cuda.synchronize()
        return (bool((self.s == -7).all()) and bool((self.im == -7).all()) and
                torch.equal(self.Bp[self.level], self.bp0))

    def close(self):
        import _ia
        torch.cuda.synchronize()
        _ia.check(_ia.lib().ia_comm_destroy(self.comm), 'ia_comm_destroy')


def copy_args(a):
    import _ia
    b = _ia.IaSynthArgs()
    ctypes.memmove(ctypes.byref(b), ctypes.byref(a), ctypes.sizeof(b))
    return b


def test_sharded_refusals_through_the_c_abi(gpu):
    """IA_E_ARG with a message, before anything is launched (every output keeps its fill): a
    sharded level with an lsh, with IA_COLOR16=0, inside ia_synth_levels3_batch, and with 2^32
    rows."""
    import _ia
    lib, st = _ia.lib(), _ia.stream()
    lv = ShardedLevel()
    prev = lib.ia_diag_set_color16(1)
    try:
        a = copy_args(lv.args)
        a.lsh = ctypes.pointer(_ia.IaLsh())
        assert lib.ia_synth_level3(ctypes.byref(a), st) == _ia.IA_E_ARG
        assert 'lsh' in lib.ia_last_error().decode()
        lib.ia_diag_set_color16(0)
        assert lib.ia_synth_level3(ctypes.byref(lv.args), st) == _ia.IA_E_ARG
        assert 'IA_COLOR16' in lib.ia_last_error().decode()
        arr = (_ia.IaSynthArgs * 1)(lv.args)
        assert lib.ia_synth_levels3(arr, 1, st) == _ia.IA_E_ARG
        assert 'IA_COLOR16' in lib.ia_last_error().decode()
        lib.ia_diag_set_color16(1)
        for K in (1, 2):
            arr = (_ia.IaSynthArgs * K)(*[lv.args] * K)
            assert lib.ia_synth_levels3_batch(arr, 1, K, st) == _ia.IA_E_ARG
            assert 'comm' in lib.ia_last_error().decode()
        big = copy_args(lv.args)          # 2^20 A' images of 64 x 64: 2^32 rows (no buffer is read)
        big.src.nAp, big.src.Ah, big.src.Aw = 1 << 20, 64, 64
        big.N_total = 1 << 32
        assert lib.ia_synth_level3(ctypes.byref(big), st) == _ia.IA_E_ARG
        assert '2^32' in lib.ia_last_error().decode()
        assert lv.untouched()
    finally:
        lib.ia_diag_set_color16(prev)
        lv.close()


def test_level3_resources_keep_a_screen_resident(gpu):
    """ia_level3_resources reports k_peer_finish3 and the level's screen.  The waiting kernel is
    small: at most 96 VGPRs and 12 KB of LDS, so that three of its workgroups fit a CU's SIMDs
    and LDS beside a 152-VGPR, 77 KB screen workgroup (residency_ok: jmax >= 3).  With the
    reported numbers the forward-progress rule keeps a screen workgroup resident beside the
    waiting ones for every world and input of this module, pipelined."""
    import _ia
    import image_analogies as ia
    lv = ShardedLevel()
    try:
        fused, screen = ia.level3_resources(lv.args)
        print('k_peer_finish3: %d B LDS, %d VGPRs; screen: %d B LDS, %d VGPRs' % (fused + screen))
        plain = copy_args(lv.args)
        plain.dbr = plain.rot = None
        _, screen0 = ia.level3_resources(plain)
        assert 0 < fused[0] <= 12 * 1024 and 0 < fused[1] <= 96
        assert ia.residency_ok(1, fused, screen)[1] >= 3
        assert screen[0] == 7 * 11 * 64 * 16 and screen0[0] == 4 * 22 * 64 * 16     # k_screen3r, k_screen3
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        for name in list(cs.CASES) + ['noise']:
            B_pyr, L = cs.pyramids(name)[0][2], cs.pyramids(name)[0][4]
            shapes = [B_pyr[l].shape[:2] for l in range(1, L)]
            for world in (2, 3):
                for sc in (screen, screen0):
                    assert ia.sharded_schedule(shapes, True, world, fused, sc, cus) is True
                    waiters = world * sum(ia.wave_max_queries(*s) for s in shapes)
                    assert ia.residency_ok(waiters, fused, sc, cus)[0]
    finally:
        lv.close()
