"""LSH batches of luminance jobs (synthesize_batch_dev(..., lsh=...), ia_synth_levels_lsh_batch:
the query rows, the LSH query and the LSH tail with the job as a grid dimension, one level index
with its tables per DB group and level) against a fresh synthesize_dev(lsh=...) of every job
alone, the oracle's LshIndex for job 0, the C-ABI's refusals and multi_main's files."""
import ctypes
import functools
import glob
import os

import numpy as np
import pytest
import torch

import ia_oracle as o
from conftest import analogy_inputs, smooth_noise

pytestmark = pytest.mark.gpu

PARAMS = (dict(tables=8, hashes=3, width=1.0, seed=7), dict(tables=4, hashes=1, width=4.0, seed=1))
IDS = lambda p: '%(tables)d-%(hashes)d-%(width)g-%(seed)d' % p  # noqa: E731
KAPPAS = (1.0, 5.0, 2.0)


def dev(a, dtype=torch.float64):
    return torch.as_tensor(np.ascontiguousarray(a)).to('cuda', dtype)


@functools.lru_cache(maxsize=None)
def host_jobs():
    """The host pyramids of three jobs in two groups, never modified: job 0 is
    test_lsh_synthesis_vs_oracle's, job 1 has its A / A' and another B and B' seed, job 2 an
    A / A' of its own of the same shapes.  Returns (jobs, groups, levels, weights)."""
    A, Aps, B = analogy_inputs(2, (30, 40), (28, 33), n_ap=2)
    j0 = o.setup_luminance(A, Aps, B, seed=2)
    j1 = o.setup_luminance(A, Aps, smooth_noise(53, (28, 33)), seed=54)
    A2, Aps2, B2 = analogy_inputs(61, (30, 40), (28, 33), n_ap=2)
    j2 = o.setup_luminance(A2, Aps2, B2, seed=63)
    assert j0[4] == j1[4] == j2[4]
    return [j0[:4], (j0[0], j0[1], j1[2], j1[3]), j2[:4]], [0, 0, 1], j0[4], o.compute_weights(3, 5, 12, 1)


def dev_jobs():
    """Fresh device jobs: jobs of one group get the SAME A and A' pyramid tensors."""
    jobs, groups, _, _ = host_jobs()
    sides, out = {}, []
    for (A_pyr, Ap_list, B_pyr, Bp_pyr), g in zip(jobs, groups):
        if g not in sides:
            sides[g] = ([dev(p) for p in A_pyr], [[dev(p) for p in q] for q in Ap_list])
        out.append(sides[g] + ([dev(p) for p in B_pyr], [dev(b) for b in Bp_pyr]))
    return out


def to_host(out, Bp_dev):
    torch.cuda.synchronize()
    return ({level: tuple(x.cpu().numpy() if torch.is_tensor(x) else tuple(y.cpu().numpy() for y in x)
                          for x in res) for level, res in out.items()},
            [b.cpu().numpy() for b in Bp_dev])


def frozen(params):
    return tuple(sorted(params.items()))


@functools.lru_cache(maxsize=None)
def alone(fparams, debug=False):
    """synthesize_dev(lsh=...) of every job alone, on device pyramids of its own: computed once
    per parameter set, shared by the tests, never modified."""
    import image_analogies as ia
    jobs, _, L, w = host_jobs()
    res = []
    for (A_pyr, Ap_list, B_pyr, Bp_pyr), k in zip(jobs, KAPPAS):
        Bp_dev = [dev(b) for b in Bp_pyr]
        out = ia.synthesize_dev([dev(p) for p in A_pyr], [[dev(p) for p in q] for q in Ap_list],
                                [dev(p) for p in B_pyr], Bp_dev, L, k, w, lsh=dict(fparams), debug=debug)
        res.append(to_host(out, Bp_dev))
    return res


def assert_same(got, want, tag):
    (out, Bp), (rout, rBp) = got, want
    assert sorted(out) == sorted(rout), tag
    for level in rout:
        assert len(out[level]) == len(rout[level]), (tag, level)
        assert np.array_equal(out[level][0], rout[level][0]), (tag, level, 's')
        assert np.array_equal(out[level][1], rout[level][1]), (tag, level, 'im')
        if len(rout[level]) > 2:
            for x, y in zip(out[level][2], rout[level][2]):
                assert np.array_equal(x, y), (tag, level, 'debug')
        assert np.array_equal(Bp[level], rBp[level]), (tag, level, "B'")


def run_batch(params, debug=False):
    import image_analogies as ia
    _, _, L, w = host_jobs()
    jobs = dev_jobs()
    outs = ia.synthesize_batch_dev(jobs, L, list(KAPPAS), w, debug=debug, lsh=params)
    return [to_host(out, job[3]) for out, job in zip(outs, jobs)]


@pytest.mark.parametrize('params', PARAMS, ids=IDS)
def test_three_jobs_two_groups(gpu, params):
    """Every job's s, im and B' at every level equal its own unbatched run; job 0 (kappa 1) also
    equals the scanline oracle driven by LshIndex over the device's centre, width and
    projections.  A job reading another job's tables, centre, weights or B', or a group's width
    applied to the other group, shows here."""
    import algorithms
    got = run_batch(params)
    want = alone(frozen(params))
    jobs, _, L, w = host_jobs()
    for q in range(3):
        assert_same(got[q], want[q], 'job %d' % q)
    assert not np.array_equal(want[0][0][L - 1][0], want[1][0][L - 1][0])
    assert not np.array_equal(want[0][0][L - 1][0], want[2][0][L - 1][0])
    A_pyr, Ap_list, B_pyr, Bp_pyr = jobs[0]
    A_d, Ap_d = [dev(p) for p in A_pyr], [[dev(p) for p in q] for q in Ap_list]
    As = o.create_index(A_pyr, Ap_list, L)
    Bp_ref = [b.copy() for b in Bp_pyr]
    out, Bp = got[0]
    for level in range(1, L):
        index = algorithms.level_index(A_d, Ap_d, level, lsh=params)
        h = index.lsh
        lsh = o.LshIndex(As[level], index.center.cpu().numpy(), index.lsh_proj_host, h.L, h.k, np.float32(h.w))
        rs_, rim = o.synthesize_level(level, L, A_pyr, Ap_list, B_pyr, Bp_ref, As[level], w, 1.0,
                                      matcher=lambda q: lsh.match(q)[0][0])
        assert np.array_equal(out[level][0], rs_), level
        assert np.array_equal(out[level][1], rim), level
        assert np.array_equal(Bp[level], Bp_ref[level]), level


def test_one_job_and_repetition(gpu):
    """K = 1 through ia_synth_levels_lsh_batch makes the single job's run; a second call on
    fresh B' copies gives the same result."""
    import image_analogies as ia
    params = PARAMS[0]
    _, _, L, w = host_jobs()
    want = alone(frozen(params))
    for _ in range(2):
        job = dev_jobs()[0]
        outs = ia.synthesize_batch_dev([job], L, [KAPPAS[0]], w, lsh=params)
        assert len(outs) == 1
        assert_same(to_host(outs[0], job[3]), want[0], 'K = 1')
    first = run_batch(params)
    again = run_batch(params)
    for q in range(3):
        assert_same(again[q], first[q], 'second call, job %d' % q)
        assert_same(again[q], want[q], 'second call, job %d' % q)


def test_debug_tensors(gpu):
    params = PARAMS[0]
    got = run_batch(params, debug=True)
    want = alone(frozen(params), debug=True)
    L = host_jobs()[2]
    for q in range(3):
        assert len(got[q][0][L - 1]) == 3 and len(want[q][0][L - 1]) == 3
        assert_same(got[q], want[q], 'job %d' % q)
    assert got[0][0][L - 1][2][0].any()       # (the records are written)


def batch_calls(jobs, params, debug=False):
    """The _LevelCall list of synthesize_batch_dev(lsh=params) (level-major), nothing launched."""
    import _ia
    import algorithms
    import image_analogies as ia
    _, _, L, w = host_jobs()
    group = ia.db_groups(jobs)
    wd = _ia.to_dev(w)
    calls = []
    for level in range(1, L):
        shared = {}
        for q, (A_pyr, Ap_list, B_pyr, Bp_pyr) in enumerate(jobs):
            if group[q] not in shared:
                shared[group[q]] = algorithms.level_index(A_pyr, Ap_list, level, None, params)
            calls.append(ia._LevelCall(level, L, shared[group[q]], B_pyr[level - 1], B_pyr[level],
                                       Bp_pyr[level - 1], Bp_pyr[level], wd, KAPPAS[q], None, False, False, debug))
    return calls


def test_one_table_set_per_group_and_level(gpu, monkeypatch):
    """LevelIndex.build_lsh runs 2 x levels times for the three jobs of two groups, and the jobs
    of a group pass the same lsh->mem and centre."""
    import _ia
    import algorithms
    params = PARAMS[0]
    L = host_jobs()[2]
    calls = []
    real = algorithms.LevelIndex.build_lsh

    def counted(self, *a, **k):
        calls.append(1)
        return real(self, *a, **k)
    monkeypatch.setattr(algorithms.LevelIndex, 'build_lsh', counted)
    seen = []
    lib = _ia.lib()
    entry = lib.ia_synth_levels_lsh_batch

    class Spy:
        def __getattr__(self, name):
            return getattr(lib, name)

        def ia_synth_levels_lsh_batch(self, arr, n, K, st):
            seen.append([(a.lsh.contents.mem, a.center, a.workspace, a.s) for a in arr])
            return entry(arr, n, K, st)
    monkeypatch.setattr(_ia, 'lib', lambda: Spy())
    got = run_batch(params)
    assert len(calls) == 2 * (L - 1)
    assert len(seen) == 1 and len(seen[0]) == 3 * (L - 1)
    for j in range(L - 1):
        a0, a1, a2 = seen[0][3 * j:3 * j + 3]
        assert a0[0] == a1[0] != a2[0] and a0[1] == a1[1] != a2[1]
        assert len({a0[2], a1[2], a2[2]}) == 3 and len({a0[3], a1[3], a2[3]}) == 3
    for q, w in enumerate(alone(frozen(params))):
        assert_same(got[q], w, 'job %d' % q)


def copy_struct(x):
    y = type(x)()
    ctypes.memmove(ctypes.byref(y), ctypes.byref(x), ctypes.sizeof(y))
    return y


def test_refusals_through_the_c_abi(gpu):
    """IA_E_ARG before anything is enqueued, the field named, every output keeping its fill;
    then the unchanged arguments run."""
    import _ia
    import algorithms
    lib, st = _ia.lib(), _ia.stream()
    params = PARAMS[0]
    L = host_jobs()[2]
    jobs = dev_jobs()
    calls = batch_calls(jobs, params)
    last = calls[3 * (L - 2):]
    level = L - 1
    trio = lambda: (_ia.IaSynthArgs * 3)(*[copy_struct(c.args) for c in last])  # noqa: E731
    fills = []
    for q in range(3):
        last[q].s.fill_(-7)
        last[q].im.fill_(-7)
        fills.append((last[q].s, last[q].im, jobs[q][3][level], jobs[q][3][level].clone()))
    good = trio()
    other = algorithms.level_index(*dev_jobs()[0][:2], level, None, params)   # job 0's index again
    spare = torch.zeros(56 * 64, dtype=torch.float32, device='cuda')
    dbg = (torch.zeros((28 * 33, 7), dtype=torch.int32, device='cuda'),
           torch.zeros((28 * 33, 2), dtype=torch.float64, device='cuda'))

    def lsh_with(a, **fields):
        h = copy_struct(a.lsh.contents)
        for f, v in fields.items():
            setattr(h, f, v)
        a.lsh = ctypes.pointer(h)
        return h

    def case(what, change, K=3):
        bad = trio()
        held = change(bad)
        sub = (_ia.IaSynthArgs * K)(*bad[:K])
        assert lib.ia_synth_levels_lsh_batch(sub, 1, K, st) == _ia.IA_E_ARG, what
        msg = lib.ia_last_error().decode()
        assert what in msg, (what, msg)
        del held

    def set1(field, value):
        return lambda bad: setattr(bad[1], field, value)
    case('lsh', set1('lsh', None))
    case('center', set1('center', None))
    case('center', lambda bad: setattr(bad[0], 'center', None), K=1)
    case('comm', set1('comm', 0x1000))                       # (refused before it is looked into)
    case('differ in nrows', set1('nrows', good[1].nrows - 1))
    case('row0', lambda bad: [setattr(b, 'nrows', b.nrows - 1) for b in bad])
    case('differ in H', set1('H', good[1].H - 1))
    case('differ in src.Aw', lambda bad: setattr(bad[2].src, 'Aw', bad[2].src.Aw - 1))
    case('differ in lsh->L', lambda bad: lsh_with(bad[2], L=good[2].lsh.contents.L - 1))
    case('differ in lsh->k', lambda bad: lsh_with(bad[2], k=good[2].lsh.contents.k - 1))

    def with_debug(bad):
        bad[1].dbg_px, bad[1].dbg_dist = _ia.ptr(dbg[0]).value, _ia.ptr(dbg[1]).value
    case('debug outputs', with_debug)
    case('sharing lsh->mem differ in lsh->proj', lambda bad: lsh_with(bad[1], proj=_ia.ptr(spare).value))
    case('sharing lsh->mem differ in lsh->w', lambda bad: lsh_with(bad[1], w=good[1].lsh.contents.w * 2))
    case('sharing lsh->mem differ in center', set1('center', good[2].center))
    case('sharing lsh->mem differ in src.Ap_lg',
         lambda bad: setattr(bad[1].src, 'Ap_lg', _ia.ptr(other.Ap_lg).value))
    case('L*k', lambda bad: [lsh_with(b, L=13, k=5) for b in bad])
    case('mem, proj', lambda bad: lsh_with(bad[2], proj=None))
    for K in (0, 129):
        assert lib.ia_synth_levels_lsh_batch(good, 1, K, st) == _ia.IA_E_ARG
        assert 'K out of range' in lib.ia_last_error().decode()
    torch.cuda.synchronize()
    for s, im, bp, bp0 in fills:
        assert bool((s == -7).all()) and bool((im == -7).all()) and torch.equal(bp, bp0)
    assert lib.ia_synth_levels_lsh_batch(good, 1, 3, st) == 0
    assert lib.ia_synth_status(good, 3, st) == 0
    for s, im, bp, bp0 in fills:
        assert not bool((s == -7).any()) and not bool((im == -7).any()) and not torch.equal(bp, bp0)


def test_multi_main_files(gpu, monkeypatch, tmp_path):
    """multi_main(batch=3) with convert=True under c.matcher = 'lsh' on three runs from small
    colour files (runs 0 and 1 name one A / A' pair): ONE synthesize_batch_dev call carrying the
    lsh, files byte-identical to the unbatched loop's; none with IA_LSH_BATCH=0."""
    from PIL import Image
    from scipy.ndimage import gaussian_filter
    import algorithms
    import config
    import image_analogies as ia
    import lsh3_ref as r

    def png(name, img):
        path = str(tmp_path / (name + '.png'))
        Image.fromarray(np.clip(np.round(img * 255), 0, 255).astype(np.uint8), 'RGB').save(path)
        return path
    A = r.colour(581, (26, 30))
    fA = png('A', A)
    fAp = png('Ap', np.dstack([gaussian_filter(A[..., ch], 1.2) for ch in range(3)]))
    fAp2 = png('Ap2', np.dstack([gaussian_filter(A[..., ch], 2.0) for ch in range(3)]))
    fB = [png('B%d' % i, r.colour(582 + i, (24, 20))) for i in range(3)]
    ks = [1.0, 6.0, 0.5]
    old = config.matcher, config.convert

    def fresh():
        config.convert, config.remap_lum, config.init_rand, config.AB_weight = True, False, True, 1
        config.k, config.seed, config.levels, config.matcher = 1.0, 5, None, 'lsh'
        return config

    def runs(tag):
        d = lambda i: str(tmp_path / ('%s%d' % (tag, i))) + '/'  # noqa: E731
        return [(fA, [fAp if i < 2 else fAp2], fB[i], d(i), {'k': ks[i]}) for i in range(3)]
    spied = []
    real = ia.synthesize_batch_dev

    def spy(jobs, *a, **k):
        spied.append((len(jobs), k.get('lsh')))
        return real(jobs, *a, **k)
    monkeypatch.setattr(ia, 'synthesize_batch_dev', spy)
    try:
        monkeypatch.delenv('IA_LSH_BATCH', raising=False)
        monkeypatch.setitem(ia.LSH_BATCH_DEFAULT, False, 1)
        got = ia.multi_main(runs('b'), fresh(), rank=0, world=1, batch=3)
        assert spied == [(3, algorithms.lsh_params(config))] and spied[0][1] is not None
        del spied[:]
        monkeypatch.setenv('IA_LSH_BATCH', '0')
        off = ia.multi_main(runs('o'), fresh(), rank=0, world=1, batch=3)
        assert spied == []
        ref = ia.multi_main(runs('u'), fresh(), rank=0, world=1)
        assert spied == []
    finally:
        config.matcher, config.convert = old
    L = len(ref[0])
    assert sorted(got) == sorted(off) == sorted(ref) == [0, 1, 2]
    for j in ref:
        for x, y, z in zip(got[j], off[j], ref[j]):
            assert np.array_equal(x, z) and np.array_equal(y, z), j
        names = sorted(os.path.basename(p) for p in glob.glob(str(tmp_path / ('u%d' % j) / '*.jpg')))
        assert len(names) >= L
        for n in names:
            want = (tmp_path / ('u%d' % j) / n).read_bytes()
            for tag in 'bo':
                assert (tmp_path / ('%s%d' % (tag, j)) / n.replace('u%d' % j, '%s%d' % (tag, j))).read_bytes() == want, \
                    (tag, j, n)
