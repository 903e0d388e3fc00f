"""LSH batches of 3-channel jobs (synthesize_batch_dev(..., lsh=...), ia_synth_levels3_lsh_batch:
k_query3b and k_lsh3_pixelb with the job as a grid dimension, one set of tables per DB group and
level) against a fresh synthesize_dev(lsh=...) of every job alone, the restatement-driven oracle
(tests/lsh3_ref.py) for job 0, the C-ABI's refusals and multi_main's files."""
import ctypes
import functools
import glob
import os

import numpy as np
import pytest
import torch

import ia_oracle as o
import lsh3_ref as r

pytestmark = pytest.mark.gpu

IDS = lambda p: '%d-%d-%g-%d' % p  # noqa: E731
KAPPAS = (1.0, 5.0, 2.0)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to('cuda', dtype=torch.float64)


def kw(params):
    return dict(zip(('tables', 'hashes', 'width', 'seed'), params))


@functools.lru_cache(maxsize=None)
def host_jobs(twice=False):
    """The host pyramids of the jobs, never modified.  Three jobs, two groups: job 0 is
    lsh3_ref.case(), job 1 has its A / A' and another B and B' seed, job 2 an A / A' of its own
    of the same shapes.  twice: two jobs over the case whose every row exists twice."""
    if twice:
        c0 = r.case(93, (12, 14), (11, 13), 1, True)
        B_pyr = r.pyr3(r.colour(197, (11, 13)))
        return c0, [(c0[0], c0[1], c0[2], c0[3]), (c0[0], c0[1], B_pyr, o.initialize_Bp(B_pyr, True, 198))], [0, 0]
    c0 = r.case()
    B_pyr = r.pyr3(r.colour(191, (28, 33)))
    j1 = (c0[0], c0[1], B_pyr, o.initialize_Bp(B_pyr, True, 192))
    j2 = r.inputs(131, (30, 40), (28, 33), n_ap=2)[:4]
    return c0, [(c0[0], c0[1], c0[2], c0[3]), j1, j2], [0, 0, 1]


def dev_jobs(twice=False):
    """Fresh device jobs: jobs of one group get the SAME A and A' pyramid tensors."""
    _, jobs, groups = host_jobs(twice)
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


@functools.lru_cache(maxsize=None)
def alone(params, debug=False, twice=False):
    """synthesize_dev(lsh=...) of every job alone, on device pyramids of its own: computed once
    per parameter set, shared by the tests, never modified."""
    import image_analogies as ia
    c0, jobs, _ = host_jobs(twice)
    res = []
    for (A_pyr, Ap_list, B_pyr, Bp_pyr), k in zip(jobs, KAPPAS):
        Bp_dev = [dev(b) for b in Bp_pyr]
        out = ia.synthesize_dev([dev(p) for p in A_pyr], [[dev(p) for p in q] for q in Ap_list],
                                [dev(p) for p in B_pyr], Bp_dev, c0[4], k, c0[6], lsh=kw(params), debug=debug)
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


def run_batch(params, debug=False, twice=False, **kwargs):
    import image_analogies as ia
    c0, host, _ = host_jobs(twice)
    jobs = dev_jobs(twice)
    outs = ia.synthesize_batch_dev(jobs, c0[4], list(KAPPAS[:len(jobs)]), c0[6], debug=debug, lsh=kw(params),
                                   **kwargs)
    return [to_host(out, job[3]) for out, job in zip(outs, jobs)]


def restatement_of(case, params):
    """level -> the restatement over the device's own centre, width and projections."""
    import algorithms
    A_pyr, Ap_list, _, _, _, As, _ = case

    def tables(level):
        index = algorithms.LevelIndex3(dev(A_pyr[level - 1]), dev(A_pyr[level]),
                                       torch.stack([dev(p[level - 1]) for p in Ap_list]),
                                       torch.stack([dev(p[level]) for p in Ap_list])).build_lsh(**kw(params))
        h = index.lsh
        return r.LshIndexD(As[level], index.center.cpu().numpy(), index.lsh_proj_host, h.L, h.k, np.float32(h.w))
    return tables


@pytest.mark.parametrize('params', r.SYNTH_PARAMS, ids=IDS)
def test_three_jobs_two_groups(gpu, params):
    """Every job's s, im and B' at every level equal its own unbatched run; job 0 (kappa 1) also
    equals the scanline oracle driven by the restatement.  A job reading another job's tables,
    centre, weights or B', or a group's width applied to the other group, shows here."""
    got = run_batch(params)
    want = alone(params)
    assert len(got) == 3
    for q in range(3):
        assert_same(got[q], want[q], 'job %d' % q)
    # the jobs do differ from one another (the comparison above is not between equal things)
    L = host_jobs()[0][4]
    assert not np.array_equal(want[0][0][L - 1][0], want[1][0][L - 1][0])
    assert not np.array_equal(want[0][0][L - 1][0], want[2][0][L - 1][0])
    c0 = host_jobs()[0]
    ref, Bp_ref, _ = r.oracle_synthesis(c0, 1.0, restatement_of(c0, params))
    out, Bp = got[0]
    for level in range(1, L):
        assert np.array_equal(out[level][0], ref[level][0]), level
        assert np.array_equal(out[level][1], ref[level][1]), level
        assert np.array_equal(Bp[level], Bp_ref[level]), level


@pytest.mark.parametrize('params', r.SYNTH_PARAMS, ids=IDS)
def test_ties_take_the_lower_row(gpu, params):
    """Two jobs sharing an A' pyramid listed twice (every row exists twice, exact ties): the
    unbatched run's results, so the (distance, row) order decides in the batch too."""
    got = run_batch(params, twice=True)
    want = alone(params, twice=True)
    for q in range(2):
        assert_same(got[q], want[q], 'job %d' % q)
    im = np.concatenate([res[1] for res in want[0][0].values()])
    assert (im == 0).mean() > 0.5     # (the lower row of a tied pair is image 0's)


def test_one_job_and_repetition(gpu):
    """K = 1 through ia_synth_levels3_lsh_batch makes the single job's run; a second call on
    fresh B' copies gives the same result (nothing is left behind in the shared state)."""
    import image_analogies as ia
    params = r.SYNTH_PARAMS[0]
    c0 = host_jobs()[0]
    want = alone(params)
    for _ in range(2):
        job = dev_jobs()[0]
        outs = ia.synthesize_batch_dev([job], c0[4], [KAPPAS[0]], c0[6], lsh=kw(params))
        assert len(outs) == 1
        assert_same(to_host(outs[0], job[3]), want[0], 'K = 1')
    first = run_batch(params)
    again = run_batch(params)
    for q in range(3):
        assert_same(again[q], first[q], 'second call, job %d' % q)
        assert_same(again[q], want[q], 'second call, job %d' % q)


def test_debug_tensors(gpu):
    params = r.SYNTH_PARAMS[0]
    got = run_batch(params, debug=True)
    want = alone(params, debug=True)
    L = host_jobs()[0][4]
    for q in range(3):
        assert len(got[q][0][L - 1]) == 3 and len(want[q][0][L - 1]) == 3
        assert_same(got[q], want[q], 'job %d' % q)
    assert got[0][0][L - 1][2][0].any()       # (the records are written)


def test_one_table_set_per_group_and_level(gpu, monkeypatch):
    """algorithms.lsh3_tables runs 2 x levels times for the three jobs of two groups, and the
    jobs of a group pass the same lsh->mem, centre and database."""
    import _ia
    import algorithms
    import image_analogies as ia
    params = r.SYNTH_PARAMS[0]
    c0 = host_jobs()[0]
    L = c0[4]
    calls = []
    real = algorithms.lsh3_tables

    def counted(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(algorithms, 'lsh3_tables', counted)
    got = run_batch(params)
    assert len(calls) == 2 * (L - 1)
    for q, w in enumerate(alone(params)):
        assert_same(got[q], w, 'job %d' % q)
    del calls[:]
    arr, _, keep = ia._batch3_lsh_args(dev_jobs(), L, list(KAPPAS), _ia.to_dev(c0[6]), False, kw(params))
    assert len(calls) == 2 * (L - 1) and len(arr) == 3 * (L - 1)
    for j in range(L - 1):
        a0, a1, a2 = arr[3 * j], arr[3 * j + 1], arr[3 * j + 2]
        assert a0.lsh.contents.mem == a1.lsh.contents.mem != a2.lsh.contents.mem
        assert a0.center == a1.center != a2.center and a0.db == a1.db != a2.db
        assert not a0.dbr and not a0.rot         # no rotated database is built
        assert len({a0.workspace, a1.workspace, a2.workspace}) == 3 and len({a0.s, a1.s, a2.s}) == 3
    del keep


def copy_struct(x):
    y = type(x)()
    ctypes.memmove(ctypes.byref(y), ctypes.byref(x), ctypes.sizeof(y))
    return y


def test_refusals_through_the_c_abi(gpu):
    """IA_E_ARG before anything is enqueued, the field named, every output keeping its fill;
    then the unchanged arguments run."""
    import _ia
    import image_analogies as ia
    lib, st = _ia.lib(), _ia.stream()
    params = r.SYNTH_PARAMS[0]
    c0 = host_jobs()[0]
    L = c0[4]
    jobs = dev_jobs()
    arr, res, keep = ia._batch3_lsh_args(jobs, L, list(KAPPAS), _ia.to_dev(c0[6]), False, kw(params))
    level = L - 1
    trio = lambda: (_ia.IaSynthArgs * 3)(*[copy_struct(a) for a in arr[3 * (L - 2):]])  # noqa: E731
    fills = []
    for q in range(3):
        s, im = res[q][level]
        s.fill_(-7)
        im.fill_(-7)
        fills.append((s, im, jobs[q][3][level], jobs[q][3][level].clone()))
    good = trio()
    other = ia._db3_level(*dev_jobs()[0][:2], level)          # job 0's rows in memory of their own
    spare = torch.zeros(168 * 64, dtype=torch.float32, device='cuda')
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
        assert lib.ia_synth_levels3_lsh_batch(sub, 1, K, st) == _ia.IA_E_ARG, what
        msg = lib.ia_last_error().decode()
        assert what in msg and msg.startswith('ia_synth_levels3_lsh_batch'), (what, msg)
        del held

    def set1(field, value):
        return lambda bad: setattr(bad[1], field, value)
    case('lsh', set1('lsh', None))
    case('center', set1('center', None))
    case('center', lambda bad: setattr(bad[0], 'center', None), K=1)
    case('comm', set1('comm', 0x1000))                       # (refused before it is looked into)
    case('differ in nrows', set1('nrows', good[1].nrows - 1))
    case('row0', lambda bad: [setattr(b, 'nrows', b.nrows - 1) for b in bad])
    case('row0', lambda bad: setattr(bad[0], 'row0', 1), K=1)
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
    case('sharing lsh->mem differ in db', set1('db', _ia.ptr(other[6]).value))
    case('sharing lsh->mem differ in src.Ap_lg', lambda bad: setattr(bad[1].src, 'Ap_lg', _ia.ptr(other[3]).value))
    case('L*k', lambda bad: [lsh_with(b, L=13, k=5) for b in bad])
    case('16-byte aligned', lambda bad: lsh_with(bad[2], proj=good[2].lsh.contents.proj + 4))
    for K in (0, 129):
        assert lib.ia_synth_levels3_lsh_batch(good, 1, K, st) == _ia.IA_E_ARG
        assert 'K out of range' in lib.ia_last_error().decode()
    # the exact batch entry still refuses an lsh, and names the LSH entry
    assert lib.ia_synth_levels3_batch(good, 1, 3, st) == _ia.IA_E_ARG
    assert 'lsh' in lib.ia_last_error().decode()
    torch.cuda.synchronize()
    for s, im, bp, bp0 in fills:
        assert bool((s == -7).all()) and bool((im == -7).all()) and torch.equal(bp, bp0)
    assert lib.ia_synth_levels3_lsh_batch(good, 1, 3, st) == 0
    assert lib.ia_synth3_status(good, 3, st) == 0
    for s, im, bp, bp0 in fills:
        assert not bool((s == -7).any()) and not bool((im == -7).any()) and not torch.equal(bp, bp0)
    del keep


def test_multi_main_files(gpu, monkeypatch, tmp_path):
    """multi_main(batch=3) on three small colour files under c.matcher = 'lsh' with
    convert=False (runs 0 and 1 name one A / A' pair): ONE synthesize_batch_dev call carrying
    the lsh, files byte-identical to the unbatched loop's; none with IA_LSH_BATCH=0."""
    from PIL import Image
    from scipy.ndimage import gaussian_filter
    import algorithms
    import config
    import image_analogies as ia

    def png(name, img):
        path = str(tmp_path / (name + '.png'))
        Image.fromarray(np.clip(np.round(img * 255), 0, 255).astype(np.uint8), 'RGB').save(path)
        return path
    A = r.colour(571, (26, 30))
    fA = png('A', A)
    fAp = png('Ap', np.dstack([gaussian_filter(A[..., ch], 1.2) for ch in range(3)]))
    fAp2 = png('Ap2', np.dstack([gaussian_filter(A[..., ch], 2.0) for ch in range(3)]))
    fB = [png('B%d' % i, r.colour(572 + i, (24, 20))) for i in range(3)]
    ks = [1.0, 6.0, 0.5]
    old = config.matcher

    def fresh():
        config.convert, config.remap_lum, config.init_rand, config.AB_weight = False, False, True, 1
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
        monkeypatch.setitem(ia.LSH_BATCH_DEFAULT, True, 1)
        got = ia.multi_main(runs('b'), fresh(), rank=0, world=1, batch=3)
        assert spied == [(3, algorithms.lsh_params(config))] and spied[0][1] is not None
        del spied[:]
        monkeypatch.setenv('IA_LSH_BATCH', '0')
        off = ia.multi_main(runs('o'), fresh(), rank=0, world=1, batch=3)
        assert spied == []
        ref = ia.multi_main(runs('u'), fresh(), rank=0, world=1)
        assert spied == []
    finally:
        config.matcher = old
    L = len(ref[0])
    assert sorted(got) == sorted(off) == sorted(ref) == [0, 1, 2]
    for j in ref:
        for x, y, z in zip(got[j], off[j], ref[j]):
            assert np.array_equal(x, z) and np.array_equal(y, z), j
        names = sorted(os.path.basename(p) for p in glob.glob(str(tmp_path / ('u%d' % j) / '*.jpg')))
        assert len(names) == L
        for n in names:
            want = (tmp_path / ('u%d' % j) / n).read_bytes()
            for tag in 'bo':
                assert (tmp_path / ('%s%d' % (tag, j)) / n.replace('u%d' % j, '%s%d' % (tag, j))).read_bytes() == want, \
                    (tag, j, n)
