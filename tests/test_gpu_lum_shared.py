"""Luminance batches whose jobs share A and A' (DB groups: one algorithms.level_index per group
and level, one k_screen16rs launch per wave of a level with a rotated database) against the C
oracle's scanline run of every job, the forced K-job screen (k_screen16r), separate
synthesize_dev calls, multi_main's unbatched loop and the C-ABI's refusals.

The C oracle returns B', s and im; the debug records are compared with a separate
synthesize_dev call on the same inputs (whose records test_gpu_parity.py holds to the oracle)."""
import ctypes
import functools
import glob
import os

import numpy as np
import pytest
import torch

import ia_oracle as o
import ia_oracle_c as oc
from conftest import smooth_noise

pytestmark = pytest.mark.gpu

KAPPAS = (0.5, 5.0, 25.0, 1.0)
X, Y, Z = 700, 740, 780          # (A, A') seeds


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to('cuda', dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def a_images(a_seed, A_shape, n_ap):
    from scipy.ndimage import gaussian_filter
    A = smooth_noise(a_seed, A_shape)
    return A, tuple(gaussian_filter(A, 1.0 + 0.5 * i) for i in range(n_ap))


@functools.lru_cache(maxsize=None)
def job_reference(a_seed, b_seed, A_shape, B_shape, n_ap, k, cap=None):
    """One job (A, A' from a_seed; B and the B' init from b_seed) and the C oracle's scanline
    run of it: computed once, shared by every case, never modified.
    Returns (A_pyr, Ap_list, B_pyr, Bp_pyr, L, w, ref)."""
    A, Aps = a_images(a_seed, A_shape, n_ap)
    B = smooth_noise(b_seed + 1, B_shape)
    A_pyr, Ap_list, B_pyr, Bp_pyr, L = o.setup_luminance(A, list(Aps), B, cap=cap, seed=b_seed + 2)
    w = o.compute_weights(3, 5, 12, 1)
    ref = oc.synthesize(A_pyr, Ap_list, B_pyr, [b.copy() for b in Bp_pyr], L, k, w)
    return A_pyr, Ap_list, B_pyr, Bp_pyr, L, w, ref


def dev_jobs(cases, a_seeds):
    """Device jobs of the cases: jobs of one a_seed get the SAME A and A' pyramid tensors, after
    the check that their pyramids are equal arrays."""
    sides, first = {}, {}
    jobs = []
    for case, a_seed in zip(cases, a_seeds):
        if a_seed not in sides:
            sides[a_seed] = ([dev(p) for p in case[0]], [[dev(p) for p in q] for q in case[1]])
            first[a_seed] = case
        else:
            f = first[a_seed]
            assert len(f[0]) == len(case[0]) and len(f[1]) == len(case[1])
            assert all(np.array_equal(x, y) for x, y in zip(f[0], case[0]))
            assert all(np.array_equal(x, y) for p, q in zip(f[1], case[1]) for x, y in zip(p, q))
        jobs.append(sides[a_seed] + ([dev(p) for p in case[2]], [dev(b) for b in case[3]]))
    return jobs


def own_job(case):
    return ([dev(p) for p in case[0]], [[dev(p) for p in q] for q in case[1]], [dev(p) for p in case[2]],
            [dev(b) for b in case[3]])


def assert_job_equals_oracle(case, job, out, tag):
    L, ref = case[4], case[6]
    assert sorted(out) == list(range(1, L)), tag
    for level in range(1, L):
        assert np.array_equal(out[level][0].cpu().numpy(), ref[level][1]), (tag, level, 's')
        assert np.array_equal(out[level][1].cpu().numpy(), ref[level][2]), (tag, level, 'im')
        assert np.array_equal(job[3][level].cpu().numpy(), ref[level][0]), (tag, level, "B'")


def same_results(a, b):
    assert sorted(a) == sorted(b)
    for level in a:
        assert len(a[level]) == len(b[level])
        for x, y in zip(a[level], b[level]):
            if isinstance(x, tuple):
                assert all(torch.equal(p, q) for p, q in zip(x, y)), level
            else:
                assert torch.equal(x, y), level


def assert_job_equals_separate_call(ia, case, k, job, out, tag):
    alone = own_job(case)
    ref = ia.synthesize_dev(*alone, case[4], k, case[5], debug=True)
    same_results(out, ref)
    assert all(torch.equal(x, y) for x, y in zip(job[3], alone[3])), tag


@pytest.fixture
def shared(monkeypatch):
    """Every level on the rotated screen (IA_ROT_MIN_ROWS=0, IA_DB_ROT at its default) and the
    shared screen on; yields the switch, everything restored afterwards."""
    import _ia
    lib = _ia.lib()
    monkeypatch.setenv('IA_ROT_MIN_ROWS', '0')
    monkeypatch.delenv('IA_DB_ROT', raising=False)
    monkeypatch.delenv('IA_BATCH_CHUNKS', raising=False)
    prev = lib.ia_diag_set_shared_screen(1)
    yield lib.ia_diag_set_shared_screen
    lib.ia_diag_set_shared_screen(prev)


def count_indexes(monkeypatch):
    """A counting wrapper around algorithms.level_index: [(A' data_ptr, level, has dbr)]."""
    import algorithms
    calls = []
    level_index = algorithms.level_index

    def counted(A_pyr, Ap_pyr_list, level, *a, **kw):
        idx = level_index(A_pyr, Ap_pyr_list, level, *a, **kw)
        calls.append((Ap_pyr_list[0][-1].data_ptr(), level, getattr(idx, 'dbr', None) is not None))
        return idx
    monkeypatch.setattr(algorithms, 'level_index', counted)
    return calls


def nonempty_waves(B_pyr, L):
    """Waves with at least one query over levels 1 .. L - 1."""
    import _ia
    lib = _ia.lib()
    out = (ctypes.c_int * 5)()
    n = 0
    for level in range(1, L):
        H, W = B_pyr[level].shape
        for t in range((W - 1) + 3 * (H - 1) + 1):
            assert lib.ia_diag_wave_rows(H, W, t, 0, 0, out) == 0
            n += out[1] > 0
    return n


def four_jobs(n_ap):
    return [job_reference(X + n_ap, 400 + 5 * q, (36, 44), (30, 41), n_ap, k) for q, k in enumerate(KAPPAS)]


@pytest.mark.parametrize('n_ap', [1, 2])
def test_four_jobs_one_database(gpu, shared, monkeypatch, n_ap):
    """Four jobs with one (A, A') (A 36 x 44, B 30 x 41, every level on the rotated screen;
    distinct B, B' inits and kappas 0.5 / 5 / 25 / 1), debug on, one and two A' images: every
    job's B', s and im equal its oracle run and, with the debug records, a separate
    synthesize_dev call; level_index runs L - 1 times (4 (L - 1) without sharing) and every
    non-empty wave of every level is one k_screen16rs launch."""
    import _ia
    import image_analogies as ia
    cases = four_jobs(n_ap)
    L = cases[0][4]
    jobs = dev_jobs(cases, [X] * 4)
    assert ia.db_groups(jobs) == [0, 0, 0, 0]
    with monkeypatch.context() as mp:
        calls = count_indexes(mp)
        before = _ia.lib().ia_diag_shared_screen_waves()
        outs = ia.synthesize_batch_dev(jobs, L, list(KAPPAS), cases[0][5], debug=True)
        after = _ia.lib().ia_diag_shared_screen_waves()
    assert len(calls) == L - 1 and all(c[2] for c in calls), calls
    assert after - before == nonempty_waves(cases[0][2], L)
    assert len(outs) == 4
    for q, (case, job, out) in enumerate(zip(cases, jobs, outs)):
        assert_job_equals_oracle(case, job, out, q)
        assert_job_equals_separate_call(ia, case, KAPPAS[q], job, out, q)


def test_query_group_boundary_inside_a_job(gpu, shared):
    """Seven jobs of one group with B 40 x 100: waves of up to 34 queries, T = 2 with a padded
    second tile: 14 tiles in two query groups of 7, the first ending with job 3's first tile and
    the second beginning with its padded one."""
    import image_analogies as ia
    ks = [1.0, 8.0, 0.5, 25.0, 3.0, 0.25, 12.0]
    cases = [job_reference(X + 1, 440 + 7 * q, (36, 44), (40, 100), 1, k) for q, k in enumerate(ks)]
    assert max(min(b.shape[0], (b.shape[1] + 2) // 3) for b in cases[0][2]) == 34
    jobs = dev_jobs(cases, [X] * 7)
    outs = ia.synthesize_batch_dev(jobs, cases[0][4], ks, cases[0][5])
    for q, (case, job, out) in enumerate(zip(cases, jobs, outs)):
        assert_job_equals_oracle(case, job, out, q)


def test_more_than_eleven_tiles_of_one_each(gpu, shared):
    """Twelve jobs of one group with B 30 x 34 (T = 1): 12 tiles in two query groups of 6."""
    import image_analogies as ia
    ks = [0.5 + 1.5 * q for q in range(12)]
    cases = [job_reference(X + 1, 480 + 5 * q, (36, 44), (30, 34), 1, k) for q, k in enumerate(ks)]
    jobs = dev_jobs(cases, [X] * 12)
    outs = ia.synthesize_batch_dev(jobs, cases[0][4], ks, cases[0][5])
    for q, (case, job, out) in enumerate(zip(cases, jobs, outs)):
        assert_job_equals_oracle(case, job, out, q)


def test_strip_order_level(gpu, shared):
    """A 256 x 256 under a 3-level cap: the finest level's 65,536 rows lie in strip order (the
    stage map's other branch); B 33 x 47, three jobs of one group."""
    import _ia
    import image_analogies as ia
    ks = [0.5, 4.0, 20.0]
    cases = [job_reference(X + 3, 560 + 3 * q, (256, 256), (33, 47), 1, k, 3) for q, k in enumerate(ks)]
    L = cases[0][4]
    assert L == 4 and cases[0][0][L - 1].shape == (256, 256)
    jobs = dev_jobs(cases, [X] * 3)
    before = _ia.lib().ia_diag_shared_screen_waves()
    outs = ia.synthesize_batch_dev(jobs, L, ks, cases[0][5])
    assert _ia.lib().ia_diag_shared_screen_waves() - before == nonempty_waves(cases[0][2], L)
    for q, (case, job, out) in enumerate(zip(cases, jobs, outs)):
        assert_job_equals_oracle(case, job, out, q)


def mixed_cases():
    ks = [0.5, 3.0, 25.0, 1.0, 5.0, 9.0]
    four = four_jobs(1)
    cases = [four[0], job_reference(Y + 1, 520, (36, 44), (30, 41), 1, ks[1]), four[2],
             job_reference(Y + 1, 525, (36, 44), (30, 41), 1, ks[3]), four[1],
             job_reference(Z + 1, 530, (36, 44), (30, 41), 1, ks[5])]
    return cases, [KAPPAS[0], ks[1], KAPPAS[2], ks[3], KAPPAS[1], ks[5]]


def test_mixed_groups_interleaved(gpu, shared, monkeypatch):
    """Six jobs X, Y, X, Y, X, Z by their (A, A'): groups of 3, 2 and 1 in interleaved order.
    ia_batch_groups on the finest level's real argument array returns [0, 1, 0, 1, 0, 2]; one
    index per group and level; every job equals its oracle run (the singleton group goes through
    the same launch)."""
    import _ia
    import algorithms
    import image_analogies as ia
    seeds = [X, Y, X, Y, X, Z]
    cases, ks = mixed_cases()
    L, w = cases[0][4], cases[0][5]
    jobs = dev_jobs(cases, seeds)
    assert ia.db_groups(jobs) == [0, 1, 0, 1, 0, 2]
    # the finest level's argument array as synthesize_batch_dev forms it
    probe = dev_jobs(cases, seeds)
    wd = _ia.to_dev(w)
    idx = {}
    finest = []
    for q, (A_pyr, Ap_list, B_pyr, Bp_pyr) in enumerate(probe):
        g = ia.db_groups(probe)[q]
        if g not in idx:
            idx[g] = algorithms.level_index(A_pyr, Ap_list, L - 1, None, None)
        finest.append(ia._LevelCall(L - 1, L, idx[g], B_pyr[L - 2], B_pyr[L - 1], Bp_pyr[L - 2], Bp_pyr[L - 1],
                                    wd, ks[q]))
    arr = (_ia.IaSynthArgs * 6)(*[c.args for c in finest])
    grp = (ctypes.c_int * 6)()
    assert arr[0].dbr and _ia.lib().ia_batch_groups(arr, 6, grp) == 3
    assert list(grp) == [0, 1, 0, 1, 0, 2]
    del finest, idx
    with monkeypatch.context() as mp:
        calls = count_indexes(mp)
        outs = ia.synthesize_batch_dev(jobs, L, ks, w)
    assert len(calls) == 3 * (L - 1), calls
    assert [c[1] for c in calls] == [level for level in range(1, L) for _ in range(3)]
    for q, (case, job, out) in enumerate(zip(cases, jobs, outs)):
        assert_job_equals_oracle(case, job, out, q)


def test_switch_off_equals_default(gpu, shared):
    """The four-job batch with ia_diag_set_shared_screen(0) (every job through the K-job
    k_screen16r over the one shared database): torch.equal to the default on every output, and
    the shared-wave counter does not move."""
    import _ia
    import image_analogies as ia
    cases = four_jobs(1)
    L, w = cases[0][4], cases[0][5]
    a, b = dev_jobs(cases, [X] * 4), dev_jobs(cases, [X] * 4)
    assert shared(-1) == 1
    out_a = ia.synthesize_batch_dev(a, L, list(KAPPAS), w, debug=True)
    assert shared(0) == 1
    before = _ia.lib().ia_diag_shared_screen_waves()
    out_b = ia.synthesize_batch_dev(b, L, list(KAPPAS), w, debug=True)
    assert _ia.lib().ia_diag_shared_screen_waves() == before
    assert shared(1) == 0
    for q in range(4):
        same_results(out_a[q], out_b[q])
        assert all(torch.equal(x, y) for x, y in zip(a[q][3], b[q][3]))
        assert_job_equals_oracle(cases[q], b[q], out_b[q], q)


def test_repeated_shared_batch(gpu, shared):
    """The same shared batch twice on one thread: equal results (job and group tables re-staged,
    tickets and granules re-initialised), the second equal to the oracle."""
    import image_analogies as ia
    cases = four_jobs(1)
    L, w = cases[0][4], cases[0][5]
    first, second = dev_jobs(cases, [X] * 4), dev_jobs(cases, [X] * 4)
    out1 = ia.synthesize_batch_dev(first, L, list(KAPPAS), w, debug=True)
    out2 = ia.synthesize_batch_dev(second, L, list(KAPPAS), w, debug=True)
    for q in range(4):
        same_results(out1[q], out2[q])
        assert all(torch.equal(x, y) for x, y in zip(first[q][3], second[q][3]))
        assert_job_equals_oracle(cases[q], second[q], out2[q], q)


def test_default_thresholds_share_the_database_only(gpu, shared, monkeypatch):
    """Without IA_ROT_MIN_ROWS no level of the four-job batch reaches rot_min_rows(): L - 1
    indexes (shared all the same), the split-f16 screen's launches as before (the shared-wave
    counter does not move), the oracle's results."""
    import _ia
    import image_analogies as ia
    monkeypatch.delenv('IA_ROT_MIN_ROWS')
    cases = four_jobs(1)
    L = cases[0][4]
    jobs = dev_jobs(cases, [X] * 4)
    with monkeypatch.context() as mp:
        calls = count_indexes(mp)
        before = _ia.lib().ia_diag_shared_screen_waves()
        outs = ia.synthesize_batch_dev(jobs, L, list(KAPPAS), cases[0][5], debug=True)
        assert _ia.lib().ia_diag_shared_screen_waves() == before
    assert len(calls) == L - 1 and not any(c[2] for c in calls), calls
    for q, (case, job, out) in enumerate(zip(cases, jobs, outs)):
        assert_job_equals_oracle(case, job, out, q)


def test_refusals_of_half_shared_jobs(gpu, shared):
    """Two jobs passing one dbr but another center, amax, rot or db: IA_E_ARG naming the field,
    before anything is launched (every output keeps its fill); the untouched pair then runs."""
    import _ia
    import algorithms
    import image_analogies as ia
    lib, st = _ia.lib(), _ia.stream()
    cases = four_jobs(1)[:2]
    L, w = cases[0][4], _ia.to_dev(cases[0][5])
    level = L - 1
    jobs = dev_jobs(cases, [X] * 2)
    index = algorithms.level_index(jobs[0][0], jobs[0][1], level, None, None, rows=True)
    # a second index of the same contents in memory of its own
    other = algorithms.level_index(*own_job(cases[0])[:2], level, None, None, rows=True)
    calls = [ia._LevelCall(level, L, index, B[level - 1], B[level], Bp[level - 1], Bp[level], w, k)
             for (_, _, B, Bp), k in zip(jobs, KAPPAS)]
    pair = lambda: (_ia.IaSynthArgs * 2)(*[c.args for c in calls])  # noqa: E731
    good = pair()
    assert good[0].dbr and good[0].dbr == good[1].dbr and good[0].db and good[0].db == good[1].db
    fills = []
    for c, job in zip(calls, jobs):
        c.s.fill_(-7)
        c.im.fill_(-7)
        fills.append((c.s, c.im, job[3][level], job[3][level].clone()))
    for field, value in (('center', other.center), ('amax', other.amax), ('rot', other.rot), ('db', other.db)):
        bad = pair()
        setattr(bad[1], field, _ia.ptr(value).value)
        assert lib.ia_synth_levels_batch(bad, 1, 2, st) == _ia.IA_E_ARG, field
        assert lib.ia_last_error().decode().endswith('jobs sharing a database differ in ' + field)
    torch.cuda.synchronize()
    for s, im, bp, bp0 in fills:
        assert bool((s == -7).all()) and bool((im == -7).all()) and torch.equal(bp, bp0)
    assert lib.ia_synth_levels_batch(good, 1, 2, st) == 0
    assert lib.ia_synth_status(good, 2, st) == 0
    assert not bool((fills[0][0] == -7).any()) and not bool((fills[1][0] == -7).any())
    del other


def test_profile_counts_pairs_as_unshared(gpu, shared):
    """prof=True: a shared batch's records carry the pairs, jobs and screen launches of the same
    jobs under switch 0 (a shared wave counts as one screen launch)."""
    import _ia
    import image_analogies as ia
    cases = four_jobs(1)
    L, w = cases[0][4], cases[0][5]
    recs = []
    for on in (1, 0):
        shared(on)
        jobs = dev_jobs(cases, [X] * 4)
        _ia.prof_begin()
        try:
            ia.synthesize_batch_dev(jobs, L, list(KAPPAS), w, prof=True)
        finally:
            recs.append(_ia.prof_end())
    shared(1)
    assert len(recs[0]) == len(recs[1]) == L - 1
    for a, b in zip(*recs):
        assert a['pairs'] == b['pairs'] > 0 and a['jobs'] == b['jobs'] == 4
        assert a['level'] == b['level'] and a['rows'] == b['rows']
        assert a['timed_screens'] == b['timed_screens'] > 0


def test_multi_main_shares_the_runs_of_one_a_pair(gpu, monkeypatch, tmp_path):
    """multi_main(batch=5) with convert=True on five runs from colour PNGs: four name the same A
    and A' files (distinct B files and kappas), the fifth another A' file.  Two DB groups by
    build count; every B' pyramid and every level_*_color.jpg equals the unbatched loop's.  The
    same four runs under remap_lum (A depends on B) form four groups and still equal the loop."""
    from PIL import Image
    import config
    import image_analogies as ia
    from scipy.ndimage import gaussian_filter
    monkeypatch.delenv('IA_BATCH_CHUNKS', raising=False)

    def colour(seed, shape):
        return np.dstack([smooth_noise(seed + 17 * ch, shape) for ch in range(3)])

    def png(name, img):
        path = str(tmp_path / (name + '.png'))
        Image.fromarray(np.clip(np.round(img * 255), 0, 255).astype(np.uint8), 'RGB').save(path)
        return path
    A = colour(761, (32, 40))
    fA = png('A', A)
    fAp = png('Ap', np.dstack([gaussian_filter(A[..., ch], 1.2) for ch in range(3)]))
    fAp2 = png('Ap2', np.dstack([gaussian_filter(A[..., ch], 2.0) for ch in range(3)]))
    fB = [png('B%d' % i, colour(762 + i, (30, 36))) for i in range(5)]
    ks = [2.0, 11.0, 0.5, 25.0, 4.0]

    def fresh(remap):
        config.convert, config.remap_lum, config.init_rand, config.AB_weight = True, remap, True, 1
        config.k, config.seed, config.levels, config.matcher = 2.0, 9, None, 'brute'
        return config

    def runs(tag, n):
        d = lambda i: str(tmp_path / ('%s%d' % (tag, i))) + '/'  # noqa: E731
        return [(fA, [fAp if i < 4 else fAp2], fB[i], d(i), {'k': ks[i]}) for i in range(n)]

    def compare(tag_b, tag_u, n, remap, groups):
        with monkeypatch.context() as mp:
            calls = count_indexes(mp)
            got = ia.multi_main(runs(tag_b, n), fresh(remap), rank=0, world=1, batch=5)
        L = len(got[0])
        per_group = {}
        for key, level, _ in calls:
            per_group.setdefault(key, []).append(level)
        assert sorted(sorted(v) for v in per_group.values()) == [list(range(1, L))] * groups, calls
        ref = ia.multi_main(runs(tag_u, n), fresh(remap), rank=0, world=1)
        assert sorted(got) == sorted(ref) == list(range(n))
        for j in ref:
            assert len(got[j]) == len(ref[j])
            for x, y in zip(got[j], ref[j]):
                assert np.array_equal(x, y), j
            names = sorted(os.path.basename(p) for p in glob.glob(str(tmp_path / ('%s%d' % (tag_u, j)) / 'level_*_color.jpg')))
            assert len(names) >= L - 1
            for name in names:
                assert (tmp_path / ('%s%d' % (tag_b, j)) / name).read_bytes() == \
                    (tmp_path / ('%s%d' % (tag_u, j)) / name).read_bytes(), (j, name)
    compare('b', 'u', 5, False, 2)
    compare('rb', 'ru', 4, True, 4)
