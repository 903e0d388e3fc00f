"""Colour batches whose jobs share A and A' (DB groups: one ia_db3_build, one rotated database
and one k_screen3rs pass per group and level) against the numpy oracle's scanline run of every
job, the forced unshared screen (k_screen3rb), separate synthesize_dev calls, multi_main's
unbatched loop, the C-ABI's refusals and the build's resource reports."""
import ctypes
import functools
import glob
import hashlib
import os
import re

import numpy as np
import pytest
import torch

import ia_oracle as o
from conftest import ROOT, smooth_noise

pytestmark = pytest.mark.gpu

KAPPAS = (0.5, 5.0, 25.0, 1.0)
A_SHAPE = (36, 44)
X, Y, Z = 300, 340, 380          # (A, A') seeds


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to('cuda', dtype=torch.float64)


def colour(seed, shape):
    """A smooth colour image (h, w, 3) in [0, 1]: three differently seeded channels."""
    return np.dstack([smooth_noise(seed + 17 * ch, shape) for ch in range(3)])


def pyr3(img):
    """Per-channel oracle pyramids stacked (skimage multichannel=True semantics)."""
    chans = [o.compute_gaussian_pyramid(img[..., ch], 3, None) for ch in range(3)]
    return [np.dstack([c[l] for c in chans]) for l in range(len(chans[0]))]


@functools.lru_cache(maxsize=None)
def a_side(a_seed, n_ap):
    """A and its A' images from one seed: (A_pyr, Ap_list), shared by every job of the seed."""
    from scipy.ndimage import gaussian_filter
    A = colour(a_seed, A_SHAPE)
    Aps = [np.dstack([gaussian_filter(A[..., ch], 1.0 + 0.5 * i) for ch in range(3)]) for i in range(n_ap)]
    return pyr3(A), [pyr3(x) for x in Aps]


@functools.lru_cache(maxsize=None)
def a_index(a_seed, n_ap, L):
    A_pyr, Ap_list = a_side(a_seed, n_ap)
    return o.create_index(A_pyr, Ap_list, L)


@functools.lru_cache(maxsize=None)
def job_reference(a_seed, b_seed, B_shape, n_ap, k):
    """One job (A, A' from a_seed; B and the B' init from b_seed) and the oracle's scanline run
    of it with the debug lists: computed once, shared by every case, never modified."""
    A_pyr, Ap_list = a_side(a_seed, n_ap)
    B_pyr = pyr3(colour(b_seed + 1, B_shape))
    L = min(len(A_pyr), len(B_pyr))
    Bp_pyr = o.initialize_Bp(B_pyr, True, b_seed + 2)
    w = o.compute_weights(3, 5, 12, 3)
    As = a_index(a_seed, n_ap, L)
    Bp_ref = [b.copy() for b in Bp_pyr]
    ref = {}
    for level in range(1, L):
        dbg = {}
        s, im = o.synthesize_level(level, L, A_pyr, Ap_list, B_pyr, Bp_ref, As[level], w, k, debug=dbg)
        ref[level] = (s, im, dbg)
    return A_pyr, Ap_list, B_pyr, Bp_pyr, L, w, Bp_ref, ref


def dev_jobs(cases, a_seeds):
    """Device jobs of the cases: jobs of one a_seed get the SAME A and A' pyramid tensors."""
    sides = {}
    jobs = []
    for case, a_seed in zip(cases, a_seeds):
        if a_seed not in sides:
            sides[a_seed] = ([dev(p) for p in case[0]], [[dev(p) for p in q] for q in case[1]])
        jobs.append(sides[a_seed] + ([dev(p) for p in case[2]], [dev(b) for b in case[3]]))
    return jobs


def own_job(case):
    return ([dev(p) for p in case[0]], [[dev(p) for p in q] for q in case[1]], [dev(p) for p in case[2]],
            [dev(b) for b in case[3]])


def assert_job_equals_oracle(ia, case, job, out, tag):
    L, Bp_ref, ref = case[4], case[6], case[7]
    assert sorted(out) == list(range(1, L)), tag
    for level in range(1, L):
        s, im, dbg = out[level]
        rs, rim, rd = ref[level]
        assert np.array_equal(s.cpu().numpy(), rs), (tag, level)
        assert np.array_equal(im.cpu().numpy(), rim), (tag, level)
        assert np.array_equal(job[3][level].cpu().numpy(), Bp_ref[level]), (tag, level)
        rec = ia.debug_record(s, im, dbg, Bp_ref[level].shape[:2])
        for key in ('sa', 'sc', 'rstars'):
            assert rec[key] == rd[key], (tag, level, key)
        assert np.array_equal(rec['app_dist'], rd['app_dist']), (tag, level)
        assert np.array_equal(rec['coh_dist'], rd['coh_dist']), (tag, level)


def same_results(a, b):
    assert sorted(a) == sorted(b)
    for level in a:
        assert len(a[level]) == len(b[level])
        for x, y in zip(a[level], b[level]):
            if isinstance(x, tuple):
                assert all(torch.equal(p, q) for p, q in zip(x, y)), level
            else:
                assert torch.equal(x, y), level


@pytest.fixture
def shared(monkeypatch):
    """The screened matcher, the rotated DB and the fused tail at their defaults, whatever the
    environment says; yields the shared-screen knob, restored afterwards."""
    import _ia
    lib = _ia.lib()
    for var in ('IA_DB_ROT', 'IA_C3_FUSE', 'IA_ROT3_BATCH_SHARED'):
        monkeypatch.delenv(var, raising=False)
    prev16 = lib.ia_diag_set_color16(1)
    prev = lib.ia_diag_set_c3_shared_screen(1)
    yield lib.ia_diag_set_c3_shared_screen
    lib.ia_diag_set_c3_shared_screen(prev)
    lib.ia_diag_set_color16(prev16)


def count_builds(monkeypatch, ia):
    """Counting wrappers around the database build and the rotated build."""
    import algorithms
    calls = {'db3': [], 'rot': 0}
    db3_level, rot3_apply = ia._db3_level, algorithms.rot3_apply

    def counted_db3(A_pyr, Ap_pyr_list, level, *a, **kw):
        calls['db3'].append((Ap_pyr_list[0][-1].data_ptr(), level))
        return db3_level(A_pyr, Ap_pyr_list, level, *a, **kw)

    def counted_rot(*a, **kw):
        calls['rot'] += 1
        return rot3_apply(*a, **kw)
    monkeypatch.setattr(ia, '_db3_level', counted_db3)
    monkeypatch.setattr(algorithms, 'rot3_apply', counted_rot)
    return calls


def four_jobs(n_ap):
    return [job_reference(X + n_ap, 400 + 5 * q, (30, 34), n_ap, k) for q, k in enumerate(KAPPAS)]


@pytest.mark.parametrize('fuse', ['1', '0'])
@pytest.mark.parametrize('n_ap', [1, 2])
def test_four_jobs_one_database(gpu, shared, monkeypatch, n_ap, fuse):
    """Four jobs with one (A, A') (A 36 x 44, B 30 x 34, every level; distinct B, B' inits and
    kappas 0.5 / 5 / 25 / 1) in one synthesize_batch_dev call with debug: every job equals its
    own oracle run bit for bit (B', s, im, sa / sc / rstars, both distance maps), with the fused
    tail and without, with one and two A' images; the database and the rotated database are
    built once per level (L - 1 calls each; 4 (L - 1) without sharing)."""
    import image_analogies as ia
    monkeypatch.setenv('IA_C3_FUSE', fuse)
    cases = four_jobs(n_ap)
    L = cases[0][4]
    jobs = dev_jobs(cases, [X] * 4)
    assert ia.db_groups(jobs) == [0, 0, 0, 0]
    calls = count_builds(monkeypatch, ia)
    outs = ia.synthesize_batch_dev(jobs, L, list(KAPPAS), cases[0][5], debug=True)
    assert len(calls['db3']) == L - 1 and calls['rot'] == L - 1, calls
    assert len(outs) == 4
    for q, (case, job, out) in enumerate(zip(cases, jobs, outs)):
        assert_job_equals_oracle(ia, case, job, out, q)


def test_query_group_boundary_two_tiles_per_job(gpu, shared):
    """Four jobs of one group with B 40 x 100: waves of up to 34 queries, QT = 2 with a padded
    second tile, so the finest level's list has 8 entries, more than one workgroup stages (7):
    two query groups, each with tiles of two jobs; the coarser levels (QT = 1) have 4."""
    import image_analogies as ia
    ks = [1.0, 8.0, 0.5, 25.0]
    cases = [job_reference(X + 1, 440 + 7 * q, (40, 100), 1, k) for q, k in enumerate(ks)]
    assert max(min(b.shape[0], (b.shape[1] + 2) // 3) for b in cases[0][2]) == 34
    jobs = dev_jobs(cases, [X] * 4)
    outs = ia.synthesize_batch_dev(jobs, cases[0][4], ks, cases[0][5], debug=True)
    for q, (case, job, out) in enumerate(zip(cases, jobs, outs)):
        assert_job_equals_oracle(ia, case, job, out, q)


def test_query_group_boundary_inside_a_job(gpu, shared):
    """Five jobs of one group with B 40 x 100: 10 entries at the finest level, two query groups
    of 5 (an odd number of staged tiles), the first ending with job 2's first tile and the
    second beginning with its padded second one."""
    import image_analogies as ia
    ks = [1.0, 8.0, 0.5, 25.0, 3.0]
    cases = [job_reference(X + 1, 440 + 7 * q, (40, 100), 1, k) for q, k in enumerate(ks)]
    jobs = dev_jobs(cases, [X] * 5)
    outs = ia.synthesize_batch_dev(jobs, cases[0][4], ks, cases[0][5], debug=True)
    for q, (case, job, out) in enumerate(zip(cases, jobs, outs)):
        assert_job_equals_oracle(ia, case, job, out, q)


def test_query_group_boundary_eight_jobs(gpu, shared):
    """Eight jobs of one group with B 30 x 34 (QT = 1): 8 entries in two query groups."""
    import image_analogies as ia
    ks = list(KAPPAS) + [2.0, 11.0, 0.25, 50.0]
    cases = four_jobs(1) + [job_reference(X + 1, 480 + 5 * q, (30, 34), 1, k) for q, k in enumerate(ks[4:])]
    jobs = dev_jobs(cases, [X] * 8)
    outs = ia.synthesize_batch_dev(jobs, cases[0][4], ks, cases[0][5], debug=True)
    for q, (case, job, out) in enumerate(zip(cases, jobs, outs)):
        assert_job_equals_oracle(ia, case, job, out, q)


def test_mixed_groups_interleaved(gpu, shared, monkeypatch):
    """Six jobs X, Y, X, Y, X, Z by their (A, A'): groups of 3, 2 and 1 in interleaved order
    (G = 3 < K = 6).  ia_batch3_groups on the finest level's real argument array returns
    [0, 1, 0, 1, 0, 2]; one database per group and level; every job equals its oracle run."""
    import _ia
    import image_analogies as ia
    seeds = [X, Y, X, Y, X, Z]
    ks = [0.5, 3.0, 25.0, 1.0, 5.0, 9.0]
    four = four_jobs(1)
    cases = [four[0], job_reference(Y + 1, 520, (30, 34), 1, ks[1]), four[2],
             job_reference(Y + 1, 525, (30, 34), 1, ks[3]), four[1],
             job_reference(Z + 1, 530, (30, 34), 1, ks[5])]
    L, w = cases[0][4], cases[0][5]
    jobs = dev_jobs(cases, seeds)
    assert ia.db_groups(jobs) == [0, 1, 0, 1, 0, 2]
    probe = dev_jobs(cases, seeds)
    arr, _, keep = ia._batch3_args(probe, L, ks, _ia.to_dev(w), False, True)
    assert len(arr) == 6 * (L - 1)
    finest = (_ia.IaSynthArgs * 6)(*arr[6 * (L - 2):])
    grp = (ctypes.c_int * 6)()
    assert _ia.lib().ia_batch3_groups(finest, 6, grp) == 3
    assert list(grp) == [0, 1, 0, 1, 0, 2]
    del keep
    calls = count_builds(monkeypatch, ia)
    outs = ia.synthesize_batch_dev(jobs, L, ks, w, debug=True)
    assert len(calls['db3']) == 3 * (L - 1) and calls['rot'] == 3 * (L - 1), calls
    for q, (case, job, out) in enumerate(zip(cases, jobs, outs)):
        assert_job_equals_oracle(ia, case, job, out, q)


def test_shared_screen_equals_unshared_and_separate_calls(gpu, shared):
    """The four-job batch under the default (k_screen3rs) and with k_screen3rb forced on the
    shared group (ia_diag_set_c3_shared_screen(0)): torch.equal on every result and B'; both
    equal four separate synthesize_dev calls."""
    import image_analogies as ia
    cases = four_jobs(1)
    L, w = cases[0][4], cases[0][5]
    a, b = dev_jobs(cases, [X] * 4), dev_jobs(cases, [X] * 4)
    assert shared(-1) == 1
    out_a = ia.synthesize_batch_dev(a, L, list(KAPPAS), w, debug=True)
    assert shared(0) == 1
    out_b = ia.synthesize_batch_dev(b, L, list(KAPPAS), w, debug=True)
    assert shared(1) == 0
    for q in range(4):
        same_results(out_a[q], out_b[q])
        assert all(torch.equal(x, y) for x, y in zip(a[q][3], b[q][3]))
        alone = own_job(cases[q])
        ref = ia.synthesize_dev(*alone, L, KAPPAS[q], w, debug=True)
        same_results(out_a[q], ref)
        assert all(torch.equal(x, y) for x, y in zip(a[q][3], alone[3]))


def test_repeated_shared_batch(gpu, shared):
    """The same shared batch twice on one thread: equal results (job and group tables, tickets
    and granules re-initialised), the second equal to the oracle."""
    import image_analogies as ia
    cases = four_jobs(1)
    L, w = cases[0][4], cases[0][5]
    first, second = dev_jobs(cases, [X] * 4), dev_jobs(cases, [X] * 4)
    out1 = ia.synthesize_batch_dev(first, L, list(KAPPAS), w, debug=True)
    out2 = ia.synthesize_batch_dev(second, L, list(KAPPAS), w, debug=True)
    for q in range(4):
        same_results(out1[q], out2[q])
        assert all(torch.equal(x, y) for x, y in zip(first[q][3], second[q][3]))
        assert_job_equals_oracle(ia, cases[q], second[q], out2[q], q)


def test_refusals_of_half_shared_jobs(gpu, shared):
    """Two jobs passing one dbr but another db, or another rot: IA_E_ARG naming the field,
    before anything is launched (every output keeps its fill); the untouched pair then runs."""
    import _ia
    import algorithms
    import image_analogies as ia
    lib, st = _ia.lib(), _ia.stream()
    cases = four_jobs(1)[:2]
    L, w = cases[0][4], _ia.to_dev(cases[0][5])
    jobs = dev_jobs(cases, [X] * 2)
    arr, res, keep = ia._batch3_args(jobs, L, list(KAPPAS[:2]), w, False, True)
    level = L - 1
    pair = lambda: (_ia.IaSynthArgs * 2)(*arr[2 * (L - 2):])  # noqa: E731
    good = pair()
    assert good[0].dbr == good[1].dbr and good[0].db == good[1].db and good[0].rot == good[1].rot
    # a second database and rotation of the same contents in memory of their own
    other = ia._db3_level(*own_job(cases[0])[:2], level)
    rot2 = algorithms.rot3_rotation(other[6], other[5])
    fills = []
    for q in range(2):
        s, im = res[q][level]
        s.fill_(-7)
        im.fill_(-7)
        fills.append((s, im, jobs[q][3][level], jobs[q][3][level].clone()))
    bad = pair()
    bad[1].db = _ia.ptr(other[6]).value
    assert lib.ia_synth_levels3_batch(bad, 1, 2, st) == _ia.IA_E_ARG
    assert lib.ia_last_error().decode().endswith('jobs sharing a dbr differ in db')
    bad = pair()
    bad[1].rot = _ia.ptr(rot2).value
    assert lib.ia_synth_levels3_batch(bad, 1, 2, st) == _ia.IA_E_ARG
    assert lib.ia_last_error().decode().endswith('jobs sharing a dbr differ in rot')
    torch.cuda.synchronize()
    for s, im, bp, bp0 in fills:
        assert bool((s == -7).all()) and bool((im == -7).all()) and torch.equal(bp, bp0)
    assert lib.ia_synth_levels3_batch(good, 1, 2, st) == 0
    assert lib.ia_synth3_status(good, 2, st) == 0
    assert not bool((fills[0][0] == -7).any()) and not bool((fills[1][0] == -7).any())
    del keep


def test_multi_main_shares_the_runs_of_one_a_pair(gpu, shared, monkeypatch, tmp_path):
    """multi_main(batch=5) on five runs from colour PNGs: four name the same A and A' files
    (distinct B files and kappas), the fifth another A' file of the same shape.  The five form
    one batch of two DB groups: _db3_level runs L - 1 times for the four and L - 1 times for
    the fifth; every B' pyramid and every level_*_color.jpg equals the unbatched loop's."""
    from PIL import Image
    import config
    import image_analogies as ia
    from scipy.ndimage import gaussian_filter

    def png(name, img):
        path = str(tmp_path / (name + '.png'))
        Image.fromarray(np.clip(np.round(img * 255), 0, 255).astype(np.uint8), 'RGB').save(path)
        return path
    A = colour(561, (32, 40))
    fA = png('A', A)
    fAp = png('Ap', np.dstack([gaussian_filter(A[..., ch], 1.2) for ch in range(3)]))
    fAp2 = png('Ap2', np.dstack([gaussian_filter(A[..., ch], 2.0) for ch in range(3)]))
    fB = [png('B%d' % i, colour(562 + i, (30, 36))) for i in range(5)]
    ks = [2.0, 11.0, 0.5, 25.0, 4.0]

    def fresh():
        config.convert, config.remap_lum, config.init_rand, config.AB_weight = False, False, True, 1
        config.k, config.seed, config.levels, config.matcher = 2.0, 9, None, 'brute'
        return config

    def runs(tag):
        d = lambda i: str(tmp_path / ('%s%d' % (tag, i))) + '/'  # noqa: E731
        return [(fA, [fAp if i < 4 else fAp2], fB[i], d(i), {'k': ks[i]}) for i in range(5)]
    with monkeypatch.context() as mp:
        calls = count_builds(mp, ia)
        got = ia.multi_main(runs('b'), fresh(), rank=0, world=1, batch=5)
    L = len(got[0])
    per_group = {}
    for key, level in calls['db3']:
        per_group.setdefault(key, []).append(level)
    assert sorted(sorted(v) for v in per_group.values()) == [list(range(1, L))] * 2, calls
    assert calls['rot'] == 2 * (L - 1)
    ref = ia.multi_main(runs('u'), fresh(), rank=0, world=1)
    assert sorted(got) == sorted(ref) == list(range(5))
    for j in ref:
        assert len(got[j]) == len(ref[j])
        for x, y in zip(got[j], ref[j]):
            assert np.array_equal(x, y), j
        names = sorted(os.path.basename(p) for p in glob.glob(str(tmp_path / ('u%d' % j) / '*.jpg')))
        assert len(names) == L
        for n in names:
            assert (tmp_path / ('b%d' % j) / n.replace('u%d' % j, 'b%d' % j)).read_bytes() == \
                (tmp_path / ('u%d' % j) / n).read_bytes(), (j, n)


def kernel_resources():
    """{kernel name: {figure: value}} from the build's report of ia_color3.hip."""
    csrc = os.path.join(ROOT, 'image-analogies-python_amd', 'csrc')
    path = os.path.join(csrc, '_build', 'ia_color3.res')
    assert os.path.exists(path), 'no resource report: build with make -C image-analogies-python_amd/csrc'
    text = open(path).read()
    m = re.search(r'source-sha1: ([0-9a-f]{40})', text)
    src = open(os.path.join(csrc, 'ia_color3.hip'), 'rb').read()
    assert m and hashlib.sha1(src).hexdigest() == m.group(1), 'resource report older than ia_color3.hip'
    out, name = {}, None
    for line in text.splitlines():
        m = re.search(r'Function Name: (\S+)', line)
        if m:       # (plain kernels only: a template's mangled name carries its arguments)
            m = re.match(r'_ZN2ia\d+(k_[a-z0-9_]+?)E[^E]', m.group(1))
            name = m.group(1) if m else None
            if name:
                out[name] = {}
            continue
        m = re.search(r'remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)', line)
        if m and name:
            out[name].setdefault(m.group(1), int(m.group(2)))
    return out


def test_screen_resources():
    """k_screen3rs: no scratch, LDS small enough for two workgroups per CU (<= 81,920 B), the
    occupancy its launch bounds ask for; k_screen3r and k_screen3rb keep the figures of DESIGN
    section 3c (147 VGPRs, 32 SGPRs, 78,848 B of LDS, no scratch)."""
    res = kernel_resources()
    rs = res['k_screen3rs']
    assert rs['ScratchSize'] == 0 and rs['LDS Size'] <= 81920 and rs['Occupancy'] >= 2, rs
    assert rs['VGPRs'] <= 256 and rs['AGPRs'] == 0, rs
    for name in ('k_screen3r', 'k_screen3rb'):
        r = res[name]
        assert (r['VGPRs'], r['TotalSGPRs'], r['LDS Size'], r['ScratchSize']) == (147, 32, 78848, 0), (name, r)
