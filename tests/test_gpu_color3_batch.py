"""Batched 3-channel synthesis (ia_synth_levels3_batch: one k_screen3r and one k_exact3 launch
per wave for K jobs of identical shapes; synthesize_batch_dev / synthesize3_batch_dev /
multi_main(batch=K)) against the numpy oracle's scanline run of every job, the single-job
path and the c1rgb fixture, on every dispatch form, and the C-ABI's refusals."""
import functools
import hashlib
import os
import sys

import numpy as np
import pytest
import torch

import ia_oracle as o
from conftest import smooth_noise

pytestmark = pytest.mark.gpu

KAPPAS = (0.5, 5.0, 25.0)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to('cuda', dtype=torch.float64)


def colour(seed, shape):
    """A smooth colour image (h, w, 3) in [0, 1]: three differently seeded channels."""
    return np.dstack([smooth_noise(seed + 17 * ch, shape) for ch in range(3)])


def pyr3(img, cap=None):
    """Per-channel oracle pyramids stacked (skimage multichannel=True semantics)."""
    chans = [o.compute_gaussian_pyramid(img[..., ch], 3, cap) for ch in range(3)]
    return [np.dstack([c[l] for c in chans]) for l in range(len(chans[0]))]


def inputs(seed, A_shape, B_shape, n_ap=1, cap=None):
    from scipy.ndimage import gaussian_filter
    A = colour(seed, A_shape)
    Aps = [np.dstack([gaussian_filter(A[..., ch], 1.0 + 0.5 * i) for ch in range(3)])
           for i in range(n_ap)]
    B = colour(seed + 1, B_shape)
    A_pyr, B_pyr = pyr3(A, cap), pyr3(B, cap)
    Ap_list = [pyr3(x, cap) for x in Aps]
    L = min(len(A_pyr), len(B_pyr))
    Bp_pyr = o.initialize_Bp(B_pyr, True, seed + 2)
    return A_pyr, Ap_list, B_pyr, Bp_pyr, L


@pytest.fixture
def color16():
    """Select the 3-channel matcher (1 split-f16 screen + exact stage, 0 exhaustive fp64)."""
    import _ia
    lib = _ia.lib()
    prev = lib.ia_diag_set_color16(1)
    yield lib.ia_diag_set_color16
    lib.ia_diag_set_color16(prev)


@functools.lru_cache(maxsize=None)
def job_reference(seed, A_shape, B_shape, n_ap, k):
    """One job's inputs and the oracle's scanline run of them with the debug lists: computed
    once, shared by every dispatch case, never modified."""
    A_pyr, Ap_list, B_pyr, Bp_pyr, L = inputs(seed, A_shape, B_shape, n_ap=n_ap)
    w = o.compute_weights(3, 5, 12, 3)
    As = o.create_index(A_pyr, Ap_list, L)
    Bp_ref = [b.copy() for b in Bp_pyr]
    ref = {}
    for level in range(1, L):
        dbg = {}
        s, im = o.synthesize_level(level, L, A_pyr, Ap_list, B_pyr, Bp_ref, As[level], w, k, debug=dbg)
        ref[level] = (s, im, dbg)
    return A_pyr, Ap_list, B_pyr, Bp_pyr, L, w, Bp_ref, ref


def dev_job(case):
    A_pyr, Ap_list, B_pyr, Bp_pyr = case[:4]
    return ([dev(p) for p in A_pyr], [[dev(p) for p in q] for q in Ap_list], [dev(p) for p in B_pyr],
            [dev(b) for b in Bp_pyr])


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


FORMS = [(1, '1', '1'), (1, '1', '0'), (1, '0', '1'), (0, '1', '1')]
FORM_IDS = ['fused', 'unfused', 'split-fallback', 'fp64-fallback']


@pytest.mark.parametrize('matcher,rot,fuse', FORMS, ids=FORM_IDS)
@pytest.mark.parametrize('n_ap', [1, 2])
def test_three_job_batch_vs_oracle(gpu, color16, monkeypatch, n_ap, matcher, rot, fuse):
    """Three jobs of identical shapes (A 36 x 44, B 30 x 34, every level) with different
    images, B' inits and kappas (0.5, 5, 25) in ONE synthesize_batch_dev call with debug:
    every job's B' (all channels), s, im, sa / sc / rstars and both distance maps equal its
    own oracle run bit for bit; with the fused tail (k_exact3b<true>), IA_C3_FUSE=0
    (k_query3rb + k_exact3b<false>) and the two fall-back forms (IA_DB_ROT=0 and the
    exhaustive search: the jobs one after the other).  The number of A' images is a shape
    (src.nAp), so n_ap = 2 is a batch of its own."""
    import image_analogies as ia
    color16(matcher)
    monkeypatch.setenv('IA_DB_ROT', rot)
    monkeypatch.setenv('IA_C3_FUSE', fuse)
    cases = [job_reference(120 + 5 * q + n_ap, (36, 44), (30, 34), n_ap, k) for q, k in enumerate(KAPPAS)]
    jobs = [dev_job(c) for c in cases]
    outs = ia.synthesize_batch_dev(jobs, cases[0][4], list(KAPPAS), cases[0][5], debug=True)
    assert len(outs) == 3
    for q, (case, job, out) in enumerate(zip(cases, jobs, outs)):
        assert_job_equals_oracle(ia, case, job, out, q)


@pytest.mark.parametrize('fuse', ['1', '0'])
@pytest.mark.parametrize('rot_shared', ['1', '0'])
def test_second_query_tile_vs_oracle(gpu, color16, monkeypatch, fuse, rot_shared):
    """Two jobs with B 40 x 100 (A 36 x 44): waves of up to 34 queries, so the second query
    tile and its padding columns are in play; both jobs equal the oracle with and without the
    fused tail, under one rotation per batch and one per job."""
    import image_analogies as ia
    color16(1)
    monkeypatch.setenv('IA_C3_FUSE', fuse)
    monkeypatch.setenv('IA_ROT3_BATCH_SHARED', rot_shared)
    cases = [job_reference(140 + 7 * q, (36, 44), (40, 100), 1, k) for q, k in enumerate((1.0, 8.0))]
    assert max(min(b.shape[0], (b.shape[1] + 2) // 3) for b in cases[0][2]) == 34
    jobs = [dev_job(c) for c in cases]
    outs = ia.synthesize_batch_dev(jobs, cases[0][4], [1.0, 8.0], cases[0][5], debug=True)
    for q, (case, job, out) in enumerate(zip(cases, jobs, outs)):
        assert_job_equals_oracle(ia, case, job, out, q)


def same_results(a, b):
    assert sorted(a) == sorted(b)
    for level in a:
        assert len(a[level]) == len(b[level])
        for x, y in zip(a[level], b[level]):
            if isinstance(x, tuple):
                assert all(torch.equal(p, q) for p, q in zip(x, y)), level
            else:
                assert torch.equal(x, y), level


def test_one_job_batch_and_repeated_call(gpu, color16):
    """synthesize_batch_dev with one colour job equals synthesize_dev on the same inputs
    (torch.equal on everything); a second identical 2-job batch call on the same thread gives
    the same result (tickets, granules and error words re-initialised)."""
    import image_analogies as ia
    color16(1)
    cases = [job_reference(120 + 5 * q + 1, (36, 44), (30, 34), 1, k) for q, k in enumerate(KAPPAS[:2])]
    L, w = cases[0][4], cases[0][5]
    one, alone = dev_job(cases[0]), dev_job(cases[0])
    got = ia.synthesize_batch_dev([one], L, KAPPAS[0], w, debug=True)
    ref = ia.synthesize_dev(*alone, L, KAPPAS[0], w, debug=True)
    assert len(got) == 1
    same_results(got[0], ref)
    assert all(torch.equal(x, y) for x, y in zip(one[3], alone[3]))
    first, second = [dev_job(c) for c in cases], [dev_job(c) for c in cases]
    out1 = ia.synthesize_batch_dev(first, L, list(KAPPAS[:2]), w, debug=True)
    out2 = ia.synthesize_batch_dev(second, L, list(KAPPAS[:2]), w, debug=True)
    for q in range(2):
        same_results(out1[q], out2[q])
        assert all(torch.equal(x, y) for x, y in zip(first[q][3], second[q][3]))
        assert_job_equals_oracle(ia, cases[q], second[q], out2[q], q)


def test_c1rgb_inside_a_batch(gpu, color16):
    """The c1rgb workload (180 x 117, kappa 0.5) as job 0 of a 2-job batch whose job 1 is the
    same workload with kappa 5: job 0's s, im and B' hashes of every level equal
    tests/golden/c1rgb_oracle.npz; job 1 equals a separate synthesize_dev run."""
    import image_analogies as ia
    from conftest import ROOT, golden
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
    import make_config_fixtures as mcf
    color16(1)
    g = golden('c1rgb_oracle.npz')
    A_pyr, Ap_list, B_pyr, Bp_pyr, L, k = mcf.colour_workload('c1rgb')
    assert L == int(g['max_levels'])
    w = o.compute_weights(3, 5, 12, 3)
    case = (A_pyr, Ap_list, B_pyr, Bp_pyr)
    jobs = [dev_job(case), dev_job(case)]
    alone = dev_job(case)
    outs = ia.synthesize_batch_dev(jobs, L, [k, 5.0], w)
    ref = ia.synthesize_dev(*alone, L, 5.0, w)
    torch.cuda.synchronize()
    assert sorted(outs[0]) == list(range(1, L))
    for level in range(1, L):
        s, im = outs[0][level]
        assert np.array_equal(s.cpu().numpy(), g['s%d' % level].astype(np.int32)), level
        assert np.array_equal(im.cpu().numpy(), g['im%d' % level].astype(np.int32)), level
        bp = np.ascontiguousarray(jobs[0][3][level].cpu().numpy(), dtype=np.float64)
        assert hashlib.sha256(bp.tobytes()).hexdigest() == str(g['bp_sha%d' % level]), level
        assert torch.equal(jobs[1][3][level], alone[3][level]), level
    same_results(outs[1], ref)


def test_batch_refusals_through_the_c_abi(gpu, color16):
    """ia_synth_levels3_batch returns IA_E_ARG, before anything is launched (every output
    keeps its fill), for jobs of different W, for K = 2 without a rotated DB, and for K = 0
    and K = 129."""
    import _ia
    import algorithms
    import image_analogies as ia
    color16(1)
    lib, st = _ia.lib(), _ia.stream()
    w = _ia.to_dev(o.compute_weights(3, 5, 12, 3))
    fills = []

    def level_args(seed, B_shape, rotated):
        A_pyr, Ap_list, B_pyr, Bp_pyr = dev_job(inputs(seed, (20, 24), B_shape)[:4])
        level = len(B_pyr) - 1
        built = ia._db3_level(A_pyr, Ap_list, level)
        rot = dbr = None
        if rotated:
            rot, dbr = algorithms.rot3_build(built[6], built[5])
        a, (s, im, _), bufs = ia._level3_args(built, rot, dbr, B_pyr, Bp_pyr, level, level + 1, 1.0, w, False)
        s.fill_(-7)
        im.fill_(-7)
        fills.append((s, im, Bp_pyr[level], Bp_pyr[level].clone()))
        return a, (built, rot, dbr, bufs, A_pyr, Ap_list, B_pyr, Bp_pyr)

    def call(args, K):
        arr = (_ia.IaSynthArgs * len(args))(*args)
        return lib.ia_synth_levels3_batch(arr, 1, K, st)

    a0, k0 = level_args(150, (16, 18), True)
    a1, k1 = level_args(152, (16, 18), True)
    a2, k2 = level_args(154, (16, 20), True)
    b0, k3 = level_args(156, (16, 18), False)
    b1, k4 = level_args(158, (16, 18), False)
    assert call([a0, a2], 2) == _ia.IA_E_ARG
    assert 'W' in lib.ia_last_error().decode()
    assert call([b0, b1], 2) == _ia.IA_E_ARG
    assert 'dbr' in lib.ia_last_error().decode()
    assert call([a0, a1], 0) == _ia.IA_E_ARG
    assert call([a0, a1] * 65, 129) == _ia.IA_E_ARG
    torch.cuda.synchronize()
    for s, im, bp, bp0 in fills:
        assert bool((s == -7).all()) and bool((im == -7).all()) and torch.equal(bp, bp0)
    # the same arguments pass once they agree: the refusals were about the arguments alone
    assert call([a0, a1], 2) == 0
    arr = (_ia.IaSynthArgs * 2)(a0, a1)
    assert lib.ia_synth3_status(arr, 2, st) == 0
    assert not bool((fills[0][0] == -7).any()) and not bool((fills[1][0] == -7).any())


def test_multi_main_batch_equals_unbatched(gpu, color16, tmp_path):
    """multi_main(batch=2) on three runs from small colour PNGs: runs 0 and 1 have the same
    shapes and differ in k (run 1 through an override, run 0 keeps the config's own), run 2 has
    another B size and goes alone.  The returned B' pyramids equal those of multi_main without
    batch, every level_*_color.jpg has identical bytes, and the overrides of the batched path
    leave the caller's config as it was."""
    import glob
    from PIL import Image
    import config
    import image_analogies as ia
    from scipy.ndimage import gaussian_filter
    color16(1)

    def png(name, img):
        path = str(tmp_path / (name + '.png'))
        Image.fromarray(np.clip(np.round(img * 255), 0, 255).astype(np.uint8), 'RGB').save(path)
        return path
    A = colour(161, (32, 40))
    fA = png('A', A)
    fAp = png('Ap', np.dstack([gaussian_filter(A[..., ch], 1.2) for ch in range(3)]))
    fB0, fB1, fB2 = png('B0', colour(162, (30, 36))), png('B1', colour(163, (30, 36))), png('B2', colour(164, (26, 33)))

    def fresh():
        config.convert, config.remap_lum, config.init_rand, config.AB_weight = False, False, True, 1
        config.k, config.seed, config.levels, config.matcher = 2.0, 9, None, 'brute'
        return config

    def runs(tag):
        d = lambda i: str(tmp_path / ('%s%d' % (tag, i))) + '/'  # noqa: E731
        return [(fA, [fAp], fB0, d(0)), (fA, [fAp], fB1, d(1), {'k': 11.0}), (fA, [fAp], fB2, d(2), {'k': 0.5})]
    cb = fresh()
    got = ia.multi_main(runs('b'), cb, rank=0, world=1, batch=2)
    assert cb.k == 2.0
    ref = ia.multi_main(runs('u'), fresh(), rank=0, world=1)
    assert sorted(got) == sorted(ref) == [0, 1, 2]
    for j in ref:
        assert len(got[j]) == len(ref[j])
        for x, y in zip(got[j], ref[j]):
            assert np.array_equal(x, y), j
        names = sorted(os.path.basename(p) for p in glob.glob(str(tmp_path / ('u%d' % j) / 'level_*_color.jpg')))
        assert names
        for n in names:
            assert (tmp_path / ('b%d' % j) / n).read_bytes() == (tmp_path / ('u%d' % j) / n).read_bytes(), (j, n)
    # run 0 kept the config's own k: a single run of it with k = 2 gives the same B'
    alone = ia.multi_main(runs('a')[:1], fresh(), rank=0, world=1)
    assert all(np.array_equal(x, y) for x, y in zip(got[0], alone[0]))
    other = fresh()
    other.k = 11.0
    differs = ia.multi_main(runs('d')[:1], other, rank=0, world=1)
    assert not all(np.array_equal(x, y) for x, y in zip(got[0], differs[0]))
