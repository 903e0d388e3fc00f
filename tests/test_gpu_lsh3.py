"""The LSH matcher for 3-channel matching (c.matcher = 'lsh' with convert=False): the HIP
tables (ia_lsh3_build), the stand-alone query (ia_lsh3_match_batch) and the fused per-pixel
kernel of the synthesis (k_lsh3_pixel, through ia_synth_level3 and ia_synth_levels3) against
the numpy restatement of the definition (tests/lsh3_ref.py), driven by the device's own centre,
width and projections.  There is no reference LSH code: these pin the HIP path to this build's
definition.  test_lsh3_ref.py shows that on these inputs an LSH synthesis differs from the
exact one on most pixels, so none of the parity tests below passes on the exact matcher."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import lsh3_ref as r

pytestmark = pytest.mark.gpu

IDS = lambda p: '%d-%d-%g-%d' % p  # noqa: E731


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to('cuda', dtype=torch.float64)


def kw(params):
    return dict(zip(('tables', 'hashes', 'width', 'seed'), params))


def level_index(case, level, params):
    """The device index of one level with its LSH tables, and the restatement over the same
    centre, width and projections."""
    import algorithms
    A_pyr, Ap_list, _, _, _, As, _ = case
    index = algorithms.LevelIndex3(dev(A_pyr[level - 1]), dev(A_pyr[level]),
                                   torch.stack([dev(p[level - 1]) for p in Ap_list]),
                                   torch.stack([dev(p[level]) for p in Ap_list])).build_lsh(**kw(params))
    return index, restatement(index, As[level])


def restatement(index, As_level):
    h = index.lsh
    assert index.lsh_proj_host.shape == (h.L * h.k, 168)
    assert index.center.shape == (165,) and index.lsh_proj.shape == (h.L * h.k, 168)
    return r.LshIndexD(As_level, index.center.cpu().numpy(), index.lsh_proj_host, h.L, h.k,
                       np.float32(h.w))


@functools.lru_cache(maxsize=None)
def reference(params, twice=False):
    """The oracle's scanline synthesis of the case driven by the restatement over the device's
    centre, width and projections of every level: computed once per parameter set, shared by
    the dispatch cases, never modified."""
    case = r.case(93, (12, 14), (11, 13), 1, True) if twice else r.case()
    ref, Bp_ref, tabs = r.oracle_synthesis(case, 1.0, lambda level: level_index(case, level, params)[1])
    return case, ref, Bp_ref, tabs


def run_device(case, params, **kwargs):
    import image_analogies as ia
    A_pyr, Ap_list, B_pyr, Bp_pyr, L, _, w = case
    Bp_dev = [dev(b) for b in Bp_pyr]
    out = ia.synthesize_dev([dev(p) for p in A_pyr], [[dev(p) for p in q] for q in Ap_list],
                            [dev(p) for p in B_pyr], Bp_dev, L, 1.0, w, lsh=kw(params), **kwargs)
    torch.cuda.synchronize()
    return out, Bp_dev


def assert_equals_oracle(out, Bp_dev, ref, Bp_ref, L):
    for level in range(1, L):
        assert np.array_equal(out[level][0].cpu().numpy(), ref[level][0]), level
        assert np.array_equal(out[level][1].cpu().numpy(), ref[level][1]), level
        got = Bp_dev[level].cpu().numpy()
        assert got.shape[2] == 3 and np.array_equal(got, Bp_ref[level]), level


@pytest.mark.parametrize('params', r.MATCH_PARAMS, ids=IDS)
def test_lsh3_match_vs_restatement(gpu, params):
    """LevelIndex3.match on the finest level (2,400 rows), 250 queries (100 rows, 100 perturbed
    rows, 50 uniform): the restatement's index on >= 99 % of them (the project's tolerance for
    fp32 double rounding in the emulated FMA chain, as test_gpu_lsh.py), the distance bit-equal
    where the indices agree and never below the exact one; exact=True is still brute force."""
    case = r.case()
    L, As = case[4], case[5][case[4] - 1]
    assert As.shape == (2400, 165)
    index, ref = level_index(case, L - 1, params)
    rs = np.random.RandomState(4)
    Q = np.vstack([As[rs.randint(0, len(As), 100)],
                   As[rs.randint(0, len(As), 100)] + rs.randn(100, 165) * 0.01,
                   rs.rand(50, 165)])
    gi, gd = index.match(Q)
    gi, gd = gi.cpu().numpy(), gd.cpu().numpy()
    ri, rd = ref.match(Q)
    same = gi == ri
    print('indices equal on %.4f of the queries; look-ups: %.3f empty, %.3f capped'
          % (same.mean(), ref.empty / ref.lookups, ref.capped / ref.lookups))
    assert same.mean() >= 0.99, same.mean()
    assert np.array_equal(gd[same], rd[same])
    ei, ed = index.match(Q, exact=True)
    ei, ed = ei.cpu().numpy(), ed.cpu().numpy()
    assert np.all(gd >= ed)
    D = np.array([np.add.reduce((As - q) ** 2, axis=1) for q in Q])
    assert np.array_equal(ed, D.min(1))
    assert np.array_equal(ei, D.argmin(1))


@pytest.mark.parametrize('pipeline', [False, True], ids=['level3', 'levels3'])
@pytest.mark.parametrize('params', r.SYNTH_PARAMS, ids=IDS)
def test_lsh3_synthesis_vs_oracle(gpu, params, pipeline):
    """Whole levels with the LSH matcher, kappa 1: s, im and all three channels of B' equal the
    scanline oracle driven by the restatement, level by level, one level at a time
    (ia_synth_level3) and pipelined (ia_synth_levels3)."""
    case, ref, Bp_ref, _ = reference(params)
    out, Bp_dev = run_device(case, params, pipeline=pipeline)
    assert_equals_oracle(out, Bp_dev, ref, Bp_ref, case[4])


def test_lsh3_debug_record_holds_the_lsh_pick(gpu):
    """With debug outputs the record's p_app is the LSH pick (the oracle's sa under the
    restatement), and the other debug lists and maps equal the oracle's too."""
    import image_analogies as ia
    params = r.SYNTH_PARAMS[0]
    case, ref, Bp_ref, _ = reference(params)
    out, Bp_dev = run_device(case, params, debug=True)
    assert_equals_oracle(out, Bp_dev, ref, Bp_ref, case[4])
    for level in range(1, case[4]):
        s, im, dbg = out[level]
        rec = ia.debug_record(s, im, dbg, Bp_ref[level].shape[:2])
        rd = ref[level][2]
        for key in ('sa', 'sc', 'rstars'):
            assert rec[key] == rd[key], (level, key)
        assert np.array_equal(rec['app_dist'], rd['app_dist']), level
        assert np.array_equal(rec['coh_dist'], rd['coh_dist']), level


@pytest.mark.parametrize('params', r.SYNTH_PARAMS, ids=IDS)
def test_lsh3_ties_take_the_lower_row(gpu, params):
    """The A' pyramid listed twice: every row exists twice and the distances tie exactly; the
    (distance, row) order decides, as in the restatement (which picks image 0 wherever both
    rows of a pair are candidates)."""
    case, ref, Bp_ref, _ = reference(params, True)
    out, Bp_dev = run_device(case, params)
    assert_equals_oracle(out, Bp_dev, ref, Bp_ref, case[4])
    im = np.concatenate([ref[level][1] for level in range(1, case[4])])
    print('image 0 on %.3f of the pixels' % (im == 0).mean())


def test_lsh3_api_create_index(gpu):
    """create_index honours c.matcher = 'lsh' on colour pyramids: params describe the tables and
    best_approximate_match(_batch) goes through them."""
    import algorithms
    import config as c
    A_pyr, Ap_list, _, _, L, As, _ = r.case()
    old = c.matcher, getattr(c, 'max_levels', None)
    try:
        c.matcher, c.max_levels = 'lsh', L
        flann, params, lazy, sizes = algorithms.create_index(A_pyr, Ap_list, c)
    finally:
        c.matcher, c.max_levels = old
    lv = L - 1
    assert params[lv]['algorithm'] == 'lsh' and not params[lv]['exact']
    assert (params[lv]['tables'], params[lv]['hashes']) == (c.lsh_tables, c.lsh_hashes)
    assert sizes[lv] == (2400, 165) and np.array_equal(lazy[lv], As[lv])
    ref = restatement(flann[lv], As[lv])
    rs = np.random.RandomState(6)
    Q = As[lv][rs.randint(0, 2400, 12)] * 0.98
    want = ref.match(Q)[0]
    assert algorithms.best_approximate_match(flann[lv], params[lv], Q[0]) == want[0]
    assert np.array_equal(algorithms.best_approximate_match_batch(flann[lv], Q), want)


def test_lsh3_main_end_to_end(gpu, tmp_path):
    """image_analogies_main on small colour files with c.matcher = 'lsh' and convert=False
    returns the B' pyramid of synthesize_dev(lsh=...) on setup_dev's pyramids, which is not the
    exact run's."""
    from PIL import Image
    from scipy.ndimage import gaussian_filter
    import algorithms
    import config as c
    import image_analogies as ia
    A = r.colour(95, (26, 30))
    Ap = np.dstack([gaussian_filter(A[..., ch], 1.2) for ch in range(3)])
    B = r.colour(96, (24, 20))
    files = {}
    for name, img in (('A', A), ('Ap', Ap), ('B', B)):
        files[name] = str(tmp_path / (name + '.png'))
        Image.fromarray(np.clip(np.round(img * 255), 0, 255).astype(np.uint8), 'RGB').save(files[name])
    old = c.matcher
    c.convert, c.remap_lum, c.init_rand, c.AB_weight, c.k, c.seed = False, False, True, 1, 1.0, 5
    c.levels = None
    try:
        c.matcher = 'lsh'
        got = ia.image_analogies_main(files['A'], [files['Ap']], files['B'], str(tmp_path / 'out') + '/', c)
        lsh = algorithms.lsh_params(c)
        assert lsh is not None

        def direct(lsh):
            A_pyr, Ap_pyr, B_pyr, Bp_pyr, _ = ia.setup_dev(ia._read(files['A']), [ia._read(files['Ap'])],
                                                          ia._read(files['B']), c)
            ia.synthesize_dev(A_pyr, Ap_pyr, B_pyr, Bp_pyr, c.max_levels, c.k, _ia_weights(c), lsh=lsh)
            torch.cuda.synchronize()
            return [p.cpu().numpy() for p in Bp_pyr]
        same, exact = direct(lsh), direct(None)
    finally:
        c.matcher = old
    assert len(got) == len(same) == len(exact) and got[-1].shape == (24, 20, 3)
    for level in range(len(got)):
        assert np.array_equal(got[level], same[level]), level
    assert any(not np.array_equal(got[level], exact[level]) for level in range(1, len(got)))


def _ia_weights(c):
    import _ia
    return _ia.to_dev(c.weights)


class PlainLevel:
    """IaSynthArgs of the finest level of the tests' case with LSH tables (nothing is launched
    with it but refusals), outputs filled with -7."""

    def __init__(self, params=r.SYNTH_PARAMS[0]):
        import _ia
        import algorithms
        import image_analogies as ia
        A_pyr, Ap_list, B_pyr, Bp_pyr, L, _, w = r.case()
        A = [dev(p) for p in A_pyr]
        Ap = [[dev(p) for p in q] for q in Ap_list]
        self.B, self.Bp = [dev(p) for p in B_pyr], [dev(p) for p in Bp_pyr]
        self.level = L - 1
        self.built = ia._db3_level(A, Ap, self.level)
        self.rot, self.dbr = algorithms.rot3_build(self.built[6], self.built[5])
        self.tabs = algorithms.lsh3_tables(self.built[1], self.built[3], self.built[6], self.built[5], **kw(params))
        self.w = _ia.to_dev(w)
        self.args, (self.s, self.im, _), self.bufs = ia._level3_args(
            self.built, self.rot, self.dbr, self.B, self.Bp, self.level, L, 1.0, self.w, False)
        self.args.lsh = ctypes.pointer(self.tabs[0])
        self.args.center = _ia.ptr(self.tabs[1]).value
        self.s.fill_(-7)
        self.im.fill_(-7)
        self.bp0 = self.Bp[self.level].clone()

    def untouched(self):
        torch.cuda.synchronize()
        return (bool((self.s == -7).all()) and bool((self.im == -7).all()) and
                torch.equal(self.Bp[self.level], self.bp0))


def copy_args(a):
    import _ia
    b = _ia.IaSynthArgs()
    ctypes.memmove(ctypes.byref(b), ctypes.byref(a), ctypes.sizeof(b))
    return b


def test_lsh3_refusals_through_the_c_abi(gpu):
    """IA_E_ARG before anything is launched (every output keeps its fill): an lsh without its
    centre, tables of L k = 65 hashes, and an lsh inside ia_synth_levels3_batch for K = 1 and 2."""
    import _ia
    lib, st = _ia.lib(), _ia.stream()
    lv = PlainLevel()

    def refused(a, what):
        assert lib.ia_synth_level3(ctypes.byref(a), st) == _ia.IA_E_ARG, what
        assert 'lsh' in lib.ia_last_error().decode(), what
        arr = (_ia.IaSynthArgs * 1)(a)
        assert lib.ia_synth_levels3(arr, 1, st) == _ia.IA_E_ARG, what
        assert 'lsh' in lib.ia_last_error().decode(), what

    a = copy_args(lv.args)
    a.center = None
    refused(a, 'no centre')
    big = _ia.IaLsh()
    ctypes.memmove(ctypes.byref(big), ctypes.byref(lv.tabs[0]), ctypes.sizeof(big))
    big.L, big.k = 13, 5
    a = copy_args(lv.args)
    a.lsh = ctypes.pointer(big)
    refused(a, 'L k = 65')
    for K in (1, 2):
        arr = (_ia.IaSynthArgs * K)(*[lv.args] * K)
        assert lib.ia_synth_levels3_batch(arr, 1, K, st) == _ia.IA_E_ARG
        assert 'lsh' in lib.ia_last_error().decode()
    assert lv.untouched()
    # the same arguments as they stand do run (the refusals above were about what was changed)
    _ia.check(lib.ia_synth_level3(ctypes.byref(lv.args), st), 'ia_synth_level3')
    assert not lv.untouched()
