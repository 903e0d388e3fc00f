"""Pin the CPU oracle against the reference: golden vectors produced by the reference's
own modules (tests/golden/make_golden.py), the KATs of the reference's tests
(algorithms_test.py, config_test.py, img_preprocess_test.py), and C-vs-numpy oracle
agreement.  CPU only."""
import numpy as np
import pytest

import ia_oracle as o
import ia_oracle_c as oc
from conftest import analogy_inputs, golden


# ---- config.py ----------------------------------------------------------------------------

def test_weights_match_reference_goldens():
    g = golden()
    g310 = golden('ref_weights_py310.npz')
    for ch, key in ((1, 'ch1'), (3, 'ch3')):
        w = o.compute_weights(3, 5, 12, ch)
        # reference config.py under this interpreter's numpy: bit-exact
        assert np.array_equal(w, g310[key])
        # under the skimage-era numpy 1.26.4: np.exp differs by <= 1 ulp
        assert np.allclose(w, g['weights_%s' % key], rtol=1e-15, atol=0)


def test_compute_weights_kat():
    """config_test.py:5-62 restated."""
    for ch in (1, 3):
        gs = o.matlab_style_gauss2D((3, 3), 0.5)
        gl = o.matlab_style_gauss2D((5, 5), 1)
        w_sm = np.repeat(((1. / 9) * gs).flatten(), ch)
        w_lg = np.repeat(((1. / 25) * gl).flatten(), ch)
        w_half = np.repeat(((1. / 12) * gl.flatten()[:12]), ch)
        assert len(w_sm) == 9 * ch and len(w_lg) == 25 * ch and len(w_half) == 12 * ch
        assert np.isclose(np.sum(w_sm), ch / 9.)
        assert np.isclose(np.sum(w_lg), ch / 25.)
        assert np.sum(w_half) < ch * 0.5 / 12
        assert np.allclose(o.compute_weights(3, 5, 12, ch), np.hstack([w_sm, w_lg, w_sm, w_half]))


# ---- img_preprocess.py -------------------------------------------------------------------------

def test_yiq_rgb_match_reference():
    g = golden()
    assert np.array_equal(o.convert_to_YIQ(g['yiq_in']), g['yiq_out'])
    assert np.array_equal(o.convert_to_RGB(g['yiq_out']), g['rgb_out'])
    assert np.array_equal(o.convert_to_YIQ(g['yiq_u8_in'] / 255.), g['yiq_u8_out'])


def test_yiq_einsum_order():
    """The kernels' per-channel order (m0*x0 + m2*x2) + m1*x1 is numpy's einsum order."""
    x = np.random.RandomState(3).rand(31, 17, 3)
    e = o.convert_to_YIQ(x)
    for i in range(3):
        m = o.YIQ_M[i]
        assert np.array_equal(e[..., i], (m[0] * x[..., 0] + m[2] * x[..., 2]) + m[1] * x[..., 1])


def test_converts_roundtrip():
    """img_preprocess_test.py:6-13."""
    img = np.random.RandomState(0xba5eba11).rand(25, 25, 3)
    assert np.allclose(o.convert_to_RGB(o.convert_to_YIQ(img)), img, atol=0.05)
    for img in (np.ones((25, 25, 3)), np.zeros((25, 25, 3))):
        assert np.allclose(o.convert_to_RGB(o.convert_to_YIQ(img)), img)


def test_remap_luminance_matches_reference():
    g = golden()
    a, ap = o.remap_luminance(g['remap_A'], [g['remap_Ap']], g['remap_B'])
    assert np.array_equal(a, g['remap_A_out']) and np.array_equal(ap[0], g['remap_Ap_out'])
    # img_preprocess_test.py:16-26 intent (the reference test passes a bare array)
    B = g['remap_B']
    for X in (a, ap[0]):
        assert np.isclose(np.mean(B), np.mean(X), atol=0.05)
        assert np.isclose(np.std(B), np.std(X), atol=0.05)


@pytest.mark.parametrize('k', range(9))
def test_pyramid_bit_exact_vs_skimage(k):
    """img_preprocess.py:47-63 -> skimage 0.18.3 pyramid_gaussian, every level bit-exact."""
    g = golden()
    img = g['pyr%d_in' % k]
    n = int(g['pyr%d_n' % k])
    pyr = o.compute_gaussian_pyramid(img, 3)
    assert len(pyr) == n
    for l in range(n):
        assert np.array_equal(pyr[l], g['pyr%d_l%d' % (k, l)]), (k, l)


def test_oracle_reproduces_reference_setup_fixture():
    """ref_setup_golden.npz (make_setup_golden.py: the reference's pyramids of plateau and noise
    images outside [0, 1] at 45 x 61 and 21 x 37, and its remap_luminance + compress_values +
    pyramid chain): the oracle reproduces every array bit for bit, so it is a sound reference
    for out-of-range data; the seeded generators still give the inputs the fixture was
    made from."""
    import test_gpu_setup as gs
    g = golden('ref_setup_golden.npz')
    images = gs.msg.golden_images()
    assert len(images) == 16
    for name, img in images.items():
        assert gs.msg.sha(img) == str(g[name + '_sha']), name
        pyr = o.compute_gaussian_pyramid(img, 3)
        assert len(pyr) == int(g[name + '_n']) >= 3, name
        for l in range(len(pyr) - 1):
            assert np.array_equal(pyr[l], g['%s_l%d' % (name, l)]), (name, l)
    A, Ap, B = gs.msg.chain_inputs()
    assert [gs.msg.sha(x) for x in (A, Ap, B)] == [str(s) for s in g['chain_sha']]
    Ar, Apr = o.remap_luminance(A, [Ap], B)
    assert Apr[0].min() < -0.5 and Apr[0].max() > 1.5
    Ac, Bc = o.compress_values(Ar, B, gs.msg.CHAIN_WEIGHT)
    for name, img in (('A', Ac), ('Ap', Apr[0]), ('B', Bc)):
        pyr = o.compute_gaussian_pyramid(img, 3)
        assert len(pyr) == int(g['chain_%s_n' % name]), name
        for l, lvl in enumerate(pyr):
            assert np.array_equal(lvl, g['chain_%s_l%d' % (name, l)]), (name, l)


def test_plateau_inputs_engage_the_clip():
    """The inputs of test_gpu_setup.test_pyramid_clip_engaged_vs_oracle have teeth: on every
    plateau pair and shape the oracle's clip changes values on the side(s) the pair can engage
    (the fixture's sizes included), while it changes none on the saturated noise of
    test_pyramid_streaming_form_equals_tiled[flat] nor on an even-sized plateau image."""
    import test_gpu_setup as gs
    assert len(gs.PLATEAU_CASES) == 18
    for name, shape in gs.PLATEAU_CASES:
        gs.assert_clip_engaged(name, gs.plateau_image(name, shape))
    for shape in [(2048, 2048), (96, 130), (8, 4), (517, 300), (33, 1000), (4, 5), (2, 2), (3, 255), (257, 124)]:
        flat = np.minimum(1.0, np.random.RandomState(sum(shape)).rand(*shape) * 3.0)
        assert gs.clip_counts(flat) == (0, 0), shape
    assert gs.clip_counts(gs.plateau_image('mixed', (96, 130))) == (0, 0)


def test_initialize_Bp():
    """img_preprocess_test.py:29-42 intent, seeded."""
    img = np.random.RandomState(0xba5eba11).rand(25, 40)
    pyr = o.compute_gaussian_pyramid(img, 3)
    for a, b in zip(pyr, o.initialize_Bp(pyr, init_rand=False)):
        assert np.array_equal(a, b)
    for a, b in zip(pyr, o.initialize_Bp(pyr, init_rand=True, seed=5)):
        assert not np.allclose(a, b)
    r1 = o.initialize_Bp(pyr, True, seed=5)
    r2 = o.initialize_Bp(pyr, True, seed=5)
    assert all(np.array_equal(a, b) for a, b in zip(r1, r2))


# ---- algorithms.py KATs (algorithms_test.py:10-115) --------------------------------------------

SM_0 = np.array([[0, 0, 0.5], [0, 0, 0.5], [0.5, 0.5, 0.5]])
LG_0 = np.array([[0.3, 0.3, 0.3, 0.3, 0.3],
                 [0.3, 1, 1, 0.3, 0.3],
                 [0.3, 1, 1, 0.3, 0.3],
                 [0.3, 0.3, 0.3, 0.3, 0.3],
                 [0.3, 0.3, 0.3, 0.3, 0.3]])


def kat_images():
    sm = 0.5 * np.ones((4, 5)); sm[0, 0] = 0
    lg = 0.3 * np.ones((7, 10)); lg[0, 0] = 1
    return sm, lg


def test_compute_feature_array_kat():
    sm, lg = kat_images()
    feat = o.compute_feature_array([sm, lg], True)
    assert len(feat) == 2 and feat[0] == []
    assert feat[1].shape == (70, 34)
    assert np.allclose(feat[1][0], np.hstack([SM_0.flatten(), LG_0.flatten()]))
    feat = o.compute_feature_array([sm, lg], False)
    assert feat[1].shape == (70, 21)
    assert np.allclose(feat[1][0], np.hstack([SM_0.flatten(), LG_0.flatten()[:12]]))


def test_extract_pixel_feature_kat():
    sm, lg = kat_images()
    assert np.allclose(o.extract_pixel_feature(sm, lg, (0, 0), True),
                       np.hstack([SM_0.flatten(), LG_0.flatten()]))
    assert np.allclose(o.extract_pixel_feature(sm, lg, (0, 0), False),
                       np.hstack([SM_0.flatten(), LG_0.flatten()[:12]]))
    # the index-map form equals explicit symmetric padding (algorithms.py:81-84)
    psm, plg = o.pad_img_pair(sm, lg)
    for r in range(7):
        for c in range(10):
            ref = np.hstack([psm[r // 2:r // 2 + 3, c // 2:c // 2 + 3].flatten(),
                             plg[r:r + 5, c:c + 5].flatten()])
            assert np.array_equal(o.extract_pixel_feature(sm, lg, (r, c), True), ref)


def test_best_coherence_match_property():
    """algorithms_test.py:158-207 restated with the current signature: with B = A and
    s(q - (1,1)) = q - (1,1), coherence must return exactly q."""
    A, Aps, _ = analogy_inputs(7, (40, 52), (8, 8))
    A_pyr = o.compute_gaussian_pyramid(A, 3)
    Ap_pyr = o.compute_gaussian_pyramid(Aps[0], 3)
    As = o.create_index(A_pyr, [Ap_pyr], len(A_pyr))[-1]
    imh, imw = A.shape
    rs = np.random.RandomState(1)
    for row, col in [(1, 1), (1, imw - 1), (imh - 1, 1), (imh - 1, imw - 1), (imh // 2, imw // 2)]:
        num_px = row * imw + col
        s = [(int(a), int(b)) for a, b in zip(rs.randint(0, imh, num_px), rs.randint(0, imw, num_px))]
        s[(row - 1) * imw + col - 1] = (row - 1, col - 1)
        im = [0] * num_px
        q = As[row * imw + col]
        p, i, r_star = o.best_coherence_match(As, (imh, imw), q, s, im, (row, col), imw)
        assert p == (row, col) and i == 0


def test_brute_force_is_first_min():
    rs = np.random.RandomState(2)
    As = rs.rand(500, 55)
    As[300] = As[100]       # exact duplicate: the lower row must win
    assert o.best_approximate_match(As, As[100] + 1e-9) == 100


# ---- C oracle == numpy oracle (end to end) -------------------------------------------------------

@pytest.mark.parametrize('case', [
    dict(seed=0, A=(30, 40), B=(28, 33), n_ap=1, k=0.5, flat=False),
    dict(seed=3, A=(26, 21), B=(17, 30), n_ap=2, k=5.0, flat=False),
    dict(seed=5, A=(24, 24), B=(24, 24), n_ap=1, k=2.0, flat=True),
])
def test_c_oracle_equals_numpy_oracle(case):
    A, Aps, B = analogy_inputs(case['seed'], case['A'], case['B'], case['n_ap'], case['flat'])
    A_pyr, Ap_list, B_pyr, Bp_pyr, L = o.setup_luminance(A, Aps, B, seed=case['seed'])
    Bp2 = [b.copy() for b in Bp_pyr]
    r1 = o.synthesize(A_pyr, Ap_list, B_pyr, Bp_pyr, L, case['k'])
    r2 = oc.synthesize(A_pyr, Ap_list, B_pyr, Bp2, L, case['k'], o.compute_weights(3, 5, 12, 1))
    assert set(r1) == set(r2) == set(range(1, L))
    for l in r1:
        for a, b in zip(r1[l], r2[l]):
            assert np.array_equal(a, b), l


def _colour_inputs(seed, A_shape, B_shape, n_ap):
    """3-channel analogy pyramids (per-channel, skimage multichannel semantics)."""
    from scipy.ndimage import gaussian_filter
    from conftest import smooth_noise
    A = np.dstack([smooth_noise(seed + 17 * ch, A_shape) for ch in range(3)])
    Aps = [np.dstack([gaussian_filter(A[..., ch], 1.0 + 0.5 * i) for ch in range(3)]) for i in range(n_ap)]
    B = np.dstack([smooth_noise(seed + 1 + 17 * ch, B_shape) for ch in range(3)])

    def pyr3(img):
        chans = [o.compute_gaussian_pyramid(img[..., ch], 3) for ch in range(3)]
        return [np.dstack([c[l] for c in chans]) for l in range(len(chans[0]))]
    A_pyr, B_pyr = pyr3(A), pyr3(B)
    Ap_list = [pyr3(x) for x in Aps]
    L = min(len(A_pyr), len(B_pyr))
    return A_pyr, Ap_list, B_pyr, o.initialize_Bp(B_pyr, True, seed + 2), L


@pytest.mark.parametrize('seed,A,B,n_ap,k', [(11, (30, 40), (20, 26), 1, 0.5), (12, (24, 22), (18, 20), 2, 25.0)])
def test_c_oracle_colour_equals_numpy_oracle(seed, A, B, n_ap, k):
    """The C oracle's 3-channel form (num_ch = 3, config.py:29-42: 165-dim rows, every
    channel of B' updated) equals the numpy oracle end to end, with the scan and with the
    projection index."""
    A_pyr, Ap_list, B_pyr, Bp_pyr, L = _colour_inputs(seed, A, B, n_ap)
    w = o.compute_weights(3, 5, 12, 3)
    r1 = o.synthesize(A_pyr, Ap_list, B_pyr, [b.copy() for b in Bp_pyr], L, k)
    for indexed in (False, True):
        r2 = oc.synthesize(A_pyr, Ap_list, B_pyr, [b.copy() for b in Bp_pyr], L, k, w, indexed=indexed)
        assert set(r1) == set(r2) == set(range(1, L))
        for l in r1:
            for a, b in zip(r1[l], r2[l]):
                assert np.array_equal(a, b), (l, indexed)


def _tie_cases(nch):
    """Label-map and constant-A inputs (tests/test_gpu_fallback.py) as oracle pyramids: flat
    regions whose rows and queries tie exactly, and a database of identical rows."""
    import test_gpu_fallback as fb
    if nch == 1:
        for images in (fb.label_inputs(5, (24, 32), (20, 24), 2, band=2, patch=6, same_bg=True),
                       fb.degenerate_inputs('const_exact', 6, (24, 32), (20, 24)),
                       fb.degenerate_inputs('const_round', 6, (24, 32), (20, 24))):
            yield o.setup_luminance(*images, seed=5)
    else:
        yield fb.colour_label_inputs(5, (24, 32), (20, 24), 2, band=2, patch=6)
        A = np.dstack([np.full((24, 32), v) for v in (0.25, 0.5, 0.75)])
        B = np.dstack([fb.smooth_noise(7 + 17 * ch, (20, 24)) for ch in range(3)])
        A_pyr, Ap_list, B_pyr, _, L = fb.colour_pyramids(A, [np.full((24, 32, 3), 0.5)], B)
        yield A_pyr, Ap_list, B_pyr, o.initialize_Bp(B_pyr, True, 7), L


@pytest.mark.parametrize('nch', [1, 3])
def test_c_oracle_equals_numpy_oracle_on_exact_ties(nch):
    """The checker of the GPU full-scan tests (test_gpu_fallback.py) on its own inputs, 1 and 3
    channels: with flat regions tying hundreds of rows exactly, and with every row of the
    database identical, the C oracle (scan and projection index) equals the numpy oracle."""
    w = o.compute_weights(3, 5, 12, nch)
    for A_pyr, Ap_list, B_pyr, Bp_pyr, L in _tie_cases(nch):
        r1 = o.synthesize(A_pyr, Ap_list, B_pyr, [b.copy() for b in Bp_pyr], L, 1.0)
        for indexed in (False, True):
            r2 = oc.synthesize(A_pyr, Ap_list, B_pyr, [b.copy() for b in Bp_pyr], L, 1.0, w, indexed=indexed)
            assert set(r1) == set(r2) == set(range(1, L))
            for l in r1:
                for a, b in zip(r1[l], r2[l]):
                    assert np.array_equal(a, b), (l, indexed)


@pytest.mark.parametrize('nch', [1, 3])
def test_oracle_index_takes_lowest_row_of_a_large_tie(nch):
    """The projection index on a label-map level (A 128 x 160, two A' images of one
    background: 40,960 rows, most of them one bit-identical flat row): for the flat row
    itself, nudged copies of it and textured rows, the index returns the brute-force scan's
    row and distance, and for the flat queries that row is the LOWEST of thousands of tied
    rows."""
    import test_gpu_fallback as fb
    if nch == 1:
        A, Aps, _ = fb.label_inputs(8, (128, 160), (8, 8), 2, band=3, patch=40, same_bg=True)
        A_pyr = o.compute_gaussian_pyramid(A, 3, 1)
        Ap_list = [o.compute_gaussian_pyramid(x, 3, 1) for x in Aps]
    else:
        A_pyr, Ap_list, _, _, _ = fb.colour_label_inputs(8, (128, 160), (8, 8), 2, band=3, patch=40, cap=1)
    db = oc.LevelDB(1, A_pyr, Ap_list)
    assert db.N == 40960
    flat = db.rows[db.N - 1]
    tied = np.flatnonzero((db.rows == flat).all(axis=1))
    assert len(tied) > 5000 and tied[0] > 0           # (the top band: row 0 is textured)
    rs = np.random.RandomState(9)
    Q = np.vstack([flat[None], flat + rs.randn(8, db.D) * 1e-9, flat + rs.randn(8, db.D) * 0.05,
                   db.rows[rs.randint(0, tied[0], 8)], db.rows[tied[rs.randint(0, len(tied), 8)]]])
    i0, d0 = db.scan(Q)
    assert i0[0] == tied[0] and d0[0] == 0.0 and (i0[-8:] == tied[0]).all()
    d = np.add.reduce((db.rows - Q[3]) ** 2, axis=1)
    assert i0[3] == np.argmin(d) and d0[3] == d.min()
    for P in (1, 4):
        i1, d1 = db.index(P).nn(Q)
        assert np.array_equal(i0, i1) and np.array_equal(d0, d1), P
    if nch == 1:
        i2, d2 = db.nn(Q)
        assert np.array_equal(i0, i2) and np.array_equal(d0, d2)


# ---- the inputs of tests/test_gpu_shards.py tie across the ranks as they claim -----------------
# (the oracle, numpy and the library's host-only geometry calls; floors of 100 finest-level
# queries, as the one-GPU tie tests use: B's flat half is 384 of 768 pixels)

def _rank_ties(name, world):
    """Per rank: the tied segments per finest-level query of the rank's shard (shard_ties)."""
    import test_gpu_shards as sh
    return [sh.shard_ties(name, r, world)[0] for r in range(world)]


@pytest.mark.parametrize('name,world', [('tie2@small', 2), ('tie2@small', 3), ('over@shards', 2),
                                        ('linear@image', 2)])
def test_shard_inputs_tie_across_ranks_with_the_winner_on_rank_0(name, world):
    """At least 100 queries whose nearest row has bit-identical copies in two or more ranks'
    row ranges, the oracle's winner (the lowest row) in rank 0's."""
    import test_gpu_shards as sh
    case = sh.shard_case(name)
    held = np.array([t > 0 for t in _rank_ties(name, world)])
    across = held.sum(axis=0) >= 2
    end0 = sum(sh.shard_rows(len(case.rows), 0, world))
    print('%s world %d: %d queries tied across ranks, %d of them won on rank 0'
          % (name, world, across.sum(), (case.nn[across] < end0).sum()))
    assert across.sum() >= 100 and (case.nn[across] < end0).all()
    if name == 'over@shards':   # each rank's candidate list overflows
        for t in _rank_ties(name, world):
            assert (t > 1024).sum() >= 100, (t > 1024).sum()


def test_shard_input_tie_late_wins_on_rank_1_with_nothing_on_rank_0():
    """tie_late@small over 3 ranks: at least 100 queries whose tied rows lie on ranks 1 and 2
    and nowhere in rank 0's range; the winner in rank 1's; rank 2's rows are all one row."""
    import test_gpu_shards as sh
    case = sh.shard_case('tie_late@small')
    t0, t1, t2 = _rank_ties('tie_late@small', 3)
    late = (t0 == 0) & (t1 > 0) & (t2 > 0)
    N = len(case.rows)
    r1, n1 = sh.shard_rows(N, 1, 3)
    r2, n2 = sh.shard_rows(N, 2, 3)
    print('tie_late@small: %d late queries' % late.sum())
    assert late.sum() >= 100
    assert ((case.nn[late] >= r1) & (case.nn[late] < r1 + n1)).all()
    assert (case.rows[r2:r2 + n2] == case.rows[r2]).all()


@pytest.mark.parametrize('name', ['straddle@strip', 'over@shards'])
def test_shard_inputs_middle_rank_straddles_the_image_boundary(name):
    """Over 3 ranks the middle rank's range contains the image boundary Ah Aw, its shard is in
    strip order, and at least 100 queries tie over two or more of its segments on each side of
    the boundary; over@shards stays at or below 1024 tied segments on every rank."""
    import test_gpu_shards as sh
    case = sh.shard_case(name)
    Ah, Aw = case.pyr[0][case.L - 1].shape
    N = len(case.rows)
    row0, nrows = sh.shard_rows(N, 1, 3)
    assert N == 2 * Ah * Aw and row0 < Ah * Aw < row0 + nrows
    import ctypes
    import _ia
    m = (ctypes.c_int * 3)()
    _ia.check(_ia.lib().ia_diag_stage_map(row0, nrows, Aw, Ah, m), 'ia_diag_stage_map')
    assert m[0] == Aw
    lo = sh.shard_ties(name, 1, 3, keep=lambda g: g < Ah * Aw)
    hi = sh.shard_ties(name, 1, 3, keep=lambda g: g >= Ah * Aw)
    assert np.array_equal(lo + hi, sh.shard_ties(name, 1, 3)[0])
    both = (lo >= 2) & (hi >= 2)
    print('%s: %d queries tied over >= 2 segments on each side (most %d + %d)' % (name, both.sum(), lo.max(), hi.max()))
    assert both.sum() >= 100
    if name == 'over@shards':
        assert max(t.max() for t in _rank_ties(name, 3)) <= 1024


def test_shard_input_padded_ties_with_each_shards_last_row():
    """padded@shards over 2 ranks: each shard's rows do not fill its chunks, and at least 100
    queries' nearest row is bit-identical to the shard's last real row, which its padding
    repeats."""
    import _ia
    import test_gpu_shards as sh
    case = sh.shard_case('padded@shards')
    N = len(case.rows)
    for r in range(2):
        row0, nrows = sh.shard_rows(N, r, 2)
        assert _ia.lib().ia_db_rows_padded(nrows) > nrows
        want = int((case.rows[case.nn] == case.rows[row0 + nrows - 1]).all(axis=1).sum())
        ties, nseg = sh.shard_ties('padded@shards', r, 2)
        print('padded@shards rank %d: %d queries tied with the last row, over at most %d of %d segments'
              % (r, want, ties.max(), nseg))
        assert want >= 100 and ties.max() <= 1024


# ---- the inputs of tests/test_gpu_bounds.py have teeth (numpy and the oracle only) -------------

@pytest.mark.parametrize('n', [55, 165])
def test_bound_rotations_are_what_they_claim(n):
    """rotation_of (the stand-in for algorithms._eigh): every rotation passes the builders'
    orthonormality check once rounded to fp32 (||V^T V - I||_F <= 2 sqrt(n) 2^-24), w is the
    variance along each column, 'reversed' holds the principal directions by increasing
    variance after the builders' flip, 'identity' the unit matrix, and no two coincide."""
    import test_gpu_bounds as gb
    X = np.random.RandomState(3).standard_normal((4 * n, n)) * np.linspace(0.1, 3.0, n)
    C = X.T @ X / len(X)
    held = {}
    for kind in ('principal',) + gb.ROTATIONS:
        w, V = gb.rotation_of(kind, C)
        R = gb.held_rotation(V).astype(np.float64)
        dev = np.linalg.norm(R.T @ R - np.eye(n))
        print('rotation %s (n = %d): ||V^T V - I||_F = %.2g of %.2g' % (kind, n, dev, 2 * np.sqrt(n) * 2.0 ** -24))
        assert dev <= 2 * np.sqrt(n) * 2.0 ** -24
        assert np.allclose(w, np.einsum('ij,ij->j', V, C @ V), rtol=1e-9)
        held[kind] = R
    var = lambda R: np.einsum('ij,ij->j', R, C @ R)  # noqa: E731
    assert (np.diff(var(held['principal'])) <= 1e-12).all()
    assert (np.diff(var(held['reversed'])) >= -1e-12).all()
    assert np.array_equal(held['reversed'], held['principal'][:, ::-1])
    assert np.array_equal(held['identity'], np.eye(n))
    kinds = sorted(held)
    for i, a in enumerate(kinds):
        for b in kinds[i + 1:]:
            assert np.abs(held[a] - held[b]).max() > 0.1, (a, b)


@pytest.mark.parametrize('data', ['smooth', 'white', 'outlier'])
def test_bound_inputs_need_the_skip_term(data):
    """The rotated screen restated in numpy (emulate_screen: f16 hi parts only for the
    components >= P, exact products, the library's scales and segment order) on the 256 x 512
    level and the queries of test_r16_bound_under_rotation: under every non-principal rotation
    the worst |segment minimum - fp64| exceeds 2 eps_0 (the bound without its skip term), and
    eps_R still holds it.  A kernel that dropped or understated the skip term cannot pass
    those inputs.  Measured: smooth 50 / 27 / 31 eps_0 (reversed / identity / random; 0.70 /
    0.41 / 0.45 eps_R), white 27 / 23 / 27 (0.49 / 0.42 / 0.49), outlier 7.9 / 2.9 / 7.7
    (0.50 / 0.25 / 0.49); the principal basis: 6.7, 25 and 7.0 eps_0 with the worst-case
    queries, 1.7, 12.5 and 3.8 without."""
    import test_gpu_bounds as gb
    lv = gb.bound_level(data)
    order, seg = gb.segment_order(len(lv.As), *lv.A_pyr[1].shape)
    assert len(lv.As) == 131072 and len(order) // seg == 512
    for kind in gb.ROTATIONS:
        V = gb.held_rotation(gb.rotation_of(kind, lv.cov())[1])
        Q = lv.queries(kind)
        assert Q.shape == (342, 55)
        r = gb.emulate_screen(lv.As, lv.center, lv.amax, Q, order, seg, V)
        err = np.abs(r['m'] - r['x'])
        w0, wR = (err / r['eps0'][:, None]).max(), (err / r['epsR'][:, None]).max()
        w64 = (err[:64] / r['eps0'][:64, None]).max()
        print('emulated r16 screen [%s, %s]: A_skip / A = %.3f, worst error %.3g eps_0 (first 64 queries '
              '%.3g), %.3g eps_R' % (data, kind, r['askip'] / lv.amax, w0, w64, wR))
        assert w0 >= 2.0 and w64 >= 2.0
        assert wR < 1.0


def test_strip_case_needs_the_skip_term_end_to_end():
    """The strip case of test_strip_synthesis_under_rotation under the reversed rotation, with
    the oracle's own queries: for 6 of the 768 finest-level queries (at least 3 are asked) an
    exact stage that tested m_j <= e* + 2 eps_0 would drop the true winner's segment, while
    eps_R keeps it; the comparison with the oracle can therefore see a lost skip term."""
    import test_gpu_bounds as gb
    n, total = gb.affected_queries(gb.e2e_case('strip'))
    print('strip case, reversed rotation: %d of %d queries lose their winner under eps_0 alone' % (n, total))
    assert n >= 3


@pytest.mark.parametrize('data', ['white', 'outlier'])
def test_split16_inputs_stay_inside_eps16_with_flush(data):
    """The split-f16 screen restated in numpy on the 128 x 256 level of
    test_split16_bound_on_white_and_outlier_data, with f16 subnormals kept and flushed to
    zero: the representation error stays below eps16 (a correct kernel passes), and on the
    outlier data most scaled lo parts are f16 subnormals (the flush allowance is exercised)."""
    import test_gpu_bounds as gb
    from test_gpu_split16 import _scales
    lv = gb.bound_level(data, (128, 256))
    order, seg = gb.segment_order(len(lv.As), *lv.A_pyr[1].shape)
    for flush in (False, True):
        r = gb.emulate_screen(lv.As, lv.center, lv.amax, lv.Q, order, seg, None, flush=flush)
        worst = (np.abs(r['m'] - r['x']) / r['eps0'][:, None]).max()
        print('emulated split16 screen [%s, flush %s]: worst error %.3g eps16' % (data, flush, worst))
        assert worst < 1.0
    if data == 'outlier':
        al = gb.f16_split(np.ldexp((lv.As - lv.center).astype(np.float32).astype(np.float64),
                                   _scales(lv.amax, 0.0)[0]))[1]
        sub = float(((np.abs(al) < 2.0 ** -14) & (al != 0)).mean())
        print('outlier data: %.1f %% of the scaled lo parts are f16 subnormals' % (100 * sub))
        assert sub > 0.5


# ---- LSH restatement (this build's definition, no reference code) -------

def test_lsh_keys_kat():
    """One table, one axis-aligned projection, b = 0, w = 1: key = floor(x0) * golden."""
    proj = np.zeros((1, 56), np.float32)
    proj[0, 0] = 1.0
    X = np.zeros((4, 55), np.float32)
    X[:, 0] = [0.5, 1.5, -0.5, 7.0]
    keys = o.lsh_hash_keys(X, proj, 1, 1, 1.0)[:, 0]
    want = [(h * 0x9E3779B1) & 0x7fffffff for h in (0, 1, 0xffffffff, 7)]
    assert [o.lsh_bits(n) for n in (1, 2, 3, 1024, 1025, 1 << 40)] == [2, 2, 3, 11, 12, 30]
    assert keys.tolist() == want


def test_lsh_single_bucket_is_bruteforce():
    """A bucket wider than the data holds every row: with N <= cap the LSH matcher is the
    exact first-minimum brute force."""
    rs = np.random.RandomState(0)
    As = rs.rand(30, 55)
    proj = np.zeros((2, 56), np.float32)
    proj[:, :55] = rs.randn(2, 55)
    proj[:, 55] = 5e5      # offset b = w / 2 keeps every |p . x| << w in bucket 0
    Q = np.vstack([As[:5], rs.rand(20, 55)])
    idx, dist = o.lsh_match(As, As.mean(0), proj, 1, 2, 1e6, Q)
    for q, i, d in zip(Q, idx, dist):
        dd = np.add.reduce((As - q) ** 2, axis=1)
        assert i == np.argmin(dd) and d == dd.min()


def test_lsh_recall_on_perturbed_rows():
    """Sanity of the definition: near-duplicate queries find their row (or an equally
    close one) in most cases with the default 16 x 4 tables."""
    A, Aps, _ = analogy_inputs(4, (40, 50), (8, 8))
    pyr = o.compute_gaussian_pyramid(A, 3)
    ppyr = o.compute_gaussian_pyramid(Aps[0], 3)
    As = o.create_index(pyr, [ppyr], len(pyr))[-1]
    c = As.mean(0)
    rs = np.random.RandomState(1)
    sigma = np.sqrt(((As - c) ** 2).mean())
    P = np.zeros((64, 56), np.float32)
    P[:, :55] = rs.standard_normal((64, 55))
    P[:, 55] = rs.uniform(0, sigma, 64)
    rows = rs.randint(0, len(As), 200)
    Q = As[rows] + rs.randn(200, 55) * 1e-3 * sigma
    idx, dist = o.lsh_match(As, c, P, 16, 4, sigma, Q)
    exact = np.array([np.add.reduce((As - q) ** 2, axis=1).min() for q in Q])
    assert np.all(dist >= exact)
    assert np.mean(dist == exact) > 0.9


def test_c3_fixture_reproduces_coarse_levels():
    """tests/golden/c3_oracle.npz (make_config_fixtures.py c3) re-derived here for its
    three coarsest synthesized levels from bench.py's c3 inputs."""
    import hashlib
    import sys
    import ia_oracle_c as oc
    from conftest import ROOT
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import bench
    g = golden('c3_oracle.npz')
    conf = bench.CONFIGS['c3']
    A, Ap, B = bench.make_inputs(conf, 0)
    A_pyr, Ap_list, B_pyr, Bp_pyr, L = o.setup_luminance(A, [Ap], B, cap=conf['levels'], seed=2)
    assert L == int(g['max_levels'])
    out = oc.synthesize(A_pyr, Ap_list, B_pyr, Bp_pyr, L, conf['k'],
                        o.compute_weights(3, 5, 12, 1), levels=[1, 2, 3])
    for l, (bp, s, im) in out.items():
        assert np.array_equal(s, g['s%d' % l]) and np.array_equal(im, g['im%d' % l])
        assert hashlib.sha256(bp.tobytes()).hexdigest() == str(g['bp_sha%d' % l])


@pytest.mark.parametrize('full', [True, False])
def test_level_features_3ch_match_extract_patches_2d(full):
    """The oracle's 3-channel feature rows equal the reference's construction
    (algorithms.py:11-47): symmetric np.pad, sklearn extract_patches_2d, flatten, the
    c.num_ch * c.n_half cut of the fine half, coarse patch at (row // 2) * ceil(w / 2) +
    col // 2."""
    from sklearn.feature_extraction.image import extract_patches_2d
    rs = np.random.RandomState(5)
    lg = rs.rand(9, 12, 3)
    sm = rs.rand(5, 6, 3)
    pad = lambda x, p: np.pad(x, ((p, p), (p, p), (0, 0)), mode='symmetric')  # noqa: E731
    psm = extract_patches_2d(pad(sm, 1), (3, 3))
    plg = extract_patches_2d(pad(lg, 2), (5, 5))
    plg = plg.reshape(plg.shape[0], -1)
    if not full:
        plg = plg[:, :3 * 12]
    h, w = lg.shape[:2]
    ref = np.vstack([np.hstack([psm[(r // 2) * int(np.ceil(w / 2.)) + c // 2].flatten(),
                                plg[r * w + c].flatten()])
                     for r in range(h) for c in range(w)])
    got = o.level_features(sm, lg, full)
    assert got.shape == ref.shape and np.array_equal(got, ref)


# ---- the projection index the full-size fixtures were generated through ------------------

def _fixture_module():
    import os
    import sys
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
    if here not in sys.path:
        sys.path.insert(0, here)
    import make_config_fixtures as mf
    return mf


def test_oracle_index_equals_scan_at_c4_scale():
    """c4_full.npz was generated through the oracle's projection index.  On
    c4's finest level (4,194,304 rows, bench.py's seed-0 inputs) the index must return the
    brute-force scan's row and distance for every committed c4 query (512 captured from a
    GPU synthesis + 64 near-ties; c4_queries.npz holds the scan's answers,
    make_config_fixtures.make_c4), at P = 1 and P = 4 projections (~20 s on 8 threads)."""
    mf = _fixture_module()
    prev = oc.set_threads(8)
    try:
        A, Aps, B, k, cap, seed = mf.workload('c4')
        A_pyr = o.compute_gaussian_pyramid(A, 3, cap)
        Ap_pyr = o.compute_gaussian_pyramid(Aps[0], 3, cap)
        db = oc.LevelDB(len(A_pyr) - 1, A_pyr, [Ap_pyr])
        assert db.N == 4194304
        f = golden('c4_queries.npz')
        for P in (1, 4):
            ix = db.index(P)
            idx, d = ix.nn(f['q'])
            del ix
            assert np.array_equal(idx, f['idx']), P
            assert np.array_equal(d, f['dist']), P
    finally:
        oc.set_threads(prev)


def test_colour_index_equals_scan_165_dims():
    """the index's rounding margin for 165-dim rows.  Random rows, exact
    duplicates, 1e-12 near-ties and nudged rows of a 3-channel level: index == scan."""
    rs = np.random.RandomState(11)
    mf = _fixture_module()
    A_pyr, Ap_list, B_pyr, Bp_pyr, L, k = mf.colour_workload('c1rgb')
    db = oc.LevelDB(L - 1, A_pyr, Ap_list)
    assert db.D == 165
    N = db.N
    Q = np.vstack([db.rows[rs.randint(0, N, 16)], db.rows[rs.randint(0, N, 16)] + 1e-12,
                   db.rows[rs.randint(0, N, 16)] + rs.randn(16, 165) * 1e-3, rs.rand(8, 165)])
    i0, d0 = db.scan(Q)
    for P in (1, 4):
        i1, d1 = db.index(P).nn(Q)
        assert np.array_equal(i0, i1) and np.array_equal(d0, d1), P


def test_colour_fixture_equals_brute_force_scan():
    """c1rgb_oracle.npz (generated through the projection index) re-derived with the
    brute-force scan at every level: s, im and the B' hash (~60 s on 8 threads)."""
    mf = _fixture_module()
    prev = oc.set_threads(8)
    try:
        A_pyr, Ap_list, B_pyr, Bp_pyr, L, k = mf.colour_workload('c1rgb')
        w = o.compute_weights(3, 5, 12, 3)
        out = oc.synthesize(A_pyr, Ap_list, B_pyr, Bp_pyr, L, k, w, indexed=False)
    finally:
        oc.set_threads(prev)
    f = golden('c1rgb_oracle.npz')
    assert sorted(out) == list(range(1, int(f['max_levels'])))
    for l, (bp, s, im) in out.items():
        assert np.array_equal(s.astype(np.int16), f['s%d' % l]), l
        assert np.array_equal(im.astype(np.uint8), f['im%d' % l]), l
        assert mf.bp_hash(bp) == str(f['bp_sha%d' % l]), l
