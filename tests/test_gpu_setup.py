"""The reference's setup options on the device, against the oracle: remap_lum (A and A' leave
[0, 1]), AB_weight != 1 (the A/B half of every row on another scale than the A'/B' half) and
init_rand=False (B' starts as B's pyramid, built before the compression), through setup_dev,
every form of the exact stage, a batch, the colour matcher and image_analogies_main; the
pyramid kernels on data outside [0, 1] with warp's clip ENGAGED (plateau images on odd sizes:
the resampled plateaus round past the blurred extremes, which each test asserts from the
oracle alone); the reference's own pyramids of those inputs (tests/golden/
ref_setup_golden.npz); and the elementwise kernels at their block edges.

Every comparison is bit-exact.  The generators (plateau, noise_image) live in
tests/golden/make_setup_golden.py, which also writes the fixture; the reference-only helpers
here (unclipped_reduce, clip_counts, reference_setup, option_case) need no GPU and are shared
with the CPU tests of test_oracle.py."""
import math
import sys
import types

import numpy as np
import pytest

import ia_oracle as o
from conftest import GOLDEN, analogy_inputs, golden
from test_gpu_fallback import LumCase, assert_case, dev, dev_job, form  # noqa: F401 (form: a fixture)

if GOLDEN not in sys.path:
    sys.path.insert(0, GOLDEN)
import make_setup_golden as msg  # noqa: E402
from make_setup_golden import noise_image, plateau  # noqa: E402

pytestmark = pytest.mark.gpu


# ---- reference-only helpers --------------------------------------------------------------------

def unclipped_reduce(img):
    """(blurred image, its bilinear resample WITHOUT warp's clip): o.bilinear_resize up to its
    last line, restated so that the oracle itself stays as it is."""
    h, w = img.shape
    out_shape = (math.ceil(h / 2.0), math.ceil(w / 2.0))
    sm = o.gaussian_blur(img)
    sx, tx, sy, ty = o.affine_coeffs((h, w), out_shape)
    c = np.arange(out_shape[1], dtype=np.float64) * sx + tx
    r = np.arange(out_shape[0], dtype=np.float64) * sy + ty
    minr, maxr = np.floor(r).astype(np.int64), np.ceil(r).astype(np.int64)
    minc, maxc = np.floor(c).astype(np.int64), np.ceil(c).astype(np.int64)
    dr, dc = (r - minr)[:, None], (c - minc)[None, :]
    r0, r1 = o.mirror_index(minr, h)[:, None], o.mirror_index(maxr, h)[:, None]
    c0, c1 = o.mirror_index(minc, w)[None, :], o.mirror_index(maxc, w)[None, :]
    top = (1 - dc) * sm[r0, c0] + dc * sm[r0, c1]
    bot = (1 - dc) * sm[r1, c0] + dc * sm[r1, c1]
    return sm, (1 - dr) * top + dr * bot


def clip_counts(img):
    """(values the oracle's clip raised to the blurred minimum, values it lowered to the blurred
    maximum) in pyramid_reduce(img); also checks that the restated resample is the oracle's."""
    sm, raw = unclipped_reduce(img)
    ref = o.pyramid_reduce(img)
    assert np.array_equal(np.clip(raw, sm.min(), sm.max()).view(np.int64), ref.view(np.int64))
    changed = raw != ref
    return int((changed & (raw < sm.min())).sum()), int((changed & (raw > sm.max())).sum())


# which side of the clip a plateau pair must engage (a zero bound cannot: every blurred value
# and every bilinear sample of values >= 0 is >= 0, likewise <= 0; (255, 3) was measured to
# engage on the high side only)
PLATEAU_SIDES = {'mixed': (True, True), 'u8': (False, True), 'zero_hi': (True, False), 'zero_lo': (False, True)}
PLATEAU_SHAPES = [(45, 61), (21, 37), (117, 181), (257, 124)]
# (1 x 61: the two-kernel path k_blur + k_resample, whose clip is its own; 2 x 61: k_pyr_reduce
# under either form; only the mixed pair engages there)
THIN_SHAPES = [(1, 61), (2, 61)]
PLATEAU_CASES = [(n, s) for n in sorted(msg.PLATEAUS) for s in PLATEAU_SHAPES] + [('mixed', s) for s in THIN_SHAPES]
NOISE_SHAPES = [(96, 130), (8, 4), (33, 70), (4, 5), (5, 300)]


def plateau_image(name, shape):
    hi, lo = msg.PLATEAUS[name]
    return plateau(shape, hi, lo, sum(shape))


def assert_clip_engaged(name, img):
    low, high = clip_counts(img)
    want_low, want_high = PLATEAU_SIDES[name]
    print('plateau %s %s: oracle clips %d low, %d high' % (name, img.shape, low, high))
    assert (low > 0 or not want_low) and (high > 0 or not want_high), (name, img.shape, low, high)


SETUPS = {
    'plain': {},
    'remap': dict(remap_lum=True),
    'ab_small': dict(AB_weight=0.25),
    'ab_large': dict(AB_weight=4.0),
    'init_b': dict(init_rand=False),
    'all': dict(remap_lum=True, AB_weight=0.5, init_rand=False),
}
OPTION_SIZES = {'small': ((40, 52), (24, 31), None, 2), 'strip': ((256, 512), (12, 30), 1, 1)}
_CASES = {}


def option_case(name):
    """'<setup>@<size>': the oracle run of analogy_inputs(93, ...) under SETUPS[<setup>], once
    per module ('small': every level, two A'; 'strip': a 131,072-row strip level, one A')."""
    if name not in _CASES:
        kind, size = name.split('@')
        A_shape, B_shape, cap, n_ap = OPTION_SIZES[size]
        _CASES[name] = LumCase(analogy_inputs(93, A_shape, B_shape, n_ap), cap, 1.0, 93, tie=False,
                               setup=SETUPS[kind])
    return _CASES[name]


def assert_differs_from_plain(name):
    """The option changes the oracle's result: a product that ignored it would fail."""
    case, plain = option_case(name), option_case('plain@' + name.split('@')[1])
    l = case.L - 1
    n = int((case.ref[l][1] != plain.ref[l][1]).any(axis=1).sum())
    print('%s: %d of %d finest-level pixels differ from the plain run' % (name, n, len(case.ref[l][1])))
    assert n > 0


def image_scale(x):
    """image_analogies.py:32-37."""
    return 255. if np.max(x) > 1.0 else 1.0


def reference_setup(A, Aps, B, convert, AB_weight=1, remap_lum=False, init_rand=True, cap=None, seed=0):
    """img_setup's numeric part from the oracle: (A_pyr, Ap_list, B_pyr, Bp_pyr, colour pyramids,
    max_levels).  The A' scale comes from the first row of the LAST A'."""
    sA, sB, sAp = image_scale(A), image_scale(B), image_scale(Aps[-1][0])
    f64 = lambda x, s: np.asarray(x / s, dtype=np.float64)  # noqa: E731  (uint8 / 255. is fp64 already)
    if convert:
        B_yiq = o.convert_to_YIQ(f64(B, sB))
        Ay, By = o.convert_to_YIQ(f64(A, sA))[..., 0], B_yiq[..., 0]
        Apy = [o.convert_to_YIQ(f64(x, sAp))[..., 0] for x in Aps]
    else:
        Ay, By, Apy = f64(A, sA), f64(B, sB), [f64(x, sAp) for x in Aps]
    A_pyr, Ap_list, B_pyr, Bp_pyr, L = o.setup_luminance(Ay, Apy, By, AB_weight, remap_lum, cap=cap,
                                                         init_rand=init_rand, seed=seed)
    colour = [o.compute_gaussian_pyramid(B_yiq, 3, cap)] if convert else Ap_list
    return A_pyr, Ap_list, B_pyr, Bp_pyr, colour, L


def to_rgb(x):
    return np.dstack([x, x * 0.8 + 0.1, 1 - x])


def as_dtype(x, dtype):
    if dtype == 'uint8':
        return np.round(255 * x).astype(np.uint8)
    return x.astype(dtype)


# (dtype, convert, remap_lum, AB_weight, init_rand, levels): every value of every option, the
# all-on case with and without convert
SETUP_GRID = [
    ('uint8', True, False, 1, True, None),
    ('uint8', True, True, 0.25, False, 2),
    ('float32', True, True, 4.0, True, None),
    ('float64', True, False, 0.25, False, None),
    ('float64', True, True, 1, False, 2),
    ('float32', True, False, 4.0, False, 2),
    ('uint8', False, False, 4.0, True, None),
    ('float32', False, True, 0.25, True, 2),
    ('float64', False, True, 4.0, False, None),
    ('uint8', False, False, 1, False, 2),
    ('float64', False, False, 1, True, None),
    ('float32', False, False, 0.25, False, None),
]


def setup_images(dtype, convert, seed=41):
    A, Aps, B = analogy_inputs(seed, (40, 52), (24, 31), n_ap=2)
    lift = to_rgb if convert else (lambda x: x)
    return as_dtype(lift(A), dtype), [as_dtype(lift(x), dtype) for x in Aps], as_dtype(lift(B), dtype)


def config(**kw):
    """A parameter namespace like the config module's."""
    c = types.SimpleNamespace(convert=False, remap_lum=False, init_rand=True, AB_weight=1, k=1.0, n_sm=3,
                              levels=None, seed=0, matcher='brute')
    c.__dict__.update(kw)
    return c


# ---- 1. pyramid kernels outside [0, 1], the clip engaged ----------------------------------------

def both_forms(img):
    """pyramid_reduce_dev under the tiled form (0) and the one-pass form (1)."""
    import _ia
    import img_preprocess as ip
    x = dev(img)
    outs = []
    for f in (0, 1):
        prev = _ia.pyr_form(f, 16)
        try:
            outs.append(ip.pyramid_reduce_dev(x).cpu().numpy())
        finally:
            _ia.pyr_form(prev, 16)
    return outs


def assert_reduce(img):
    ref = o.pyramid_reduce(img)
    tiled, wave = both_forms(img)
    assert np.array_equal(tiled, ref)
    assert np.array_equal(wave, ref)
    assert np.array_equal(tiled.view(np.int64), wave.view(np.int64))


@pytest.mark.parametrize('name,shape', PLATEAU_CASES)
def test_pyramid_clip_engaged_vs_oracle(gpu, name, shape):
    """Plateau images on odd sizes: the oracle's clip changes values (asserted from the oracle
    alone, on the side(s) the pair can engage), so the rewrite branches of k_pyr_clip_p and
    k_pyr_clip (1 x 61: k_resample's clip) run.  Both forms equal the oracle and each other
    bit for bit, the pairs with a bound of exactly 0.0 included."""
    img = plateau_image(name, shape)
    assert_clip_engaged(name, img)
    assert_reduce(img)


@pytest.mark.parametrize('shape', NOISE_SHAPES)
@pytest.mark.parametrize('kind', msg.NOISE)
def test_pyramid_out_of_range_noise_vs_oracle(gpu, kind, shape):
    """Noise of mixed sign, all negative, 0 .. 255 and -0.47 .. 1.24 through k_pyr_wave<true>,
    k_pyr_wave<false> and the tiled k_pyr_reduce: the order-preserving keys and the fmin / fmax
    partials on data that is not in [0, 1]."""
    assert_reduce(noise_image(kind, shape, sum(shape) + 1))


@pytest.mark.parametrize('cap', [None, 2])
def test_full_pyramid_of_mixed_sign_plateau(gpu, cap):
    import img_preprocess as ip
    img = plateau_image('mixed', (117, 181))
    ref = o.compute_gaussian_pyramid(img, 3, cap)
    got = ip.compute_gaussian_pyramid(img, 3, cap)
    assert len(got) == len(ref) == (3 if cap else 6)
    for a, b in zip(got, ref):
        assert np.array_equal(a.view(np.int64), b.view(np.int64))


# ---- 2. the reference's own outputs -------------------------------------------------------------

def test_reference_fixture_pyramids_on_device(gpu):
    """ref_setup_golden.npz (the reference's pyramids of the plateau and out-of-range images,
    and its remap + compress + pyramid chain): the kernels reproduce every array."""
    import img_preprocess as ip
    g = golden('ref_setup_golden.npz')
    for name, img in msg.golden_images().items():
        assert msg.sha(img) == str(g[name + '_sha']), name
        pyr = ip.compute_gaussian_pyramid(img, 3)
        assert len(pyr) == int(g[name + '_n']), name
        for l in range(len(pyr) - 1):
            assert np.array_equal(pyr[l], g['%s_l%d' % (name, l)]), (name, l)
    A, Ap, B = msg.chain_inputs()
    assert [msg.sha(x) for x in (A, Ap, B)] == [str(s) for s in g['chain_sha']]
    Ar, Apr = ip.remap_luminance(A, [Ap], B)
    Ac, Bc = ip.compress_values(Ar, B, msg.CHAIN_WEIGHT)
    for name, img in (('A', Ac), ('Ap', Apr[0]), ('B', Bc)):
        pyr = ip.compute_gaussian_pyramid(img, 3)
        assert len(pyr) == int(g['chain_%s_n' % name]), name
        for l, lvl in enumerate(pyr):
            assert np.array_equal(lvl, g['chain_%s_l%d' % (name, l)]), (name, l)


# ---- 3. elementwise kernels at block edges --------------------------------------------------------

EDGE_COUNTS = [1, 255, 256, 257, 65537]


def typed(rs, shape, dtype, div):
    """Values x of the dtype with x / div in [0, 1]."""
    if dtype == np.uint8:
        return rs.randint(0, 256 if div == 255 else 2, size=shape).astype(np.uint8)
    return (div * rs.rand(*shape)).astype(dtype)


@pytest.mark.parametrize('n', EDGE_COUNTS)
def test_yiq_and_scale_kernels_at_block_edges(gpu, n):
    import torch
    import img_preprocess as ip
    rs = np.random.RandomState(n)
    for dtype in (np.uint8, np.float32, np.float64):
        for div in (255.0, 1.0):
            x = typed(rs, (1, n, 3), dtype, div)
            ref = o.convert_to_YIQ(x.astype(np.float64) / div)
            xd = torch.as_tensor(x).to('cuda')
            for want in (True, False):
                yiq, y = ip.rgb_to_yiq_dev(xd, div, want_yiq=want)
                assert (yiq is not None) == want
                assert np.array_equal(y.cpu().numpy(), ref[..., 0]), (dtype, div, want)
                if want:
                    assert np.array_equal(yiq.cpu().numpy(), ref), (dtype, div)
            g = typed(rs, (1, n), dtype, div)
            got = ip.scale_dev(torch.as_tensor(g).to('cuda'), div)
            assert got.dtype == torch.float64 and tuple(got.shape) == (1, n)
            assert np.array_equal(got.cpu().numpy(), g.astype(np.float64) / div), (dtype, div)


@pytest.mark.parametrize('n', EDGE_COUNTS)
def test_axpb_and_rgb_kernels_at_block_edges(gpu, n):
    import img_preprocess as ip
    rs = np.random.RandomState(n + 1)
    x = 2.5 * rs.rand(1, n) - 1.2
    ratio, m, b = 1.7320508, 0.4321, -0.25
    assert np.array_equal(ip._axpb_dev(dev(x), 0, ratio).cpu().numpy(), ratio * x)
    assert np.array_equal(ip._axpb_dev(dev(x), 1, ratio, m, b).cpu().numpy(), ratio * (x - m) + b)
    yiq = 2.0 * rs.rand(1, n, 3) - 0.5
    assert np.array_equal(ip.convert_to_RGB(yiq), o.convert_to_RGB(yiq))


@pytest.mark.parametrize('n', EDGE_COUNTS)
def test_color_output_convert_branch_at_block_edges(gpu, n):
    """ia_color_output with convert: B' as Y and I / Q values that drive every channel below 0
    and above 1 (asserted on the unclipped oracle for n >= 255), against np.clip of the
    oracle's RGB."""
    import image_analogies as ia
    rs = np.random.RandomState(n + 2)
    Bp = 3.0 * rs.rand(1, n) - 1.0
    yiq = np.dstack([rs.rand(1, n), 3.0 * rs.rand(1, n) - 1.5, 3.0 * rs.rand(1, n) - 1.5])
    rgb = o.convert_to_RGB(np.dstack([Bp, yiq[..., 1:]]))
    if n >= 255:
        for ch in range(3):
            assert (rgb[..., ch] < 0).any() and (rgb[..., ch] > 1).any() and \
                ((rgb[..., ch] > 0) & (rgb[..., ch] < 1)).any()
    got = ia.color_output(0, dev(Bp), None, None, [[dev(yiq)]], config(convert=True))
    assert np.array_equal(got, np.clip(rgb, 0, 1))


@pytest.mark.parametrize('C', [1, 3])
@pytest.mark.parametrize('n', EDGE_COUNTS)
def test_color_output_copy_branch_three_sources(gpu, n, C):
    """ia_color_output without convert through color_output and a three-pyramid
    color_pyr_list (the torch.stack branch, im > 0): every pixel copies its source's colour."""
    import torch
    import image_analogies as ia
    rs = np.random.RandomState(n + 3 + C)
    ah, aw = 7, 9
    src = rs.rand(3, ah, aw) if C == 1 else rs.rand(3, ah, aw, 3)
    s = np.stack([rs.randint(0, ah, n), rs.randint(0, aw, n)], axis=1).astype(np.int32)
    im = rs.randint(0, 3, n).astype(np.int32)
    if n >= 3:
        im[:3] = [0, 1, 2]
    picked = src[im, s[:, 0], s[:, 1]]
    ref = (np.repeat(picked[:, None], 3, axis=1) if C == 1 else picked).reshape(1, n, 3)
    pyrs = [[dev(src[i])] for i in range(3)]
    got = ia.color_output(0, dev(np.zeros((1, n))), torch.as_tensor(s).to('cuda'),
                          torch.as_tensor(im).to('cuda'), pyrs, config(convert=False))
    assert np.array_equal(got, ref)


# ---- 4. setup_dev over the option grid -----------------------------------------------------------

def assert_setup(got, ref, c):
    A_pyr, Ap_list, B_pyr, Bp_pyr, colour = got
    rA, rAp, rB, rBp, rcol, L = ref
    assert c.max_levels == L

    def same(a, b, what):
        assert len(a) == len(b), what
        for l, (x, y) in enumerate(zip(a, b)):
            x = x.cpu().numpy()
            assert x.dtype == np.float64 and x.shape == y.shape, (what, l)
            assert np.array_equal(x, y), (what, l)
    same(A_pyr, rA, 'A')
    same(B_pyr, rB, 'B')
    same(Bp_pyr, rBp, "B'")
    assert len(Ap_list) == len(rAp) and len(colour) == len(rcol)
    for i, (p, q) in enumerate(zip(Ap_list, rAp)):
        same(p, q, "A'%d" % i)
    for i, (p, q) in enumerate(zip(colour, rcol)):
        same(p, q, 'colour %d' % i)


@pytest.mark.parametrize('dtype,convert,remap,abw,init_rand,levels', SETUP_GRID)
def test_setup_dev_option_grid_vs_oracle(gpu, dtype, convert, remap, abw, init_rand, levels):
    """setup_dev from uint8 / float32 / float64 images (RGB with convert, luminance without)
    under remap_lum, AB_weight, init_rand and a level cap: every level of A, each A', B, B' and
    the colour pyramid(s) equals the oracle's, and c.max_levels is right."""
    import image_analogies as ia
    A, Aps, B = setup_images(dtype, convert)
    if dtype == 'uint8':
        assert image_scale(A) == image_scale(B) == image_scale(Aps[-1][0]) == 255.
    c = config(convert=convert, remap_lum=remap, AB_weight=abw, init_rand=init_rand, levels=levels, seed=7)
    got = ia.setup_dev(A, Aps, B, c)
    ref = reference_setup(A, Aps, B, convert, abw, remap, init_rand, levels, 7)
    assert ref[5] == (3 if levels else 4)
    assert_setup(got, ref, c)


def test_setup_dev_ap_scale_from_first_row_of_last_ap(gpu):
    """The reference's scale rule read literally: a uint8 A' (the last of two) whose FIRST ROW
    is <= 1 gets scale 1.0, and every A' then stays in 0 .. 255."""
    import image_analogies as ia
    A, Aps, B = setup_images('uint8', False, seed=43)
    Aps[-1][0] = Aps[-1][0] > 127
    assert image_scale(Aps[-1][0]) == 1.0 and image_scale(Aps[-1]) == 255. and image_scale(Aps[0][0]) == 255.
    c = config(seed=3)
    got = ia.setup_dev(A, Aps, B, c)
    ref = reference_setup(A, Aps, B, False, seed=3)
    assert ref[1][0][-1].max() > 200 and ref[0][-1].max() <= 1.0
    assert_setup(got, ref, c)


# ---- 5. synthesis under the options ------------------------------------------------------------

OPTION_KINDS = ('remap', 'ab_small', 'ab_large', 'init_b', 'all')


def run_case(case):
    import image_analogies as ia
    A, Ap, B, Bp = dev_job(case)
    out = ia.synthesize_dev(A, Ap, B, Bp, case.L, case.k, case.w, debug=True)
    assert_case(case, out, Bp)


@pytest.mark.parametrize('name', ['xwave', 'rescore', 'worklist'])
@pytest.mark.parametrize('kind', OPTION_KINDS)
def test_options_row_levels_vs_oracle(gpu, form, kind, name):
    """A 40 x 52, two A', B 24 x 31, every level, k = 1: B', s, im, sa and app_dist of every
    level equal the oracle's under each option, which changes the oracle's own result."""
    case = option_case(kind + '@small')
    assert_differs_from_plain(kind + '@small')
    if kind in ('remap', 'all'):
        assert case.pyr[1][0][-1].min() < 0 or case.pyr[1][0][-1].max() > 1
    form(name)
    run_case(case)


@pytest.mark.parametrize('name', ['default', 'split16'])
@pytest.mark.parametrize('kind', ['remap', 'ab_small', 'all'])
def test_options_strip_level_vs_oracle(gpu, form, kind, name):
    """A 256 x 512 (131,072 rows: k_xstrip over the rotated and the split-f16 screen), B
    12 x 30: the relative scale of the row's two halves reaches amax, the R16 rotation and
    its skipped-dimension term."""
    case = option_case(kind + '@strip')
    assert_differs_from_plain(kind + '@strip')
    form(name)
    run_case(case)


def test_options_batch_vs_oracle(gpu):
    """'all' and 'ab_large' as two jobs of one synthesize_batch_dev call."""
    import image_analogies as ia
    cases = [option_case('all@small'), option_case('ab_large@small')]
    jobs = [dev_job(c) for c in cases]
    outs = ia.synthesize_batch_dev(jobs, cases[0].L, [c.k for c in cases], cases[0].w, debug=True)
    for c, out, job in zip(cases, outs, jobs):
        assert_case(c, out, job[3])


_COLOUR = {}


def colour_option_case():
    """3-channel pyramids under AB_weight = 0.5 and init_rand=False (B' starts as the pyramid
    of the UNcompressed B) with the numpy oracle's scanline run and the plain run's s."""
    if not _COLOUR:
        from test_gpu_color3 import colour, pyr3
        from scipy.ndimage import gaussian_filter
        A, B = colour(61, (36, 44)), colour(62, (30, 34))
        Aps = [np.dstack([gaussian_filter(A[..., ch], 1.0 + 0.5 * i) for ch in range(3)]) for i in range(2)]
        w = o.compute_weights(3, 5, 12, 3)
        for key, abw, init_rand in (('opt', 0.5, False), ('plain', 1, True)):
            Ac, Bc = o.compress_values(A, B, abw)
            A_pyr, B_pyr = pyr3(Ac), pyr3(Bc)
            Ap_list = [pyr3(x) for x in Aps]
            L = min(len(A_pyr), len(B_pyr))
            Bp0 = o.initialize_Bp(B_pyr if init_rand else pyr3(B), init_rand, 5)
            As = o.create_index(A_pyr, Ap_list, L)
            Bp, ref = [b.copy() for b in Bp0], {}
            for level in range(1, L):
                dbg = {}
                s, im = o.synthesize_level(level, L, A_pyr, Ap_list, B_pyr, Bp, As[level], w, 1.0, debug=dbg)
                ref[level] = (s, im, dbg)
            _COLOUR[key] = (A_pyr, Ap_list, B_pyr, Bp0, L, w, ref, Bp)
    return _COLOUR['opt'], _COLOUR['plain']


@pytest.mark.parametrize('rot', ['1', '0'])
def test_options_colour_matching_vs_oracle(gpu, monkeypatch, rot):
    """The 165-dim matcher (rotated screen and split-f16 screen) with the A/B channels at half
    the scale of A'/B' and B' started from B: B', s, im and the debug record equal the
    oracle's scanline run."""
    import image_analogies as ia
    (A_pyr, Ap_list, B_pyr, Bp0, L, w, ref, Bp_ref), plain = colour_option_case()
    assert not np.array_equal(ref[L - 1][0], plain[6][L - 1][0])
    monkeypatch.setenv('IA_DB_ROT', rot)
    Bp_dev = [dev(b) for b in Bp0]
    out = ia.synthesize_dev([dev(p) for p in A_pyr], [[dev(p) for p in q] for q in Ap_list],
                            [dev(p) for p in B_pyr], Bp_dev, L, 1.0, w, debug=True)
    for level in range(1, L):
        s, im, dbg = out[level]
        rs, rim, rd = ref[level]
        assert np.array_equal(s.cpu().numpy(), rs), level
        assert np.array_equal(im.cpu().numpy(), rim), level
        assert np.array_equal(Bp_dev[level].cpu().numpy(), Bp_ref[level]), level
        rec = ia.debug_record(s, im, dbg, Bp_ref[level].shape[:2])
        for key in ('sa', 'sc', 'rstars'):
            assert rec[key] == rd[key], (level, key)
        assert np.array_equal(rec['app_dist'], rd['app_dist']), level
        assert np.array_equal(rec['coh_dist'], rd['coh_dist']), level


# ---- 6. image_analogies_main with the options -----------------------------------------------------

def _main_files(tmp_path, images, mode):
    from test_gpu_outputs import _write_png
    files = {}
    for name, img in images.items():
        files[name] = str(tmp_path / (name + '.png'))
        _write_png(files[name], img, mode)
    return files


def test_main_convert_with_every_option_vs_oracle(gpu, tmp_path):
    """convert, remap_lum, init_rand=False, AB_weight 0.5, a 2-level cap, two A' files,
    debug: every level's colour image, s, im and debug record equal the oracle's, whose s
    differs from the same run without the three options."""
    import matplotlib.pyplot as plt
    import image_analogies as ia
    from test_gpu_outputs import _check, _oracle_run
    A, Aps, B = analogy_inputs(74, (36, 47), (33, 40), n_ap=2)
    rgb = lambda x: np.dstack([x, 0.3 + 0.5 * x * x, 1 - x])  # noqa: E731
    files = _main_files(tmp_path, {'A': rgb(A), 'Ap0': rgb(Aps[0]), 'Ap1': rgb(Aps[1]), 'B': rgb(B)}, 'RGB')
    c = config(convert=True, remap_lum=True, init_rand=False, AB_weight=0.5, levels=2, k=1.0, seed=74)
    out = {}
    ia.image_analogies_main(files['A'], [files['Ap0'], files['Ap1']], files['B'], str(tmp_path / 'out') + '/',
                            c, debug=True, outputs=out)
    dec = {n: plt.imread(p)[..., :3].astype(np.float64) for n, p in files.items()}
    B_yiq = o.convert_to_YIQ(dec['B'] / image_scale(dec['B']))
    color_pyr = o.compute_gaussian_pyramid(B_yiq, 3, 2)

    def color(level, Bp_pyr, s, im, Ap_list):
        return np.clip(o.convert_to_RGB(np.dstack([Bp_pyr[level], color_pyr[level][:, :, 1:]])), 0, 1)
    sAp = image_scale(dec['Ap1'][0])
    lum = (o.convert_to_YIQ(dec['A'] / image_scale(dec['A']))[..., 0],
           [o.convert_to_YIQ(dec[n] / sAp)[..., 0] for n in ('Ap0', 'Ap1')], B_yiq[..., 0])
    ref, L = _oracle_run(*lum, 74, 1.0, color, dict(AB_weight=0.5, remap_lum=True, init_rand=False, cap=2))
    plain, _ = _oracle_run(*lum, 74, 1.0, color, dict(cap=2))
    assert L == 3 and c.max_levels == 3
    assert not np.array_equal(ref[L - 1]['s'], plain[L - 1]['s'])
    _check(out, ref, L)


def test_main_greyscale_two_sources_vs_oracle(gpu, tmp_path):
    """convert=False on greyscale files with two A' (AB_weight 0.5, B' started from B): every
    colour pixel is its source's value in the A' pyramid of ITS image; im takes both values."""
    import matplotlib.pyplot as plt
    import image_analogies as ia
    from test_gpu_outputs import _check, _oracle_run
    A, Aps, B = analogy_inputs(75, (30, 41), (34, 38), n_ap=2)
    files = _main_files(tmp_path, {'A': A, 'Ap0': Aps[0], 'Ap1': Aps[1], 'B': B}, 'L')
    c = config(convert=False, init_rand=False, AB_weight=0.5, k=1.0, seed=75)
    out = {}
    ia.image_analogies_main(files['A'], [files['Ap0'], files['Ap1']], files['B'], str(tmp_path / 'out') + '/',
                            c, debug=True, outputs=out)
    dec = {n: plt.imread(p).astype(np.float64) for n, p in files.items()}
    assert dec['A'].ndim == 2

    def color(level, Bp_pyr, s, im, Ap_list):
        H, W = Bp_pyr[level].shape
        v = np.array([Ap_list[i][level][r, cc] for (r, cc), i in zip(s, im)]).reshape(H, W)
        return np.repeat(v[..., None], 3, axis=2)
    sAp = image_scale(dec['Ap1'][0])
    lum = (dec['A'] / image_scale(dec['A']), [dec['Ap0'] / sAp, dec['Ap1'] / sAp], dec['B'] / image_scale(dec['B']))
    ref, L = _oracle_run(*lum, 75, 1.0, color, dict(AB_weight=0.5, init_rand=False))
    plain, _ = _oracle_run(*lum, 75, 1.0, color)
    assert not np.array_equal(ref[L - 1]['s'], plain[L - 1]['s'])
    assert set(ref[L - 1]['im'].tolist()) == {0, 1}
    _check(out, ref, L)
