"""The screens' error bounds where they are load-bearing: under
rotations other than the level's own principal basis (reversed, identity, random
orthonormal: the skipped components then hold most of the energy, and only the term
2^-9 1.01 A_skip |q'_skip| of eps_R, per segment K c_j in k_xstrip, keeps the bound true),
on white noise and on data whose scaled values sit near the f16 floor (one outlier pixel
sets amax), and under centres other than the image means.  The diagnostic screens are
checked against fp64 per (query, segment); whole syntheses (strip and row-form levels, a
batch, colour, shifted centres) against the C oracle, B', s, im and every approximate pick.

The rotations come from a monkeypatched algorithms._eigh (no product hook), and every test
asserts that the index holds the rotation it asked for.  The reference-only part (the
inputs, rotation_of, the numpy restatement of the rotated screen emulate_screen) is shared
with the CPU tests of tests/test_oracle.py, which show that these inputs would catch a
kernel that mishandled the skip term."""
import math

import numpy as np
import pytest

import ia_oracle as o
from conftest import analogy_inputs
from test_gpu_fallback import (LumCase, assert_case, dev, dev_job, form,  # noqa: F401 (form: a fixture)
                               run_profiled, segment_order)
from test_gpu_split16 import U32, _scales

pytestmark = pytest.mark.gpu

R16_P = 3                 # ia_rot16.h R16_P: components that keep their cross terms
R16_EPS_A2 = 90.0         # ia_rot16.h R16_EPS_A2 (the 16x16x32 form)
ROTATIONS = ('reversed', 'identity', 'random')
DATA = ('smooth', 'white', 'outlier')
RANDOM_SEED = 20


# ---- reference-only: rotations, inputs, the screens in numpy ----------------------------------

def rotation_of(kind, C, eigh=np.linalg.eigh):
    """(w, V) as algorithms._eigh returns them (the builders then reverse the columns):
    'principal' the eigh of C itself; 'reversed' the same with w and the columns reversed (after
    the builder's flip the components come by INCREASING variance, the split slots hold the
    least energy); 'identity' the canonical basis (after the flip); 'random' the Q of a seeded
    Gaussian matrix.  w[i] is always the variance of C along column i."""
    n = C.shape[0]
    w, V = eigh(C)
    if kind == 'principal':
        return w, V
    if kind == 'reversed':
        return w[::-1].copy(), V[:, ::-1].copy()
    if kind == 'identity':
        V = np.eye(n)[:, ::-1].copy()
    else:
        assert kind == 'random'
        V = np.linalg.qr(np.random.RandomState(RANDOM_SEED).standard_normal((n, n)))[0]
    return np.einsum('ij,ij->j', V, C @ V), V


def held_rotation(V):
    """The fp32 rotation an index holds for _eigh's V (columns by decreasing w)."""
    return np.ascontiguousarray(V[:, ::-1]).astype(np.float32)


def bound_images(kind, seed, shape):
    """(A, A'): 'smooth' analogy_inputs; 'white' uniform noise, A' independent of A; 'outlier'
    the smooth pair times 2^-12 with one interior pixel of each set to 1.0 (it sets amax, so
    nearly every scaled value of the split forms sits near the f16 floor)."""
    if kind == 'white':
        rs = np.random.RandomState(seed)
        return rs.rand(*shape), rs.rand(*shape)
    A, Aps, _ = analogy_inputs(seed, shape, (8, 8), n_ap=1)
    if kind == 'smooth':
        return A, Aps[0]
    assert kind == 'outlier'
    A, Ap = A * 2.0 ** -12, Aps[0] * 2.0 ** -12
    A[shape[0] // 2, shape[1] // 2] = Ap[shape[0] // 2, shape[1] // 2] = 1.0
    return A, Ap


def bound_queries(As, seed, scale, n=342):
    """n queries in a fixed shuffled order: exact rows (half of them drawn from the rows
    farthest from the rows' mean: the largest products, and on outlier data the only rows
    that see the outlier), near ties of both, 0.01-noise rows, far queries (uniform up to the
    rows' largest value) and the rows' mean (about the centre)."""
    rs = np.random.RandomState(seed)
    N = len(As)
    k = (n - 1) // 5
    far = np.argsort(((As - As.mean(0)) ** 2).sum(1))[-64:]
    pick = lambda c: np.r_[rs.randint(0, N, c - c // 2), far[rs.randint(0, len(far), c // 2)]]  # noqa: E731
    last = n - 1 - 4 * k
    Q = np.vstack([As[pick(k)],
                   As[pick(k)] + rs.randn(k, 55) * 1e-7 * scale,
                   As[pick(k)] + rs.randn(k, 55) * 0.01 * scale,
                   As[pick(k)] + rs.randn(k, 55) * 0.01 * As.max(),
                   rs.rand(last, 55) * As.max(),
                   np.full((1, 55), As.mean())])
    return Q[rs.permutation(n)]


def data_scale(kind):
    return 2.0 ** -12 if kind == 'outlier' else 1.0


class BoundLevel:
    """The finest level of an (A, A') pair under a 1-level cap, from the reference alone: the
    pyramids, the fp64 rows, the queries, the centre (image means) and the bound A."""

    def __init__(self, kind, seed, shape):
        A, Ap = bound_images(kind, seed, shape)
        self.kind = kind
        self.A_pyr = o.compute_gaussian_pyramid(A, 3, cap=1)
        self.Ap_pyr = o.compute_gaussian_pyramid(Ap, 3, cap=1)
        assert len(self.A_pyr) == 2
        self.As = o.create_index(self.A_pyr, [self.Ap_pyr], 2)[1]
        self.Q = bound_queries(self.As, seed + 1, data_scale(kind))
        self.center = np.r_[np.full(34, self.A_pyr[1].mean()), np.full(21, self.Ap_pyr[1].mean())]
        self.amax = amax_bound(self.A_pyr, [self.Ap_pyr], 1, self.center)

        self._queries = {}

    def cov(self):
        a = self.As - self.center
        return a.T @ a / len(a)

    def queries(self, kind):
        """The level's queries under rotation `kind`: 16 worst-case ones first, then self.Q."""
        if kind not in self._queries:
            V = held_rotation(rotation_of(kind, self.cov())[1])
            self._queries[kind] = np.vstack([worst_case_queries(self, V), self.Q[:len(self.Q) - 16]])
        return self._queries[kind]


def worst_case_queries(lv, V32, count=16, P=R16_P):
    """Queries aimed at the dropped cross terms, from the reference alone: for the `count` rows
    of largest |rho_skip|, kappa = rho + 2 |a'| d with d the unit vector along the f16 rounding
    errors alpha_l of the row's scaled skipped components (the row stays its segment's minimum,
    so the screen reports its value), then each scaled beta_k (k >= P) moved from its f16 value
    by 0.45 ulp towards the sign that gives alpha_h beta_l the sign of alpha_l beta_h.  The
    dropped products of that (row, query) pair along d then all have one sign: the errors add
    up instead of averaging out, which is what the Cauchy-Schwarz term of eps_R allows for."""
    V = V32.astype(np.float64)
    a = lv.As - lv.center
    rho = (a @ V).astype(np.float32).astype(np.float64)
    top = np.argsort((rho[:, P:] ** 2).sum(1))[-count:]
    alpha = np.ldexp(rho[top], _scales(lv.amax, 0.0)[0])
    ah = alpha.astype(np.float16).astype(np.float64)
    al = alpha - ah
    al[:, :P] = 0.0
    na = np.linalg.norm(a[top], axis=1)
    kap = rho[top] + al * (2.0 * na / np.maximum(np.linalg.norm(al, axis=1), 1e-300))[:, None]
    eq = np.array([_scales(lv.amax, float(x @ x))[2] for x in kap])
    bh = np.ldexp(-2.0 * kap, eq[:, None]).astype(np.float16)
    beta = bh.astype(np.float64) - np.sign(ah) * 0.45 * np.spacing(np.abs(bh)).astype(np.float64)
    beta[:, :P] = np.ldexp(-2.0 * kap[:, :P], eq[:, None])
    return lv.center + np.ldexp(beta, -eq[:, None]) / -2.0 @ V.T


_LEVELS = {}


def bound_level(kind, shape=(256, 512)):
    if (kind, shape) not in _LEVELS:
        _LEVELS[kind, shape] = BoundLevel(kind, 45, shape)
    return _LEVELS[kind, shape]


def amax_bound(A_pyr, Ap_list, level, center):
    """The split scale's A restated: fl32, rounded up, of sqrt(sum over the
    features of the larger squared deviation of their image's value range from the centre)."""
    imgs = (A_pyr[level - 1], A_pyr[level], np.stack([p[level - 1] for p in Ap_list]),
            np.stack([p[level] for p in Ap_list]))
    rng = [(x.min(), x.max()) for x in imgs]
    b2 = 0.0
    for k in range(55):
        lo, hi = rng[0 if k < 9 else (1 if k < 34 else (2 if k < 43 else 3))]
        b2 += max((lo - center[k]) ** 2, (hi - center[k]) ** 2)
    a = math.sqrt(b2 * (1.0 + 1e-12))
    f = np.float32(a)
    return float(f if f >= a else np.nextafter(f, np.float32(np.inf)))


def f16_split(x, flush=False):
    """ia_split16.h split16f / split16d in numpy: x -> fp32 -> (hi, lo) f16 values, as fp64;
    flush: f16 subnormals (below 2^-14) read as zero."""
    x = np.asarray(x, dtype=np.float64)
    h = x.astype(np.float32).astype(np.float16).astype(np.float64)
    l = (x - h).astype(np.float32).astype(np.float16).astype(np.float64)
    if flush:
        h = np.where(np.abs(h) < 2.0 ** -14, 0.0, h)
        l = np.where(np.abs(l) < 2.0 ** -14, 0.0, l)
    return h, l


def emulate_screen(rows, center, amax, Q, order, seg, V32=None, P=R16_P, flush=False, eps_a2=R16_EPS_A2):
    """The rotated screen (V32: the fp32 rotation, components >= P as f16 hi parts only,
    exact products, the scales of _scales; V32 None: the split-f16 screen, every component
    split) over `rows` in the library's segment order.  Returns a dict of (M, nseg) segment
    minima in unscaled units: 'm' the emulated ones, 'x' the fp64 ones; per query 'nq',
    'nsk', 'eps0' (the bound without the skip term; V32 None: eps16) and 'epsR'; 'askip'."""
    a = rows - center
    N = len(a)
    na = np.einsum('ij,ij->i', a, a)
    assert math.sqrt(na.max()) <= amax * (1 + 1e-6)
    if V32 is None:
        V, P = np.eye(55), 55
    else:
        V = V32.astype(np.float64)
    rho = (a @ V).astype(np.float32).astype(np.float64)
    askip = float(np.sqrt((rho[:, P:] ** 2).sum(1)).max())
    ea, R, _ = _scales(amax, 0.0)
    ah, al = f16_split(np.ldexp(rho, ea), flush)
    nh, nl = f16_split(np.ldexp(na.astype(np.float32).astype(np.float64), ea - R), flush)
    pos = np.minimum(np.asarray(order), N - 1)           # the padding repeats the last row
    nseg = len(pos) // seg
    q = Q - center
    nq = np.einsum('ij,ij->i', q, q)
    kap = q @ V
    nsk = (kap[:, P:] ** 2).sum(1)
    eq = np.array([_scales(amax, float(x))[2] for x in nq])
    bh, bl = f16_split(np.ldexp(-2.0 * kap, eq[:, None]), flush)
    n16 = np.ldexp(1.0, eq + R).astype(np.float16).astype(np.float64)
    m, x = np.empty((len(Q), nseg)), np.empty((len(Q), nseg))
    for m0 in range(0, len(Q), 64):
        s = slice(m0, m0 + 64)
        S = ah @ bh[s].T + al[:, :P] @ bh[s, :P].T + ah[:, :P] @ bl[s, :P].T + np.outer(nh + nl, n16[s])
        S = np.ldexp(S, -(ea + eq[s])[None, :])
        E = na[:, None] - 2.0 * (a @ q[s].T)
        m[s] = S[pos].reshape(nseg, seg, -1).min(axis=1).T
        x[s] = E[pos].reshape(nseg, seg, -1).min(axis=1).T
    if V32 is None:
        eps0 = U32 * (300 * amax * np.sqrt(nq) + 50 * amax * amax)
    else:
        eps0 = U32 * (360 * amax * np.sqrt(nq) + eps_a2 * amax * amax)
    return dict(m=m, x=x, nq=nq, nsk=nsk, eps0=eps0, epsR=eps0 + 2.0 ** -9 * 1.01 * askip * np.sqrt(nsk),
                askip=askip)


def strip_images():
    """The end-to-end strip input: A 256 x 512 (131,072 rows, 512 segments), B 16 x 48."""
    return analogy_inputs(93, (256, 512), (16, 48), 1)


_E2E = {}


def e2e_case(name):
    """The oracle runs of the end-to-end tests, once per module."""
    if name not in _E2E:
        if name == 'strip':
            _E2E[name] = LumCase(strip_images(), 1, 1.0, 93)
        else:
            assert name == 'small'
            _E2E[name] = LumCase(analogy_inputs(94, (40, 52), (24, 31), 1), None, 1.0, 94, tie=False)
    return _E2E[name]


def affected_queries(case, kind='reversed'):
    """Queries of the case's finest level for which an exact stage testing m_j <= e* + 2 eps_0
    drops the true winner's segment while eps_R keeps it, from the emulation alone."""
    A_pyr, Ap_list = case.pyr[0], case.pyr[1]
    l = case.L - 1
    c = np.r_[np.full(34, A_pyr[l].mean()), np.full(21, np.stack([p[l] for p in Ap_list]).mean())]
    amax = amax_bound(A_pyr, Ap_list, l, c)
    a = case.rows - c
    V = held_rotation(rotation_of(kind, a.T @ a / len(a))[1])
    order, seg = segment_order(len(case.rows), A_pyr[l].shape[0], A_pyr[l].shape[1])
    r = emulate_screen(case.rows, c, amax, case.Q[l], order, seg, V)
    inv = np.empty(len(case.rows), dtype=np.int64)
    keep = np.asarray(order) < len(case.rows)
    inv[np.asarray(order)[keep]] = np.flatnonzero(keep)
    mo = r['m'][np.arange(len(case.nn)), inv[case.nn] // seg]
    es = r['m'].min(axis=1)
    return int(((mo > es + 2 * r['eps0']) & (mo <= es + 2 * r['epsR'])).sum()), len(case.nn)


# ---- the rotation fixture --------------------------------------------------------------------------

@pytest.fixture
def rotation(monkeypatch):
    """select(kind): algorithms._eigh returns rotation_of(kind, C) from now on; the returned
    record lists every (kind, w, V) handed to a builder since.  Undone after the test."""
    import algorithms
    real = algorithms._eigh
    rec = {'kind': 'principal', 'calls': []}

    def fake(C):
        w, V = rotation_of(rec['kind'], C, real)
        rec['calls'].append((rec['kind'], w, V))
        return w, V

    monkeypatch.setattr(algorithms, '_eigh', fake)

    def select(kind):
        rec['kind'] = kind
        del rec['calls'][:]
        return rec
    return select


def rot_matrix(rot, n):
    """The n x n fp32 rotation of an index's device buffer (55: ld 56; 165: ld 168)."""
    R = rot.cpu().numpy()
    return R[:56 * 56].reshape(56, 56)[:55, :55] if n == 55 else R.reshape(165, 168)[:, :165]


def assert_rotation(rot, rec, kind, n, call=-1, rot_var=None):
    """The index holds the rotation asked for: the fp32 of the V that _eigh's stand-in returned
    for `kind`, which for 'identity' is the unit matrix and for the others differs from the
    principal basis (no silent fallback)."""
    got = rot_matrix(rot, n)
    k, w, V = rec['calls'][call]
    assert k == kind and V.shape == (n, n)
    assert np.array_equal(got, held_rotation(V)), kind
    if kind == 'identity':
        assert np.array_equal(got, np.eye(n, dtype=np.float32))
    if kind == 'reversed':
        assert (np.diff(w) <= 0).all() and w[0] > w[-1]      # _eigh's order reversed
    if rot_var is not None:
        assert np.array_equal(rot_var, w[::-1])


@pytest.fixture
def indices(monkeypatch):
    """Every index algorithms.level_index builds during the test (the synthesis drivers')."""
    import algorithms
    real = algorithms.level_index
    built = []

    def spy(*a, **k):
        idx = real(*a, **k)
        built.append(idx)
        return idx
    monkeypatch.setattr(algorithms, 'level_index', spy)
    return built


# ---- the screens at their diagnostic entry points ------------------------------------------------

def _index_of(lv, **kw):
    import algorithms
    return algorithms.level_index([dev(p) for p in lv.A_pyr], [[dev(p) for p in lv.Ap_pyr]], 1, **kw)


@pytest.mark.parametrize('wave', [0, 1])
@pytest.mark.parametrize('data', DATA)
@pytest.mark.parametrize('kind', ROTATIONS)
def test_r16_bound_under_rotation(gpu, rotation, kind, data, wave):
    """k_screen16r (block form) and k_screen16w (wave form) on a 256 x 512 level (131,072 rows,
    512 segments of 256: the strip level where k_xstrip runs) whose rotation is not its principal
    basis, on smooth, white and outlier data, M = 64 (one query group) and 342 (several): every
    segment minimum within eps_j of fp64, A_skip and A_skip,j bound the skipped components,
    and the codes c_j decode to at least A_skip,j."""
    import _ia
    from test_gpu_rot16 import _r16_vs_fp64
    lib = _ia.lib()
    assert lib.ia_db_rot_components() == R16_P and lib.ia_db_rot_eps_a2() == R16_EPS_A2
    lv = bound_level(data)
    rec = rotation(kind)
    idx = _index_of(lv, rot=True)
    assert idx.dbr is not None and len(lv.As) == 131072
    assert_rotation(idx.rot, rec, kind, 55, rot_var=idx.rot_var)
    amax, askip = (float(x) for x in idx.amax.cpu().numpy())
    assert amax == pytest.approx(lv.amax, rel=1e-6)
    prev = lib.ia_diag_set_r16_form(wave)
    try:
        worst = _r16_vs_fp64(idx, lv.As, lv.queries(kind), [64, 342], tight=False)
    finally:
        lib.ia_diag_set_r16_form(prev)
    print('r16 screen [%s, %s, %s form]: A_skip / A = %.3f, worst |segmin - exact| / eps_j = %.3g'
          % (data, kind, 'wave' if wave else 'block', askip / amax, worst))
    assert worst < 1.0


@pytest.mark.parametrize('data', ['white', 'outlier'])
def test_split16_bound_on_white_and_outlier_data(gpu, data):
    """The split-f16 screen (rows and image form, bit-equal) on a 128 x 256 level of white
    noise and of outlier data (most scaled values near the f16 floor: the flush / subnormal
    allowance of eps16): every segment minimum within eps16 of fp64."""
    from test_gpu_split16 import _screen_vs_fp64
    lv = bound_level(data, (128, 256))
    idx = _index_of(lv, rows=True)
    assert idx.db is not None and idx.dbi is not None
    assert float(idx.amax[0].item()) == pytest.approx(lv.amax, rel=1e-6)
    worst = _screen_vs_fp64(idx, lv.As, lv.Q, [len(lv.Q)])
    print('split16 screen [%s]: worst |segmin - exact| / eps16 = %.3g' % (data, worst))
    assert worst < 1.0


@pytest.mark.parametrize('kind', ['reversed', 'identity'])
def test_screen3r_bound_under_rotation(gpu, rotation, kind):
    """test_screen3r_error_bound's check (45 x 70, two A' images, scale 1) with the colour
    rotation reversed and the identity: every tile minimum within eps_Rc of fp64."""
    from test_gpu_color3 import _screen3r_vs_fp64
    rec = rotation(kind)
    worst, idx = _screen3r_vs_fp64(1.0)
    assert_rotation(idx.rot, rec, kind, 165)
    print('R16c screen [%s]: worst |tile min - exact| / eps = %.3g' % (kind, worst))
    assert 0.0 < worst <= 1.0


# ---- end to end against the C oracle ------------------------------------------------------------

_PRINCIPAL = {}


def _principal_record(name):
    """The principal-basis run of the strip case in one form (the baseline of the counts)."""
    if name not in _PRINCIPAL:
        _PRINCIPAL[name] = run_profiled(e2e_case('strip'))
    return _PRINCIPAL[name]


@pytest.mark.parametrize('name', ['default', 'xwave'])
@pytest.mark.parametrize('kind', ROTATIONS)
def test_strip_synthesis_under_rotation(gpu, form, rotation, indices, kind, name):
    """A 256 x 512 under a 1-level cap, B 16 x 48, through k_xstrip (per-segment skip bound:
    r16_kseg / r16_tseg0) and k_xwave (r16_thresholds_rows) with a rotation that is not the
    principal one: the oracle's B', s, im and approximate picks; no full scan (512 segments
    cannot reach the cap), and at least the principal basis's candidate segments (reversed:
    strictly more, the skip term widens every threshold)."""
    case = e2e_case('strip')
    form(name)
    base = _principal_record(name)
    assert base['full_scans'] == 0
    del indices[:]
    rec = rotation(kind)
    got = run_profiled(case)
    assert len(indices) == 1 and indices[0].dbr is not None
    assert_rotation(indices[0].rot, rec, kind, 55, rot_var=indices[0].rot_var)
    print('strip [%s, %s]: full_scans %d, candidate segments %d (principal basis %d) for %d queries'
          % (kind, name, got['full_scans'], got['candidate_segments'], base['candidate_segments'],
             case.queries[case.L - 1]))
    assert got['full_scans'] == 0
    assert got['candidate_segments'] >= base['candidate_segments']
    if kind == 'reversed':
        assert got['candidate_segments'] > base['candidate_segments']


def _run(case):
    import image_analogies as ia
    A, Ap, B, Bp = dev_job(case)
    out = ia.synthesize_dev(A, Ap, B, Bp, case.L, case.k, case.w, debug=True)
    assert_case(case, out, Bp)


@pytest.mark.parametrize('kind', ['reversed', 'random'])
def test_row_levels_synthesis_under_rotation(gpu, monkeypatch, rotation, indices, kind):
    """A 40 x 52, B 24 x 31, every level, with IA_ROT_MIN_ROWS = 0: the small row-form levels
    take the rotated screen in k_xwave; the oracle's results under a non-principal rotation."""
    monkeypatch.setenv('IA_ROT_MIN_ROWS', '0')
    case = e2e_case('small')
    rec = rotation(kind)
    _run(case)
    assert len(indices) == case.L - 1 == len(rec['calls'])
    for i, idx in enumerate(indices):
        assert idx.dbr is not None, i
        assert_rotation(idx.rot, rec, kind, 55, call=i, rot_var=idx.rot_var)


def test_batch_synthesis_under_reversed_rotation(gpu, rotation, indices):
    """Two jobs of the strip case as one batch (ia_synth_levels_batch) under the reversed
    rotation: both equal the oracle."""
    import image_analogies as ia
    case = e2e_case('strip')
    rec = rotation('reversed')
    jobs = [dev_job(case), dev_job(case)]
    outs = ia.synthesize_batch_dev(jobs, case.L, case.k, case.w, debug=True)
    assert len(indices) == 2
    for i, idx in enumerate(indices):
        assert idx.dbr is not None
        assert_rotation(idx.rot, rec, 'reversed', 55, call=i, rot_var=idx.rot_var)
    for job, out in zip(jobs, outs):
        assert_case(case, out, job[3])


_COLOUR = {}


def _colour_case():
    """Colour pyramids (A 36 x 44, B 30 x 34, one A') and the numpy oracle's run, once."""
    if not _COLOUR:
        from test_gpu_color3 import inputs
        A_pyr, Ap_list, B_pyr, Bp_pyr, L = inputs(84, (36, 44), (30, 34), n_ap=1)
        w = o.compute_weights(3, 5, 12, 3)
        As = o.create_index(A_pyr, Ap_list, L)
        Bp_ref = [b.copy() for b in Bp_pyr]
        ref = {}
        for level in range(1, L):
            dbg = {}
            s, im = o.synthesize_level(level, L, A_pyr, Ap_list, B_pyr, Bp_ref, As[level], w, 1.0, debug=dbg)
            ref[level] = (s, im, dbg)
        _COLOUR.update(pyr=(A_pyr, Ap_list, B_pyr, Bp_pyr, L), w=w, ref=ref, Bp_ref=Bp_ref)
    return _COLOUR


@pytest.mark.parametrize('shared', ['1', '0'])
@pytest.mark.parametrize('kind', ['reversed', 'identity'])
def test_colour_synthesis_under_rotation(gpu, monkeypatch, rotation, kind, shared):
    """The colour synthesis (R16c screen, k_exact3) against o.synthesize_level with the
    rotation reversed or the identity, one rotation for all levels (IA_ROT3_SHARED = 1) or
    one per level (0): B' in all channels, s, im and the debug lists."""
    import _ia
    import algorithms
    import image_analogies as ia
    c = _colour_case()
    A_pyr, Ap_list, B_pyr, Bp_pyr, L = c['pyr']
    monkeypatch.setenv('IA_ROT3_SHARED', shared)
    monkeypatch.setenv('IA_DB_ROT', '1')
    real, rots = algorithms.rot3_rotation, []

    def spy(db3, N):
        rots.append(real(db3, N))
        return rots[-1]
    monkeypatch.setattr(algorithms, 'rot3_rotation', spy)
    rec = rotation(kind)
    prev = _ia.lib().ia_diag_set_color16(1)
    try:
        Bp_dev = [dev(b) for b in Bp_pyr]
        out = ia.synthesize_dev([dev(p) for p in A_pyr], [[dev(p) for p in q] for q in Ap_list],
                                [dev(p) for p in B_pyr], Bp_dev, L, 1.0, c['w'], debug=True)
    finally:
        _ia.lib().ia_diag_set_color16(prev)
    assert len(rots) == len(rec['calls']) == (1 if shared == '1' else L - 1)
    for i, r in enumerate(rots):
        assert_rotation(r, rec, kind, 165, call=i)
    for level in range(1, L):
        s, im, dbg = out[level]
        rs, rim, rd = c['ref'][level]
        assert np.array_equal(s.cpu().numpy(), rs), level
        assert np.array_equal(im.cpu().numpy(), rim), level
        assert np.array_equal(Bp_dev[level].cpu().numpy(), c['Bp_ref'][level]), level
        got = ia.debug_record(s, im, dbg, c['Bp_ref'][level].shape[:2])
        for key in ('sa', 'sc', 'rstars'):
            assert got[key] == rd[key], (level, key)
        assert np.array_equal(got['app_dist'], rd['app_dist']), level
        assert np.array_equal(got['coh_dist'], rd['coh_dist']), level


# ---- another centre -----------------------------------------------------------------------------

CENTRES = ('zero', 'shifted')


@pytest.fixture
def centre(monkeypatch):
    """select(kind): _ia.mean_dev, from which LevelIndex takes its centre, returns 0 ('zero':
    uncentred) or the true mean + 0.5 ('shifted').  Undone after the test."""
    import _ia
    real = _ia.mean_dev

    def select(kind):
        assert kind in CENTRES
        monkeypatch.setattr(_ia, 'mean_dev', (lambda t: 0.0) if kind == 'zero' else (lambda t: real(t) + 0.5))
    return select


def assert_centre(idx, case, level, kind):
    A_pyr, Ap_list = case.pyr[0], case.pyr[1]
    mA, mAp = A_pyr[level].mean(), np.stack([p[level] for p in Ap_list]).mean()
    want = np.zeros(55) if kind == 'zero' else np.r_[np.full(34, mA + 0.5), np.full(21, mAp + 0.5)]
    got = idx.center.cpu().numpy()
    assert got.shape == (55,) and np.allclose(got, want, rtol=1e-12, atol=0), (level, kind)
    assert np.abs(got - np.r_[np.full(34, mA), np.full(21, mAp)]).min() > 0.1      # not the means


@pytest.mark.parametrize('name', ['default', 'xwave', 'split16'])
@pytest.mark.parametrize('kind', CENTRES)
def test_strip_synthesis_with_another_centre(gpu, form, centre, indices, kind, name):
    """The strip case with the centre 0 and the means + 0.5 ("any centre is exact for the
    distances"), through k_xstrip, k_xwave and the split-f16 screen: the oracle's results."""
    case = e2e_case('strip')
    form(name)
    centre(kind)
    _run(case)
    assert len(indices) == 1
    assert (indices[0].dbr is not None) == (name != 'split16')
    assert_centre(indices[0], case, case.L - 1, kind)


@pytest.mark.parametrize('name', ['rescore', 'worklist'])
@pytest.mark.parametrize('kind', CENTRES)
def test_row_levels_synthesis_with_another_centre(gpu, form, centre, indices, kind, name):
    """A 40 x 52, B 24 x 31, every level, through k_rescore and the work list with the centre
    0 and the means + 0.5."""
    case = e2e_case('small')
    form(name)
    centre(kind)
    _run(case)
    assert len(indices) == case.L - 1
    for level, idx in enumerate(indices, 1):
        assert_centre(idx, case, level, kind)


@pytest.mark.parametrize('kind', CENTRES)
def test_match_exact_with_another_centre(gpu, centre, kind):
    """ia_match_batch (both exact stages) with the centre 0 and the means + 0.5 equals the
    brute force (np.argmin, first minimum), row and distance."""
    import _ia
    import algorithms
    case = e2e_case('small')
    A_pyr, Ap_list = case.pyr[0], case.pyr[1]
    l = case.L - 1
    centre(kind)
    idx = algorithms.level_index([dev(p) for p in A_pyr], [[dev(p) for p in q] for q in Ap_list], l, rows=True)
    assert_centre(idx, case, l, kind)
    As = o.create_index(A_pyr, Ap_list, case.L)[l]
    rs = np.random.RandomState(4)
    Q = np.vstack([As[rs.randint(0, len(As), 24)], As[rs.randint(0, len(As), 24)] + rs.randn(24, 55) * 1e-7,
                   As[rs.randint(0, len(As), 24)] + rs.randn(24, 55) * 0.02, rs.rand(16, 55) * As.max(),
                   case.Q[l][rs.randint(0, len(case.Q[l]), 24)]])
    for mode in (0, 1):
        prev = _ia.rescore_mode(mode)
        try:
            gi, gd = idx.match(Q)
        finally:
            _ia.rescore_mode(prev)
        for m, (q, i, d) in enumerate(zip(Q, gi.cpu().numpy(), gd.cpu().numpy())):
            dd = np.add.reduce((As - q) ** 2, axis=1)
            j = int(np.argmin(dd))
            assert i == j and d == dd[j], (mode, m)
