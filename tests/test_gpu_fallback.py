"""The exact stage's fallback branches (`full = ns > RESCORE_SEGCAP ||
force_full`) against the scanline C oracle: label-map inputs whose flat regions tie over
more than 1024 segments (the full scan), over exactly 1024 (the last slist slot, no full
scan) and over the padded chunks of a linear image-form level; and constant or
near-constant A images (amax == 0, the ilogb clamp of split16_db_scale at both ends: an
analogy times 1e-25 and one times 2^62, a zero covariance for the R16 rotation, force_full on
every query).  Every form of the exact stage runs them;
B', s, im and the approximate pick of every pixel equal the oracle's bit for bit, and the
profile's full_scans proves the branch ran.

The inputs (label_inputs, colour_label_inputs, degenerate_inputs) and the reference-only
helpers (queries_from, tie_segments, app_reference) are shared with
test_gpu_color3_fallback.py and the CPU test of the checker in test_oracle.py."""
import types

import numpy as np
import pytest

import ia_oracle as o
import ia_oracle_c as oc
from conftest import analogy_inputs, smooth_noise

pytestmark = pytest.mark.gpu

SEGCAP = 1024        # RESCORE_SEGCAP (ia_exact.h): candidate segments held per query
C3_CAND = 64         # ia_color3.hip: candidate tiles (32 rows) held per colour query


# ---- inputs --------------------------------------------------------------------------------

def label_mask(shape, band, patch):
    """Textured pixels of a label map: the top `band` scanlines and one patch x patch square
    (vertically centred; on images of at least 256 columns 16 columns inside a 128-column
    strip, so every strip segment keeps flat rows beside it; else horizontally centred)."""
    H, W = shape
    m = np.zeros(shape, dtype=bool)
    m[:band] = True
    if patch:
        assert patch < 128
        r0 = (H - patch) // 2
        c0 = (W // 2) // 128 * 128 + 16 if W >= 256 else (W - patch) // 2
        m[r0:r0 + patch, c0:c0 + patch] = True
    return m


def label_inputs(seed, A_shape, B_shape, n_ap=1, band=0, patch=0, same_bg=False):
    """(A, [A'...], B) luminance label maps.  A is the constant 0.25 with texture 0.7 + 0.3
    smooth_noise on label_mask; A'_i the constant 0.6 - 0.1 i (0.6 for every i with same_bg)
    with the blurred texture on the same mask; B 0.25 in its left half, texture in its right.
    The flat rows of A / A' are bit-identical, and B's flat queries equal them exactly."""
    from scipy.ndimage import gaussian_filter
    mask = label_mask(A_shape, band, patch)
    tex = 0.7 + 0.3 * smooth_noise(seed, A_shape)
    A = np.where(mask, tex, 0.25)
    Aps = [np.where(mask, gaussian_filter(tex, 1.0 + 0.5 * i), 0.6 if same_bg else 0.6 - 0.1 * i)
           for i in range(n_ap)]
    B = np.full(B_shape, 0.25)
    half = B_shape[1] // 2
    B[:, half:] = (0.7 + 0.3 * smooth_noise(seed + 1, B_shape))[:, half:]
    return A, Aps, B


def colour_label_inputs(seed, A_shape, B_shape, n_ap=1, band=0, patch=0, cap=None):
    """The colour variant as oracle pyramids (A_pyr, Ap_list, B_pyr, Bp_pyr, L): every
    channel a label map of its own texture on one mask, the A' background equal to A's (0.25
    in every image), and B' initialised as a copy of B (initialize_Bp(..., False)): the flat
    queries then equal the flat rows exactly."""
    chans = [label_inputs(seed + 17 * ch, A_shape, B_shape, n_ap, band, patch) for ch in range(3)]
    mask = label_mask(A_shape, band, patch)
    A = np.dstack([c[0] for c in chans])
    Aps = [np.dstack([np.where(mask, c[1][i], 0.25) for c in chans]) for i in range(n_ap)]
    B = np.dstack([c[2] for c in chans])
    return colour_pyramids(A, Aps, B, cap)


def colour_pyramids(A, Aps, B, cap=None):
    A_pyr = o.compute_gaussian_pyramid(A, 3, cap)
    B_pyr = o.compute_gaussian_pyramid(B, 3, cap)
    Ap_list = [o.compute_gaussian_pyramid(x, 3, cap) for x in Aps]
    L = min(len(A_pyr), len(B_pyr))
    return A_pyr, Ap_list, B_pyr, o.initialize_Bp(B_pyr, False), L


DEGENERATE = ('near', 'const_exact', 'const_round', 'tiny', 'scaled', 'huge')


def degenerate_inputs(kind, seed, A_shape, B_shape):
    """(A, [A'], B) with a constant or near-constant A: 'near' 0.5 + 1e-10 smooth_noise (A' the
    same with another seed); 'const_exact' A = 0.25, A' = 0.75 (the means are exact: amax == 0);
    'const_round' A = 0.3, A' = 0.8 (the means round: amax ~ 1e-15); 'tiny' 1e-25 smooth_noise
    (ilogb(amax) < -60: the clamp of split16_db_scale).  B is smooth_noise in [0, 1].  'scaled':
    an ordinary analogy with EVERY image times 1e-25 (the clamp with queries as small as the
    rows, so nothing but the clamp itself can ask for the full scan).  'huge': huge_inputs (an
    analogy with every image times a power of two that puts amax at 2^61 or above: the upper
    clamp)."""
    if kind == 'huge':
        return huge_inputs(seed, A_shape, B_shape)[:3]
    if kind == 'scaled':
        A, Aps, B = analogy_inputs(seed, A_shape, B_shape, 1)
        return A * 1e-25, [Aps[0] * 1e-25], B * 1e-25
    if kind == 'near':
        A, Ap = 0.5 + 1e-10 * smooth_noise(seed, A_shape), 0.5 + 1e-10 * smooth_noise(seed + 7, A_shape)
    elif kind == 'const_exact':
        A, Ap = np.full(A_shape, 0.25), np.full(A_shape, 0.75)
    elif kind == 'const_round':
        A, Ap = np.full(A_shape, 0.3), np.full(A_shape, 0.8)
    else:
        assert kind == 'tiny'
        A, Ap = 1e-25 * smooth_noise(seed, A_shape), 1e-25 * smooth_noise(seed + 7, A_shape)
    return A, [Ap], smooth_noise(seed + 1, B_shape)


def huge_inputs(seed, A_shape, B_shape):
    """(A, [A'], B, s): an analogy under a 1-level pyramid cap with every image times the power
    of two s, the smallest with max |A - mean A| s >= 2^61 (a lower bound of amax, whose
    exponent split16_db_scale then clamps at 60).  assert_forced also wants image_range_bound s
    < 2^63.9 (|a'|^2 stays finite in fp32), and image_range_bound >= sqrt(34) max |A - mean A|:
    the admissible s span less than a binade.  So A is smooth noise of sigma 4 stretched
    about its median and clipped to [0, 1] (mean about 0.5: max |A - mean A| just above 0.5),
    A' a quarter of its blur (a small share of the bound), and only the finest level runs (a
    coarser level's narrower range would need a larger s)."""
    from scipy.ndimage import gaussian_filter
    x = smooth_noise(seed, A_shape, 4.0)
    A = np.clip(0.5 + 4.0 * (x - np.median(x)), 0.0, 1.0)
    Ap = 0.25 * gaussian_filter(A, 1.0)
    B = smooth_noise(seed + 1, B_shape)
    s = 2.0 ** np.ceil(61 - np.log2(np.abs(A - A.mean()).max()))
    return A * s, [Ap * s], B * s, s


# ---- reference-only helpers (numpy and the C oracle; no GPU) ----------------------------------

def queries_from(level, B_pyr, Bp_init, Bp_final):
    """Every pixel's query row of a level rebuilt from the oracle's B': the scan replayed over
    the level's initial B', each pixel set to its final value after its query is taken (the
    window's mirrored edge samples are pixels not yet synthesised, so the final B' alone
    would not do); the coarse level is final before the level starts."""
    H, W = B_pyr[level].shape[:2]
    cur = np.array(Bp_init[level], dtype=np.float64)
    half = np.empty((H * W, 21 * (cur.shape[2] if cur.ndim == 3 else 1)))
    for r in range(H):
        for c in range(W):
            half[r * W + c] = o.extract_pixel_feature(Bp_final[level - 1], cur, (r, c), False)
            cur[r, c] = Bp_final[level][r, c]
    assert np.array_equal(cur, Bp_final[level])
    return np.hstack([o.level_features(B_pyr[level - 1], B_pyr[level], True), half])


def tie_segments(rows, nn, order, seg, pool=None):
    """Per query: the number of segments (positions [j seg, (j + 1) seg) of `order`, the
    library's row order; positions past the last row repeat it, as the padding does) holding
    a row bit-identical to the query's nearest neighbour pool[nn].  pool: the rows nn indexes
    (default: `rows` itself); with a shard's rows and the whole level as pool the count is 0
    where the shard holds no copy of the level's nearest row."""
    N = len(rows)
    pos_row = np.minimum(np.asarray(order), N - 1)
    bits = np.ascontiguousarray(rows).view(np.uint64)
    pbits = bits if pool is None else np.ascontiguousarray(pool).view(np.uint64)
    mult = np.random.RandomState(1).randint(1, 2 ** 62, rows.shape[1]).astype(np.uint64) * np.uint64(2) + np.uint64(1)
    with np.errstate(over='ignore'):
        h = (bits * mult).sum(axis=1, dtype=np.uint64)     # a 64-bit hash per row
        count = {}
        for j in np.unique(nn):
            cand = np.flatnonzero(h == (pbits[j] * mult).sum(dtype=np.uint64))
            same = np.zeros(N, dtype=bool)
            same[cand[(bits[cand] == pbits[j]).all(axis=1)]] = True
            count[int(j)] = np.unique(np.flatnonzero(same[pos_row]) // seg).size
    return np.array([count[int(j)] for j in nn])


def has_coherence(s, im, H, W, A_h, A_w):
    """Per pixel: whether a coherence candidate exists (algorithms.py:92-130: a causal
    neighbour r in the 5 x 5 window whose s(r) + (q - r) lies inside A')."""
    s = np.asarray(s).reshape(H, W, 2)
    out = np.zeros(H * W, dtype=bool)
    for row in range(H):
        for col in range(W):
            for rr in range(max(0, row - 2), row + 1):
                for cc in range(max(0, col - 2), min(W, col + 3)):
                    if rr * W + cc < row * W + col:
                        pr, pc = s[rr, cc, 0] + row - rr, s[rr, cc, 1] + col - cc
                        if 0 <= pr < A_h and 0 <= pc < A_w:
                            out[row * W + col] = True
    return out


def app_reference(db, Q, s, im, shape, A_shape, w):
    """The reference's approximate pick of every pixel from the oracle alone: (sa, app_dist) of
    the debug record = the exact 1-NN of the reconstructed queries (pixel inside its A'
    image) and its weighted distance where a coherence candidate exists (else 0,
    image_analogies.py:141-159), plus the rows themselves."""
    H, W = shape
    A_h, A_w = A_shape
    nn, _ = db.nn(Q) if db.D == 55 else db.scan(Q)     # (165-dim rows: the scan, not the index)
    rem = nn % (A_h * A_w)
    sa = [(int(r), int(c)) for r, c in zip(rem // A_w, rem % A_w)]
    has = has_coherence(s, im, H, W, A_h, A_w)
    d = np.array([o.compute_distance(db.rows[j], q, w) if ok else 0.0 for j, q, ok in zip(nn, Q, has)])
    return nn, sa, d.reshape(H, W)


def segment_order(N, Ah, Aw, row0=0, nrows=None):
    """(order, seg): the matcher's segment order of an N-row level, or of its shard of rows
    [row0, row0 + nrows) as local rows (the chunk geometry is the shard's own:
    ia_db_chunk_rows / ia_db_rows_padded of nrows, ia_diag_stage_map of the range; host side
    only), and its segment length."""
    import _ia
    from test_gpu_split16 import _segment_order
    lib = _ia.lib()
    nrows = N - row0 if nrows is None else nrows
    npad = lib.ia_db_rows_padded(nrows)
    seg = min(lib.ia_db_chunk_rows(nrows), 512)
    idx = types.SimpleNamespace(row0=row0, src=types.SimpleNamespace(Aw=Aw, Ah=Ah))
    return _segment_order(idx, nrows, npad, seg), seg


def case_pyramids(images, cap, seed, bp_scale=None, setup=None):
    """(A_pyr, Ap_list, B_pyr, Bp_pyr, L) of a case's images: o.setup_luminance, and the random
    B' initialisation at the images' scale where the case has one."""
    A, Aps, B = images
    A_pyr, Ap_list, B_pyr, Bp_pyr, L = o.setup_luminance(A, Aps, B, cap=cap, seed=seed, **(setup or {}))
    if bp_scale is not None:
        Bp_pyr = [b * bp_scale for b in Bp_pyr]
    return A_pyr, Ap_list, B_pyr, Bp_pyr, L


class LumCase:
    """One luminance input with its oracle run (computed once per module, shared by the forms):
    per level the reference (B', s, im), the reconstructed queries' exact 1-NN, sa and
    app_dist; for the finest level the tie counts per query in the library's segment order.
    setup: further arguments of o.setup_luminance (AB_weight, remap_lum, init_rand)."""

    def __init__(self, images, cap, k, seed, tie=True, bp_scale=None, setup=None):
        self.k = k
        A_pyr, Ap_list, B_pyr, Bp_pyr, L = self.pyr = case_pyramids(images, cap, seed, bp_scale, setup)
        self.L = L
        self.w = o.compute_weights(3, 5, 12, 1)
        prev = oc.set_threads(0)
        try:
            Bp = [b.copy() for b in Bp_pyr]
            self.ref = oc.synthesize(A_pyr, Ap_list, B_pyr, Bp, L, k, self.w)
            self.app, self.Q = {}, {}
            for l in range(1, L):
                db = oc.LevelDB(l, A_pyr, Ap_list)
                self.Q[l] = queries_from(l, B_pyr, Bp_pyr, Bp)
                nn, sa, d = app_reference(db, self.Q[l], self.ref[l][1], self.ref[l][2], B_pyr[l].shape,
                                          A_pyr[l].shape, self.w)
                self.app[l] = (nn, sa, d)
                if tie and l == L - 1:
                    self.rows = db.rows.copy()
                    self.nn = nn
        finally:
            oc.set_threads(prev)
        self.queries = {l: B_pyr[l].shape[0] * B_pyr[l].shape[1] for l in range(1, L)}

    def ties(self, chunk_target=None):
        """Tied segments per finest-level query (under a chunk target: the batch path's)."""
        import _ia
        A_lg = self.pyr[0][self.L - 1]
        prev = _ia.lib().ia_set_chunk_target(chunk_target) if chunk_target else None
        try:
            order, seg = segment_order(len(self.rows), A_lg.shape[0], A_lg.shape[1])
        finally:
            if chunk_target:
                _ia.lib().ia_set_chunk_target(prev)
        return tie_segments(self.rows, self.nn, order, seg), len(order) // seg


_CASES = {}


def lum_spec(name):
    """LumCase's arguments for a named case (the rank processes of test_gpu_shards.py build the
    same pyramids from them with case_pyramids, without the oracle run)."""
    if name == 'over':      # 589,824 rows, 1152 segments: flat queries tie over > 1024
        return dict(images=label_inputs(90, (768, 768), (16, 48), 1, band=10, patch=96), cap=2, k=1.0, seed=90)
    if name == 'at':        # 524,288 rows, exactly 1024 segments, every one tied
        return dict(images=label_inputs(95, (512, 512), (16, 48), 2, band=0, patch=96, same_bg=True), cap=2,
                    k=1.0, seed=95)
    if name == 'padded':    # 156,672 rows = 306 chunks of 512 padded to 308: a linear level
        return dict(images=label_inputs(97, (204, 768), (16, 48), 1, band=0, patch=96), cap=2, k=1.0, seed=97)
    if name == 'plain':     # an ordinary job of the over-cap shapes (the batch's second job)
        return dict(images=analogy_inputs(91, (768, 768), (16, 48), 1), cap=2, k=1.0, seed=91, tie=False)
    kind, size = name.split('@')
    shapes = {'small': ((40, 52), (24, 31), None), 'strip': ((256, 512), (12, 30), 1)}[size]
    if kind == 'huge':      # (the finest level only: huge_inputs)
        A, Aps, B, sc = huge_inputs(93, shapes[0], shapes[1])
        return dict(images=(A, Aps, B), cap=1, k=1.0, seed=93, tie=False, bp_scale=sc)
    return dict(images=degenerate_inputs(kind, 93, shapes[0], shapes[1]), cap=shapes[2], k=1.0, seed=93,
                tie=False, bp_scale=1e-25 if kind == 'scaled' else None)


def lum_case(name):
    if name not in _CASES:
        _CASES[name] = LumCase(**lum_spec(name))
    return _CASES[name]


# ---- running a case on the GPU ------------------------------------------------------------------

def dev(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).to('cuda', dtype=torch.float64)


def dev_job(case):
    A_pyr, Ap_list, B_pyr, Bp_pyr, L = case.pyr
    return ([dev(p) for p in A_pyr], [[dev(p) for p in q] for q in Ap_list], [dev(p) for p in B_pyr],
            [dev(b) for b in Bp_pyr])


def assert_case(case, out, Bp_dev):
    """B', s, im of every level and the approximate pick of every pixel against the oracle.
    out and Bp_dev (indexed by level) hold device tensors, or host arrays read back from a
    rank process's file (test_gpu_shards.py)."""
    import torch
    import image_analogies as ia
    t = lambda x: x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))  # noqa: E731
    out = {l: (t(v[0]), t(v[1]), tuple(t(x) for x in v[2])) for l, v in out.items()}
    assert set(out) == set(case.ref)
    for l in sorted(case.ref):
        Bp, s, im = case.ref[l]
        assert np.array_equal(out[l][0].cpu().numpy(), s), l
        assert np.array_equal(out[l][1].cpu().numpy(), im), l
        assert np.array_equal(t(Bp_dev[l]).cpu().numpy(), Bp), l
        rec = ia.debug_record(out[l][0], out[l][1], out[l][2], Bp.shape[:2])
        nn, sa, d = case.app[l]
        assert rec['sa'] == sa, l
        assert np.array_equal(rec['app_dist'], d), l


def finest(recs, case, jobs=1):
    rec = [r for r in recs if r['level'] == case.L - 1]
    assert len(rec) == 1 and rec[0]['jobs'] == jobs
    return rec[0]


def run_profiled(case):
    """One debug synthesis under an open profile -> the finest level's profile record."""
    import _ia
    import image_analogies as ia
    A, Ap, B, Bp = dev_job(case)
    _ia.prof_begin()
    try:
        out = ia.synthesize_dev(A, Ap, B, Bp, case.L, case.k, case.w, prof=True, debug=True)
    finally:
        recs = _ia.prof_end()
    assert_case(case, out, Bp)
    return finest(recs, case)


@pytest.fixture
def form(monkeypatch):
    """Select a form of the exact stage for one test; everything is restored after it."""
    import _ia
    prev = (_ia.xwave(), _ia.rescore_mode())

    def select(name):
        if name == 'split16':           # k_xstrip (k_xwave on linear levels), split-f16 screen
            monkeypatch.setenv('IA_DB_ROT', '0')
        elif name == 'xwave':           # k_xwave image form, r16_thresholds_rows
            _ia.xwave(1)
        elif name == 'rescore':         # k_rescore
            _ia.xwave(0)
            _ia.rescore_mode(0)
        elif name == 'worklist':        # k_select, k_items, k_gather
            _ia.xwave(0)
            _ia.rescore_mode(1)
        elif name == 'rows':            # the 224-B row form
            monkeypatch.setenv('IA_DB_IMAGE', '0')
        else:
            assert name == 'default'    # k_xstrip, R16
    yield select
    _ia.xwave(prev[0])
    _ia.rescore_mode(prev[1])


# ---- over the cap -------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['default', 'split16', 'xwave', 'rescore', 'worklist', 'rows'])
def test_over_cap_full_scan_vs_oracle(gpu, form, name):
    """A 768 x 768 label map (589,824 rows, 1152 segments of 512 rows; the lowest tied row is
    not in segment 0): every flat query ties over more than 1024 segments, so the exact stage
    walks every segment of the level (`full ? si + 1 : slist[si + 1]`).  Each form equals the
    oracle and reports at least the reference count of full scans."""
    case = lum_case('over')
    ties, nseg = case.ties()
    want = int((ties > SEGCAP).sum())
    assert nseg == 1152 and want >= 100, (nseg, want)
    form(name)
    rec = run_profiled(case)
    print('over cap [%s]: reference %d queries over %d segments (most %d), full_scans %d, candidate '
          'segments %d' % (name, want, SEGCAP, ties.max(), rec['full_scans'], rec['candidate_segments']))
    assert rec['full_scans'] >= want
    assert rec['candidate_segments'] >= nseg * want


def test_over_cap_batch_vs_oracle(gpu):
    """The over-cap job and an ordinary job of the same shapes as ONE batch
    (ia_synth_levels_batch): both equal their oracle runs, and the batch's finest level
    reports the label job's full scans."""
    import _ia
    import image_analogies as ia
    case, plain = lum_case('over'), lum_case('plain')
    ties, nseg = case.ties(chunk_target=max(64, 512 // 2))
    want = int((ties > SEGCAP).sum())
    assert want >= 100, want
    jobs = [dev_job(case), dev_job(plain)]
    _ia.prof_begin()
    try:
        outs = ia.synthesize_batch_dev(jobs, case.L, [case.k, plain.k], case.w, prof=True, debug=True)
    finally:
        recs = _ia.prof_end()
    assert_case(case, outs[0], jobs[0][3])
    assert_case(plain, outs[1], jobs[1][3])
    rec = finest(recs, case, jobs=2)
    print('over cap [batch]: reference %d, full_scans %d' % (want, rec['full_scans']))
    assert rec['full_scans'] >= want


# ---- at the cap ---------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['default', 'split16', 'rescore'])
def test_at_cap_no_full_scan_vs_oracle(gpu, form, name):
    """A 512 x 512, two A' images of one background (524,288 rows, exactly 1024 segments, the
    winner row 0 of image 0): every flat query ties over all 1024 segments.  That fills slist
    to its last slot and must NOT scan (`ns > CAP`, not `>=`)."""
    case = lum_case('at')
    ties, nseg = case.ties()
    want = int((ties == SEGCAP).sum())
    assert nseg == SEGCAP and want >= 100 and ties.max() == SEGCAP, (nseg, want)
    form(name)
    rec = run_profiled(case)
    print('at cap [%s]: reference %d queries over exactly %d segments, full_scans %d, candidate segments %d'
          % (name, want, SEGCAP, rec['full_scans'], rec['candidate_segments']))
    assert rec['full_scans'] == 0
    assert rec['candidate_segments'] >= SEGCAP * want


# ---- below the cap, padded chunks ------------------------------------------------------------

@pytest.mark.parametrize('name', ['default', 'rescore'])
def test_padded_linear_level_vs_oracle(gpu, form, name):
    """A 204 x 768 (156,672 rows = 306 chunks of 512 padded to 308: a linear image-form level,
    not a strip level) whose last row is flat: the two padded segments repeat a tied row, so
    flat queries rescore windows of padded chunks too.  No full scan (308 <= 1024)."""
    case = lum_case('padded')
    ties, nseg = case.ties()
    N = len(case.rows)
    assert N == 156672 and nseg * 512 > N
    # queries whose nearest neighbour is bit-identical to the last row, which the padding repeats
    want = int((case.rows[case.nn] == case.rows[N - 1]).all(axis=1).sum())
    assert want >= 100 and ties.max() <= SEGCAP, want
    form(name)
    rec = run_profiled(case)
    print('padded [%s]: reference %d queries tied over %d of %d segments, full_scans %d, candidate '
          'segments %d' % (name, want, ties.max(), nseg, rec['full_scans'], rec['candidate_segments']))
    assert rec['full_scans'] == 0
    assert rec['candidate_segments'] >= int(ties.sum())


# ---- force_full: constant and near-constant A ----------------------------------------------------

def image_range_bound(A_pyr, Ap_list, level):
    """U >= amax from the image ranges and means alone: a centred row's 34 A values lie within
    max |A - mean A| over both pyramid levels it reads, its 21 A' values likewise."""
    def spread(sm, lg):
        m = lg.mean()
        return max(np.abs(sm - m).max(), np.abs(lg - m).max()) * (1 + 1e-9) + 1e-300
    uA = spread(A_pyr[level - 1], A_pyr[level])
    uAp = max(spread(np.stack([p[level - 1] for p in Ap_list]), np.stack([p[level] for p in Ap_list])), 0)
    return float(np.sqrt(34 * uA * uA + 21 * uAp * uAp))


FORCED = ('near', 'tiny', 'scaled', 'huge')


def assert_forced(case, kind, rec, level):
    """force_full's reference-only precondition (U 2^25 < min |q - c|; 'scaled': amax <= U <
    2^-60, the clamp of split16_db_scale; 'huge': 2^61 <= max |A - mean A| <= amax <= U <
    2^63.9, the upper clamp with |a'|^2 finite in fp32), then full_scans == the level's pixel
    count."""
    A_pyr, Ap_list = case.pyr[0], case.pyr[1]
    U = image_range_bound(A_pyr, Ap_list, level)
    if kind == 'huge':
        lo = float(np.abs(A_pyr[level] - A_pyr[level].mean()).max())
        print('force_full [huge] level %d: max |A - mean A| 2^%.2f, U 2^%.2f, full_scans %d of %d' % (
            level, np.log2(lo), np.log2(U), rec['full_scans'], case.queries[level]))
        assert lo >= 2.0 ** 61 and U < 2.0 ** 63.9
        assert rec['full_scans'] == case.queries[level]
        return
    if kind == 'scaled':
        print('force_full [scaled] level %d: U 2^%.1f, full_scans %d of %d' % (
            level, np.log2(U), rec['full_scans'], case.queries[level]))
        assert U < 2.0 ** -61
        assert rec['full_scans'] == case.queries[level]
        return
    c = np.r_[np.full(34, A_pyr[level].mean()), np.full(21, np.stack([p[level] for p in Ap_list]).mean())]
    dmin = float(np.sqrt(((case.Q[level] - c) ** 2).sum(1)).min())
    print('force_full [%s] level %d: U %.3g, min |q - c| %.3g, ratio 2^%.1f, full_scans %d of %d' % (
        kind, level, U, dmin, np.log2(dmin / U), rec['full_scans'], case.queries[level]))
    assert U * 2.0 ** 25 < dmin
    assert rec['full_scans'] == case.queries[level]


@pytest.mark.parametrize('name', ['default', 'split16'])
@pytest.mark.parametrize('kind', DEGENERATE)
def test_degenerate_A_strip_level_vs_oracle(gpu, form, kind, name):
    """A 256 x 512 (131,072 rows: a strip level where the rotated DB applies), constant or
    near-constant: every form equals the oracle; the near-constant and 1e-25 inputs force a
    full scan of every query, and so does an ordinary analogy scaled by 1e-25 (amax < 2^-60:
    the clamped scale voids the screens' error bounds) or by 2^62 ('huge': amax >= 2^61, the
    upper clamp; the scaled norm slots pass the f16 range and are clipped by the builders)."""
    case = lum_case(kind + '@strip')
    form(name)
    rec = run_profiled(case)
    if kind in FORCED:
        assert_forced(case, kind, rec, case.L - 1)


@pytest.mark.parametrize('name', ['xwave', 'rescore', 'worklist'])
@pytest.mark.parametrize('kind', DEGENERATE)
def test_degenerate_A_row_levels_vs_oracle(gpu, form, kind, name):
    """A 40 x 52, B 24 x 31, every level (row-form levels with padding; 'huge': the finest
    level only, huge_inputs).  The forms here cut rows by the fp32 re-screen (e <= Trow): under
    the upper clamp a norm slot stored as inf / -inf read back as NaN and dropped its row, the
    nearest one included, until the builders clipped it."""
    import _ia
    import image_analogies as ia
    case = lum_case(kind + '@small')
    form(name)
    A, Ap, B, Bp = dev_job(case)
    _ia.prof_begin()
    try:
        out = ia.synthesize_dev(A, Ap, B, Bp, case.L, case.k, case.w, prof=True, debug=True)
    finally:
        recs = _ia.prof_end()
    assert_case(case, out, Bp)
    if kind in FORCED:
        for rec in recs:
            assert_forced(case, kind, rec, rec['level'])


@pytest.mark.parametrize('kind', DEGENERATE)
def test_degenerate_A_match_and_rot_build(gpu, kind):
    """ia_match_batch on the degenerate levels equals the brute force (np.argmin, first
    minimum); LevelIndex(..., rot=True) builds without IA_E_ARG, amax is finite, and every
    segment minimum of the diagnostic R16 screen is finite or its query full-scans."""
    import algorithms
    from test_gpu_rot16 import _segmin_r16
    from test_gpu_split16 import _scales
    small, strip = lum_case(kind + '@small'), lum_case(kind + '@strip')
    A_pyr, Ap_list = small.pyr[0], small.pyr[1]
    l = small.L - 1
    idx = algorithms.level_index([dev(p) for p in A_pyr], [[dev(p) for p in q] for q in Ap_list], l, rows=True)
    db = oc.LevelDB(l, A_pyr, Ap_list)     # (rows is a view: valid while db lives)
    As = db.rows
    rs = np.random.RandomState(6)
    Q = np.vstack([small.Q[l][rs.randint(0, len(small.Q[l]), 48)], As[rs.randint(0, len(As), 8)],
                   rs.rand(8, 55)])
    import _ia
    for mode in (0, 1):     # one workgroup per query, the work list
        prev = _ia.rescore_mode(mode)
        try:
            gi, gd = idx.match(Q)
        finally:
            _ia.rescore_mode(prev)
        for m, (q, i, d) in enumerate(zip(Q, gi.cpu().numpy(), gd.cpu().numpy())):
            dd = np.add.reduce((As - q) ** 2, axis=1)
            j = int(np.argmin(dd))
            assert i == j and d == dd[j], (mode, m)
    # the rotated DB on the 131,072-row level
    A_pyr, Ap_list = strip.pyr[0], strip.pyr[1]
    l = strip.L - 1
    idx = algorithms.level_index([dev(p) for p in A_pyr], [[dev(p) for p in q] for q in Ap_list], l, rot=True)
    assert idx.dbr is not None and idx.rot is not None
    amax = idx.amax.cpu().numpy()
    assert np.isfinite(amax).all() and (amax >= 0).all(), amax
    M = 64
    Q = strip.Q[l][rs.randint(0, len(strip.Q[l]), M)]
    segmin = _segmin_r16(idx, Q, M, idx.N)
    c = idx.center.cpu().numpy()
    for m in range(M):
        ea, R, eq = _scales(float(amax[0]), float(((Q[m] - c) ** 2).sum()))
        # (from 2^61 up the clamped scale lets scaled values overflow f16: split16_db_clamped
        # full-scans every query, whatever its norm)
        assert np.isfinite(segmin[m]).all() or eq + R < -10 or amax[0] >= 2.0 ** 61, (m, eq, R)


def test_builders_refuse_norms_that_overflow_fp32(gpu):
    """A 128 x 256 level times 2^70 (amax ~ 2^71.5: |a'|^2 overflows fp32, every norm slot would
    hold inf and the fp32 re-screen NaN): ia_db_build, ia_db_build_image and ia_db_build_rot
    each return IA_E_ARG with a message naming the limit; the unscaled level builds."""
    import ctypes
    import torch
    import _ia
    import algorithms
    lib = _ia.lib()
    A, Aps, _ = analogy_inputs(99, (128, 256), (8, 8), 1)
    pyr = lambda x, sc: [dev(p * sc) for p in o.compute_gaussian_pyramid(x, 3, cap=1)]  # noqa: E731
    ok = algorithms.level_index(pyr(A, 1.0), [pyr(Aps[0], 1.0)], 1, rows=True, rot=True)
    assert ok.db is not None and ok.dbi is not None and ok.dbr is not None
    A70, Ap70 = pyr(A, 2.0 ** 70), pyr(Aps[0], 2.0 ** 70)
    keep = (A70[0].contiguous(), A70[1].contiguous(), torch.stack([Ap70[0]]), torch.stack([Ap70[1]]))
    big = _ia.src_level(*keep)
    st, c = _ia.stream(), _ia.ptr(ok.center)
    calls = {
        'ia_db_build': lambda am: lib.ia_db_build(ctypes.byref(big), 0, ok.nrows, c, _ia.ptr(ok.db), am, st),
        'ia_db_build_image': lambda am: lib.ia_db_build_image(ctypes.byref(big), 0, ok.nrows, c, None, am,
                                                              _ia.ptr(ok.dbi), st),
        'ia_db_build_rot': lambda am: lib.ia_db_build_rot(ctypes.byref(big), 0, ok.nrows, c, _ia.ptr(ok.rot), am,
                                                          _ia.ptr(ok.dbr), st),
    }
    for who, call in calls.items():
        amax = torch.zeros(2, dtype=torch.float32, device='cuda')
        rc = call(_ia.ptr(amax))
        msg = lib.ia_last_error()
        torch.cuda.synchronize()
        assert rc == _ia.IA_E_ARG, who
        assert who.encode() in msg and b'2^64' in msg, msg
        assert float(amax[0].item()) >= 2.0 ** 64
