"""The split tail (DESIGN.md §6b "split"; k_xstrip<false, true, CMP, true>): a pixel's candidate
segments over two workgroups.  The shares are fixed by the segments' ranks, the helper's record is
merged by the commutative (distance, row) minimum, so every result equals the oracle's and the
unsplit kernel's bit for bit: whole syntheses with the plain and the compact tail, label maps whose
flat queries tie over a handful of segments and over exactly 1024 (both workgroups hold tied rows:
the lowest row wins whichever found it), and the full-scan cases, which stay with the owner alone.
The host rule: two workgroups per pixel only where the switch applies."""
import ctypes

import numpy as np
import pytest

import ia_oracle as o
import ia_oracle_c as oc
from conftest import analogy_inputs, smooth_noise

SEGCAP = 1024        # RESCORE_SEGCAP (ia_exact.h)


@pytest.fixture
def xsplit():
    """Set the split tail's row threshold for one test (0: off); restored after it."""
    import _ia
    lib = _ia.lib()
    prev = lib.ia_diag_set_xsplit_min_rows(-1)
    yield lambda rows: lib.ia_diag_set_xsplit_min_rows(rows)
    lib.ia_diag_set_xsplit_min_rows(prev)


def counts():
    """(pixels whose helper rescored a segment, pixels won by the helper's record) so far."""
    import _ia
    out = (ctypes.c_ulonglong * 2)()
    _ia.check(_ia.lib().ia_diag_xsplit_counts(out), 'ia_diag_xsplit_counts')
    return np.array([out[0], out[1]], dtype=np.int64)


# ---- host ----------------------------------------------------------------------------------------

def test_grid_is_doubled_only_where_the_switch_applies(xsplit):
    """ia_diag_xsplit_grid (the rule level_plan decides a level's split by): 2 R workgroups on an eligible level of
    at least the threshold's rows, R below it, with the switch off and on any other level;
    ia_diag_set_xsplit_min_rows reports the threshold in force (0: off); the wave geometry and
    the pipeline's schedule do not depend on the switch."""
    import _ia
    lib = _ia.lib()
    grid = lib.ia_diag_xsplit_grid

    def geometry():
        out = (ctypes.c_int * 5)()
        rows = []
        for t in range(0, 41 + 3 * 36, 7):
            _ia.check(lib.ia_diag_wave_rows(37, 41, t, 19, 21, out), 'ia_diag_wave_rows')
            rows.append(tuple(out))
        shapes = (ctypes.c_int * 6)(10, 11, 19, 21, 37, 41)
        ones, zeros = (ctypes.c_int * 3)(1, 1, 1), (ctypes.c_int * 3)(0, 0, 0)
        log = (ctypes.c_int * (4 * 4096))()
        n = lib.ia_diag_pipe_schedule(shapes, ones, zeros, 3, 0, 16, log, 4096)
        assert 0 < n <= 4096
        return rows, tuple(log[:4 * n])

    xsplit(1 << 12)
    assert lib.ia_diag_set_xsplit_min_rows(-1) == 1 << 12
    on = geometry()
    for R in (1, 7, 342):
        assert grid(1, 1 << 12, R) == 2 * R
        assert grid(1, (1 << 12) - 1, R) == R
        assert grid(0, 1 << 22, R) == R
    xsplit(0)
    assert lib.ia_diag_set_xsplit_min_rows(-1) == 0
    assert grid(1, 1 << 22, 342) == 342 and grid(0, 1 << 22, 342) == 342
    assert geometry() == on


# ---- parity --------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('shape_A,shape_B', [((128, 128), (37, 41)), ((32, 256), (24, 50))])
def test_split_synthesis_equals_oracle_and_split_off(gpu, xsplit, monkeypatch, shape_A, shape_B):
    """The two small syntheses of test_gpu_compact.py with the split on (threshold 1) and off, each
    with the compact tail on (threshold 1) and off: B', s and im of every level equal the oracle's
    (so each other's); with the compact tail on the library counts at least the finest level's
    clean waves as compact, so both tail forms ran split; with the split off no counter moves."""
    import _ia
    from test_gpu_compact import _synth
    lib = _ia.lib()
    monkeypatch.setenv('IA_ROT_MIN_ROWS', '1')
    A, Aps, B = analogy_inputs(57, shape_A, shape_B, n_ap=1)
    pyr = o.setup_luminance(A, Aps, B, cap=2, seed=57)
    A_pyr, Ap_list, B_pyr, Bp_pyr, L = pyr
    ref = oc.synthesize(A_pyr, Ap_list, B_pyr, [b.copy() for b in Bp_pyr], L, 0.5, o.compute_weights(3, 5, 12, 1))
    H, W = shape_B
    clean = sum(1 for t in range(W, W + 3 * (H - 1)) if t % 3)
    prev = lib.ia_diag_set_compact_min_rows(-1)
    set_compact = lambda rows: lib.ia_diag_set_compact_min_rows(rows)  # noqa: E731
    try:
        for split in (1, 0):
            for cmp_rows in (1, 0):
                xsplit(split)
                n0, c0 = lib.ia_diag_compact_waves(), counts()
                got = _synth(pyr, cmp_rows, set_compact)
                dn, dc = lib.ia_diag_compact_waves() - n0, counts() - c0
                print('split %d compact %d: compact waves %d, helper pixels %d, helper wins %d'
                      % (split, cmp_rows, dn, dc[0], dc[1]))
                assert (dn >= clean > 0) if cmp_rows else dn == 0
                assert split or not dc.any()
                assert set(got) == set(ref)
                for l in sorted(ref):
                    assert np.array_equal(got[l][1], ref[l][1]) and np.array_equal(got[l][2], ref[l][2]), l
                    assert np.array_equal(got[l][0], ref[l][0]), l
    finally:
        lib.ia_diag_set_compact_min_rows(prev)


# ---- the reported plan is what runs ---------------------------------------------------------------

@pytest.mark.gpu
def test_level_plan_reports_what_runs_and_is_sampled_per_level(gpu, xsplit, monkeypatch):
    """The finest (strip-order, R16) level of the small synthesis above with both thresholds at 1:
    ia_diag_level_plan says compact waves and split candidates, and running the level advances
    both forms' counters.  ia_diag_set_xwave(1) after the arguments are built changes the NEXT
    call of the same arguments to k_xwave on the image form (the knobs are sampled when a level
    starts): the plan says so and neither counter moves."""
    import algorithms
    import image_analogies as ia
    import _ia
    from test_gpu_split16 import dev
    lib = _ia.lib()
    monkeypatch.setenv('IA_ROT_MIN_ROWS', '1')
    A, Aps, B = analogy_inputs(57, (128, 128), (37, 41), n_ap=1)
    A_pyr, Ap_list, B_pyr, Bp_pyr, L = o.setup_luminance(A, Aps, B, cap=2, seed=57)
    prev_compact, prev_xwave = lib.ia_diag_set_compact_min_rows(-1), lib.ia_diag_set_xwave(-1)
    try:
        lib.ia_diag_set_compact_min_rows(1)
        xsplit(1)
        lib.ia_diag_set_xwave(2)
        index = algorithms.level_index([dev(p) for p in A_pyr], [[dev(p) for p in q] for q in Ap_list], L - 1, rot=True)
        assert index.dbr is not None and index.dbk is not None
        Bp = [dev(b) for b in Bp_pyr]
        call = ia._LevelCall(L - 1, L, index, dev(B_pyr[L - 2]), dev(B_pyr[L - 1]), Bp[L - 2], Bp[L - 1],
                             _ia.to_dev(o.compute_weights(3, 5, 12, 1)), 0.5)
        run = lambda: _ia.check(lib.ia_synth_level(ctypes.byref(call.args), _ia.stream()), 'ia_synth_level')  # noqa: E731
        plan = _ia.level_plan(call.args)
        print('plan:', plan)
        assert plan['xw'] and plan['form'] == _ia.XW_STRIP and plan['r16'] and plan['strips']
        assert plan['rk'] and plan['split'] and plan['fused'] and not plan['peer']
        n0, c0 = lib.ia_diag_compact_waves(), counts()
        run()
        dn, dc = lib.ia_diag_compact_waves() - n0, counts() - c0
        print('as planned: compact waves %d, helper pixels %d' % (dn, dc[0]))
        assert dn > 0 and dc[0] > 0
        lib.ia_diag_set_xwave(1)
        plan = _ia.level_plan(call.args)
        assert plan['xw'] and plan['form'] == _ia.XW_IMG and not plan['rk'] and not plan['split']
        n0, c0 = lib.ia_diag_compact_waves(), counts()
        run()
        assert lib.ia_diag_compact_waves() == n0 and not (counts() - c0).any()
        _ia.sched_status()
    finally:
        lib.ia_diag_set_compact_min_rows(prev_compact)
        lib.ia_diag_set_xwave(prev_xwave)


# ---- ties and shares -----------------------------------------------------------------------------

def few_ties_inputs(seed, A_shape, B_shape):
    """(A, [A'], B): label_inputs inverted: A and A' textured everywhere but one flat 44 x 72
    rectangle inside a 128-column strip (A 0.25, A' 0.6), B flat 0.25 in its left half.  The flat
    rows are bit-identical and span a handful of strip segments."""
    from scipy.ndimage import gaussian_filter
    H, W = A_shape
    flat = np.zeros(A_shape, dtype=bool)
    r0, c0 = (H - 44) // 2, (W // 2) // 128 * 128 + 28
    flat[r0:r0 + 44, c0:c0 + 72] = True
    tex = 0.7 + 0.3 * smooth_noise(seed, A_shape)
    A = np.where(flat, 0.25, tex)
    Ap = np.where(flat, 0.6, gaussian_filter(tex, 1.0))
    B = np.full(B_shape, 0.25)
    half = B_shape[1] // 2
    B[:, half:] = (0.7 + 0.3 * smooth_noise(seed + 1, B_shape))[:, half:]
    return A, [Ap], B


def tie_case(name):
    from test_gpu_fallback import _CASES, LumCase, lum_case
    if name != 'few':
        return lum_case(name)
    if 'xsplit:few' not in _CASES:
        _CASES['xsplit:few'] = LumCase(few_ties_inputs(96, (256, 512), (16, 48)), 2, 1.0, 96)
    return _CASES['xsplit:few']


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['few', 'at'])
def test_split_ties_vs_oracle(gpu, xsplit, name):
    """Label maps whose flat finest-level queries tie, by the oracle alone (LumCase.ties), over
    between 2 and SEGCAP segments ('few': a handful; 'at': all 1024), so both workgroups of such a
    pixel hold rows at the winning distance.  With the split on the synthesis and every
    approximate pick equal the oracle's, some helpers rescored and some won; with it off both
    counters stand still and the results are the same (the oracle's)."""
    from test_gpu_fallback import run_profiled
    case = tie_case(name)
    ties, nseg = case.ties()
    # (a list of at least 2 segments is shared, and the tied segments are all listed)
    shared = int(((ties >= 2) & (ties <= SEGCAP)).sum())
    print('ties [%s]: %d segments, %d queries tied over 2..%d segments (most %d)'
          % (name, nseg, shared, SEGCAP, ties.max()))
    assert shared > 0 and ties.max() <= SEGCAP
    if name == 'few':
        assert ties.max() <= 16
    xsplit(1)
    c0 = counts()
    on = run_profiled(case)
    dc = counts() - c0
    print('ties [%s]: helper pixels %d, helper wins %d, candidate segments %d'
          % (name, dc[0], dc[1], on['candidate_segments']))
    assert dc[0] >= shared and dc[1] > 0
    assert on['full_scans'] == 0 and on['candidate_segments'] >= int(ties.sum())
    xsplit(0)
    c0 = counts()
    off = run_profiled(case)
    assert not (counts() - c0).any()
    for key in ('full_scans', 'candidate_segments', 'rows_rescored'):
        assert on[key] == off[key], key


# ---- full scans ----------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('name', ['over', 'const_exact@strip'])
def test_split_full_scans_stay_with_the_owner(gpu, xsplit, name):
    """The candidate list's overflow ('over': flat queries tie over more than 1024 segments) and
    the constant A / A' (amax == 0, every segment ties; as test_gpu_compact.py runs them) with the
    split on: the oracle's results, at least the reference count of full scans on 'over', and no
    helper counted for a pixel that scanned (a full scan is the owner's alone)."""
    from test_gpu_fallback import lum_case, run_profiled
    case = lum_case(name)
    xsplit(1)
    c0 = counts()
    rec = run_profiled(case)
    dc = counts() - c0
    pixels = case.queries[case.L - 1]
    print('full scans [%s]: %d of %d pixels, helper pixels %d' % (name, rec['full_scans'], pixels, dc[0]))
    if name == 'over':
        ties, nseg = case.ties()
        assert rec['full_scans'] >= int((ties > SEGCAP).sum()) > 0
    assert dc[0] <= pixels - rec['full_scans'] and dc[1] <= dc[0]
