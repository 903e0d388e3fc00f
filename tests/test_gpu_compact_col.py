"""Column-0 waves on the compact screen (DESIGN.md §4d "Which waves"): where a level takes the
compact DB its basis keeps the own-row axes e_53 and e_54 inside the 24 screened components
(algorithms.compact_axes_basis), and the waves t = 3y >= W, whose only border pixel is (y, 0), run
the compact screen and the compact tail too.  Whole syntheses with the switch on and off, with and
without the split tail, equal the oracle and count exactly the waves they should; the compact
bound holds for the column-0 queries; the tie / full-scan cases and the reversed basis equal the
oracle; arguments that do not claim the axes keep the clean waves only."""
import ctypes
import math

import numpy as np
import pytest

import ia_oracle as o
import ia_oracle_c as oc
from conftest import analogy_inputs

pytestmark = pytest.mark.gpu


@pytest.fixture
def knobs(monkeypatch):
    """The run-time switches of these tests: the compact threshold 1 and IA_ROT_MIN_ROWS=1 (every
    level takes the rotated screen, every strip-order level the compact DB), the column switch on;
    returns the library.
    The compact threshold, the column switch and the split threshold are restored afterwards."""
    import _ia
    lib = _ia.lib()
    prev = (lib.ia_diag_set_compact_min_rows(-1), lib.ia_diag_set_compact_col(-1),
            lib.ia_diag_set_xsplit_min_rows(-1))
    monkeypatch.setenv('IA_ROT_MIN_ROWS', '1')
    lib.ia_diag_set_compact_min_rows(1)
    lib.ia_diag_set_compact_col(1)
    yield lib
    lib.ia_diag_set_compact_min_rows(prev[0])
    lib.ia_diag_set_compact_col(prev[1])
    lib.ia_diag_set_xsplit_min_rows(prev[2])


@pytest.fixture
def built(monkeypatch):
    """(level, index) of every index algorithms.level_index builds during the test."""
    import algorithms
    real = algorithms.level_index
    out = []

    def spy(A_pyr, Ap_pyr_list, level, *a, **k):
        idx = real(A_pyr, Ap_pyr_list, level, *a, **k)
        out.append((level, idx))
        return idx
    monkeypatch.setattr(algorithms, 'level_index', spy)
    return out


def wave_counts(shape):
    """(waves past row 0, the clean ones among them) of an H x W level."""
    H, W = shape
    ts = range(W, W + 3 * (H - 1))
    return len(ts), sum(1 for t in ts if t % 3)


def expected_compact_waves(built, B_pyr, col):
    """The compact waves of one synthesis from the indices it built: per level with a compact DB
    every wave past row 0 where the switch is on and the basis keeps both axes, else the clean
    ones."""
    n = 0
    for level, idx in built:
        if idx.dbk is not None:
            every, clean = wave_counts(B_pyr[level].shape)
            n += every if col and idx.rot_axes == 2 else clean
    return n


# ---- syntheses -----------------------------------------------------------------------------------

_REF = {}


def _small(shape_A, shape_B):
    """The small syntheses of test_gpu_compact.py and their oracle run (once per module)."""
    key = (shape_A, shape_B)
    if key not in _REF:
        A, Aps, B = analogy_inputs(57, shape_A, shape_B, n_ap=1)
        pyr = o.setup_luminance(A, Aps, B, cap=2, seed=57)
        A_pyr, Ap_list, B_pyr, Bp_pyr, L = pyr
        ref = oc.synthesize(A_pyr, Ap_list, B_pyr, [b.copy() for b in Bp_pyr], L, 0.5,
                            o.compute_weights(3, 5, 12, 1))
        _REF[key] = (pyr, ref)
    return _REF[key]


def _assert_equal(got, ref):
    assert set(got) == set(ref)
    for l in sorted(ref):
        assert np.array_equal(got[l][1], ref[l][1]) and np.array_equal(got[l][2], ref[l][2]), l
        assert np.array_equal(got[l][0], ref[l][0]), l


@pytest.mark.parametrize('shape_A,shape_B', [((128, 128), (37, 41)), ((32, 256), (24, 50))])
def test_column_waves_synthesis_equals_oracle(gpu, knobs, built, shape_A, shape_B):
    """The column switch on and off, crossed with the split tail on and off: B', s and im of every
    level equal the C oracle's; the finest level's basis keeps both axes with the switch on and
    is the plain principal one with it off; the compact-wave counter
    advances by every wave t in [W, W + 3 (H - 1)) of the compact levels with the switch on and by
    those with t % 3 != 0 with it off."""
    from test_gpu_compact import _synth
    lib = knobs
    pyr, ref = _small(shape_A, shape_B)
    B_pyr, L = pyr[2], pyr[4]
    every, clean = wave_counts(shape_B)
    assert every > clean > 0
    for col in (1, 0):
        for split in (1, 0):
            lib.ia_diag_set_compact_col(col)
            lib.ia_diag_set_xsplit_min_rows(split)
            assert lib.ia_diag_set_compact_col(-1) == col
            del built[:]
            n0 = lib.ia_diag_compact_waves()
            got = _synth(pyr, 1, lib.ia_diag_set_compact_min_rows)
            dn = lib.ia_diag_compact_waves() - n0
            finest = [idx for level, idx in built if level == L - 1]
            # (the basis keeps the axes only for a process that runs the column waves)
            assert len(finest) == 1 and finest[0].dbk is not None and finest[0].rot_axes == (2 if col else 0)
            want = expected_compact_waves(built, B_pyr, col)
            print('column %d split %d: compact waves %d (finest level: %d of %d past row 0)'
                  % (col, split, dn, every if col else clean, every))
            assert want >= (every if col else clean)
            assert dn == want
            _assert_equal(got, ref)


# ---- the bound on the column-0 queries -----------------------------------------------------------

@pytest.mark.parametrize('shape', [(64, 128), (40, 256)])
def test_compact_bound_holds_on_column_queries(gpu, knobs, monkeypatch, shape):
    """test_gpu_compact.py's level with the basis that keeps the axes: e_53 and e_54 lie inside the
    span of the rotation's first 24 columns (fp32) to 1e-5, and for the column-0 wave queries of
    the small B (pixels (y, 0), y >= 1) the bound the exact stage selects by,
    L_j = m_j - eps_j - k^2 + max(0, k - R_j)^2 (eps_j as in test_compact_minima_are_lower_bounds),
    is at most numpy's fp64 minimum of e = |a'|^2 - 2 a'.q' over every segment."""
    import torch
    import _ia
    import algorithms
    from test_gpu_compact import RK_C, RK_EPS_A2, U32, _bound_level
    from test_gpu_split16 import Q16_HALVES, _scales, _segment_order, dev
    lib = knobs
    kept, axes = algorithms.rotk_span()
    assert kept == RK_C and axes == [53, 54]
    idx, As, Q = _bound_level(31 + shape[0], shape, False, monkeypatch)
    assert idx.rot_axes == 2
    Q = Q[12:20]                     # _bound_level: Qw[12::12][:8], pixels (1, 0) .. (8, 0) of the 9 x 12 B
    M, N = len(Q), len(As)
    npad = lib.ia_db_rows_padded(N)
    seg = min(lib.ia_db_chunk_rows(N), 512)
    nseg = npad // seg
    assert npad == N and M == 8
    order = _segment_order(idx, N, npad, seg)
    amax, askip = (float(x) for x in idx.amax.cpu().numpy())
    c = idx.center.cpu().numpy()
    a = As - c
    V = idx.rot.cpu().numpy()[:56 * 56].reshape(56, 56)[:55, :55].astype(np.float64)
    K = V[:, :RK_C]
    for k in axes:
        e = np.zeros(55)
        e[k] = 1.0
        res = np.linalg.norm(e - K @ (K.T @ e))
        print('|(I - V24 V24^T) e_%d| = %.3g' % (k, res))
        assert res <= 1e-5
    al = lambda n: (n + 255) // 256 * 256  # noqa: E731
    tail = idx.dbr.view(torch.uint8)[npad * lib.ia_db_rot_slots() * 2:]
    ask_dec = askip * tail[al(4 * nseg):][:nseg].cpu().numpy().astype(np.float64) / 255.0
    tk = idx.dbk.view(torch.uint8)[npad * 64:]
    codes = tk[al(4 * nseg):][:nseg].cpu().numpy().astype(np.float64)
    rmax = float(tk[al(4 * nseg) + al(nseg):][:4].view(torch.float32).cpu().numpy()[0])
    R_dec = rmax * codes / 255.0
    rho = a @ V
    rest = np.sqrt((rho[:, RK_C:] ** 2).sum(1))
    assert (rest[order].reshape(nseg, seg).max(1) <= R_dec).all()
    kap = (Q - c) @ V
    E = np.einsum('ij,ij->i', a, a)[:, None] - 2.0 * (a @ (Q - c).T)
    exact = E[order].reshape(nseg, seg, M).min(axis=1).T

    qrows = lib.ia_diag_qp_rows(M)
    q64 = torch.zeros((M, _ia.IA_DP), dtype=torch.float64, device='cuda')
    q64[:, :55] = dev(Q)
    q16 = torch.zeros((qrows, Q16_HALVES), dtype=torch.float16, device='cuda')
    nq = torch.zeros(qrows, dtype=torch.float64, device='cuda')
    nsk = torch.zeros(qrows, dtype=torch.float64, device='cuda')
    segmin = torch.full((qrows, nseg), float('nan'), dtype=torch.float32, device='cuda')
    _ia.check(lib.ia_diag_screen16k(ctypes.byref(idx.src), idx.row0, N, _ia.ptr(idx.dbk), _ia.ptr(idx.rot),
                                    _ia.ptr(idx.amax), _ia.ptr(idx.center), _ia.ptr(q64), M, _ia.ptr(q16),
                                    _ia.ptr(nq), _ia.ptr(nsk), _ia.ptr(segmin), _ia.stream()), 'ia_diag_screen16k')
    torch.cuda.synchronize()
    got = segmin[:M].cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    nqs, nsks = nq.cpu().numpy(), nsk.cpu().numpy()
    nrest = q16[:M].view(torch.float64)[:, 24].cpu().numpy()       # byte 192 of each row
    worst_lb, ncand = -np.inf, []
    for m in range(M):
        assert nrest[m] == pytest.approx(float((kap[m, RK_C:] ** 2).sum()), rel=1e-9, abs=1e-300)
        ea, R, eq = _scales(amax, float(nqs[m]))
        mj = np.ldexp(got[m], -(ea + eq))
        eps = U32 * (360 * amax * math.sqrt(nqs[m]) + RK_EPS_A2 * amax * amax + 32 * nqs[m]) + \
            2.0 ** -9 * 1.01 * ask_dec * math.sqrt(nsks[m])
        k = math.sqrt(nrest[m])
        L = mj - eps - k * k + np.maximum(0.0, k - R_dec) ** 2
        # (numpy's own rounding of e: a few ulps of |a'|^2 + 2 |a'||q'|)
        worst_lb = max(worst_lb, (L - exact[m] - 1e-13 * (amax * amax + nqs[m])).max())
        ncand.append(int((L <= exact[m, int(L.argmin())]).sum()))
    print('column-0 queries %s: max (L_j - min e) = %.3g; candidate segments per query %s of %d'
          % (shape, worst_lb, ncand, nseg))
    assert worst_lb <= 0.0


# ---- ties and full scans -------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['const_exact@strip', 'over'])
def test_column_waves_ties_and_full_scan_vs_oracle(gpu, knobs, built, name):
    """test_compact_ties_and_full_scan_vs_oracle's cases with the column switch on: the constant
    A / A' (a zero covariance: whatever basis comes back, every query scans) and the label map
    whose flat queries tie over more than 1024 segments: the oracle's B', s, im and approximate
    picks, every wave past row 0 compact where the basis keeps both axes (else the clean ones),
    and on the overflow case at least the oracle-derived count of full scans."""
    from test_gpu_fallback import SEGCAP, lum_case, run_profiled
    lib = knobs
    case = lum_case(name)
    lib.ia_diag_set_compact_col(1)
    n0 = lib.ia_diag_compact_waves()
    rec = run_profiled(case)
    dn = lib.ia_diag_compact_waves() - n0
    every, clean = wave_counts(case.pyr[2][case.L - 1].shape)
    want = expected_compact_waves(built, case.pyr[2], 1)
    print('%s: compact waves %d (finest level: %d past row 0, %d clean), axes kept %s, full scans %d'
          % (name, dn, every, clean, [idx.rot_axes for _, idx in built], rec['full_scans']))
    assert dn == want >= clean > 0
    if name == 'over':
        assert want >= every        # (a textured label map: both axes lie outside the leading columns)
        ties, nseg = case.ties()
        assert rec['full_scans'] >= int((ties > SEGCAP).sum()) > 0


# ---- the reversed basis --------------------------------------------------------------------------

def test_column_waves_under_reversed_basis(gpu, knobs, built, monkeypatch):
    """_eigh reversed, as test_gpu_compact.py patches it (the kept principal columns hold the least
    energy, so the candidate lists are long) with the column switch on: the axes are still kept,
    every wave past row 0 of the finest level runs compact, and the results equal the oracle's."""
    import algorithms
    from test_gpu_compact import _synth
    lib = knobs
    eigh = algorithms._eigh
    monkeypatch.setattr(algorithms, '_eigh', lambda C: tuple(x[..., ::-1].copy() for x in eigh(C)))
    pyr, ref = _small((128, 128), (37, 41))
    lib.ia_diag_set_compact_col(1)
    n0 = lib.ia_diag_compact_waves()
    got = _synth(pyr, 1, lib.ia_diag_set_compact_min_rows)
    dn = lib.ia_diag_compact_waves() - n0
    finest = [idx for level, idx in built if level == pyr[4] - 1]
    assert len(finest) == 1 and finest[0].rot_axes == 2
    assert dn == expected_compact_waves(built, pyr[2], 1) >= wave_counts((37, 41))[0]
    _assert_equal(got, ref)


# ---- hand-built arguments ------------------------------------------------------------------------

def test_arguments_without_the_axes_keep_the_clean_waves(gpu, knobs):
    """The finest level of the small synthesis called directly: as the level call builds its
    arguments (rot_axes = 2) ia_diag_level_compact_col says 1, and 0 with the switch off; with
    rot_axes = 0, as arguments built by hand have it, it says 0 and running the level advances the
    counter by the clean waves only."""
    import algorithms
    import image_analogies as ia
    import _ia
    from test_gpu_split16 import dev
    lib = knobs
    pyr, _ = _small((128, 128), (37, 41))
    A_pyr, Ap_list, B_pyr, Bp_pyr, L = pyr
    index = algorithms.level_index([dev(p) for p in A_pyr], [[dev(p) for p in q] for q in Ap_list], L - 1, rot=True)
    assert index.dbk is not None and index.rot_axes == 2
    Bp = [dev(b) for b in Bp_pyr]
    call = ia._LevelCall(L - 1, L, index, dev(B_pyr[L - 2]), dev(B_pyr[L - 1]), Bp[L - 2], Bp[L - 1],
                         _ia.to_dev(o.compute_weights(3, 5, 12, 1)), 0.5)
    every, clean = wave_counts(B_pyr[L - 1].shape)

    def run():
        n0 = lib.ia_diag_compact_waves()
        _ia.check(lib.ia_synth_level(ctypes.byref(call.args), _ia.stream()), 'ia_synth_level')
        _ia.sched_status()
        return lib.ia_diag_compact_waves() - n0

    lib.ia_diag_set_compact_col(1)
    assert call.args.rot_axes == 2 and _ia.level_plan(call.args)['rk']
    assert lib.ia_diag_level_compact_col(ctypes.byref(call.args), 1) == 1
    assert lib.ia_diag_level_compact_col(ctypes.byref(call.args), 2) == 0       # (a batch has no compact waves)
    lib.ia_diag_set_compact_col(0)
    assert lib.ia_diag_level_compact_col(ctypes.byref(call.args), 1) == 0
    lib.ia_diag_set_compact_col(1)
    assert run() == every
    call.args.rot_axes = 0
    assert _ia.level_plan(call.args)['rk']
    assert lib.ia_diag_level_compact_col(ctypes.byref(call.args), 1) == 0
    assert run() == clean
