"""The compact R16 screen (DESIGN.md §4d "compact"; csrc/ia_rot16.h RK_*): 24 leading components,
32 K-slots, one MFMA per 16 x 16 block on the waves without a row-0 or column-0 pixel.  Its
segment minima are lower bounds only: the bound the exact stage relies on holds for every (query,
segment) against numpy's fp64 minima, under the level's principal basis and under the reversed
one; whole syntheses with the compact form on equal the oracle and the compact form off, B', s
and im; so do the tie / full-scan cases; and no compact wave holds a row-0 or column-0 pixel."""
import ctypes
import math

import numpy as np
import pytest

import ia_oracle as o
import ia_oracle_c as oc
from conftest import analogy_inputs

U32 = 2.0 ** -24
RK_C, R16_P = 24, 3        # ia_rot16.h: kept components, components with cross terms
RK_EPS_A2 = 110.0          # ia_rot16.h RK_EPS_A2


@pytest.fixture
def compact():
    """Set the compact form's row threshold for one test (0: off); restored after it."""
    import _ia
    lib = _ia.lib()
    prev = lib.ia_diag_set_compact_min_rows(-1)
    yield lambda rows: lib.ia_diag_set_compact_min_rows(rows)
    lib.ia_diag_set_compact_min_rows(prev)


# ---- the wave rule (host only) -------------------------------------------------------------------

@pytest.mark.parametrize('H', [1, 2, 3, 7, 128])
@pytest.mark.parametrize('W', [1, 2, 3, 7, 128])
def test_no_compact_wave_holds_a_border_pixel(H, W):
    """Every wave the host would run compact (ia_diag_wave_compact) holds no pixel of row 0 or
    column 0 (their windows hold B' initialisation noise, which lies in the dropped components);
    and from W = 7 up some wave is compact."""
    import _ia
    lib = _ia.lib()
    out = (ctypes.c_int * 5)()
    _ia.check(lib.ia_diag_wave_rows(H, W, 0, 0, 0, out), 'ia_diag_wave_rows')
    nw, seen, ncompact = out[2], 0, 0
    for t in range(nw):
        _ia.check(lib.ia_diag_wave_rows(H, W, t, 0, 0, out), 'ia_diag_wave_rows')
        y_lo, M = out[0], out[1]
        px = [(y, t - 3 * y) for y in range(y_lo, y_lo + M)]
        assert all(0 <= y < H and 0 <= x < W for y, x in px)
        seen += len(px)
        if lib.ia_diag_wave_compact(W, t):
            ncompact += 1
            assert all(y >= 1 and x >= 1 for y, x in px), (H, W, t)
    assert seen == H * W
    if H >= 7 and W >= 7:
        assert ncompact > 0


# ---- the bound -----------------------------------------------------------------------------------

def _bound_level(seed, shape, reverse, monkeypatch):
    """The finest level of a 2-level analogy with two A' images, its compact DB built (threshold
    1), the oracle's rows and 48 queries: real wave queries of a small B (the oracle's synthesis,
    row 0 and column 0 included), DB rows and uniform noise."""
    import algorithms
    from test_gpu_fallback import queries_from
    from test_gpu_split16 import dev
    if reverse:     # components by INCREASING variance: the kept ones hold the least energy
        eigh = algorithms._eigh
        monkeypatch.setattr(algorithms, '_eigh', lambda C: tuple(x[..., ::-1].copy() for x in eigh(C)))
    A, Aps, B = analogy_inputs(seed, shape, (9, 12), n_ap=2)
    A_pyr, Ap_list, B_pyr, Bp_pyr, L = o.setup_luminance(A, Aps, B, cap=2, seed=seed)
    idx = algorithms.level_index([dev(p) for p in A_pyr], [[dev(p) for p in q] for q in Ap_list], L - 1, rot=True)
    assert idx.dbr is not None and idx.dbk is not None, 'the compact DB applies to a strip level'
    As = o.create_index(A_pyr, Ap_list, L)[L - 1]
    Bp = [b.copy() for b in Bp_pyr]
    oc.synthesize(A_pyr, Ap_list, B_pyr, Bp, L, 0.5, o.compute_weights(3, 5, 12, 1))
    Qw = queries_from(L - 1, B_pyr, Bp_pyr, Bp)                # 108 pixels in scanline order
    rs = np.random.RandomState(seed)
    Q = np.vstack([Qw[:12], Qw[12::12][:8], Qw[rs.choice(np.arange(13, len(Qw)), 16, replace=False)],
                   As[rs.randint(0, len(As), 4)], rs.rand(8, 55)])
    assert len(Q) == 48
    return idx, As, Q


@pytest.mark.gpu
@pytest.mark.parametrize('reverse', [False, True])
@pytest.mark.parametrize('shape', [(64, 128), (40, 256)])
def test_compact_minima_are_lower_bounds(gpu, compact, monkeypatch, shape, reverse):
    """For every (query, segment): the compact minimum is within eps_j of numpy's fp64 minimum of
    e_C over the segment's rows, and the bound the exact stage selects by,
    L_j = m_j - eps_j - k^2 + max(0, k - R_j)^2 (k = |kappa_rest|, R_j the decoded rest-norm bound),
    is at most numpy's fp64 minimum of e = |a'|^2 - 2 a'.q' over them (ia_rot16.h)."""
    import torch
    import _ia
    from test_gpu_split16 import Q16_HALVES, _scales, _segment_order, dev
    compact(1)
    idx, As, Q = _bound_level(31 + shape[0], shape, reverse, monkeypatch)
    lib = _ia.lib()
    M, N = len(Q), len(As)
    npad = lib.ia_db_rows_padded(N)
    seg = min(lib.ia_db_chunk_rows(N), 512)
    nseg = npad // seg
    assert npad == N
    order = _segment_order(idx, N, npad, seg)
    amax = float(idx.amax.cpu().numpy()[0])
    askip = float(idx.amax.cpu().numpy()[1])
    c = idx.center.cpu().numpy()
    a = As - c
    V = idx.rot.cpu().numpy()[:56 * 56].reshape(56, 56)[:55, :55].astype(np.float64)
    rho = a @ V
    # the buffers' per-segment bounds: skip codes (rotated DB), rest norms and codes (compact DB)
    al = lambda n: (n + 255) // 256 * 256  # noqa: E731
    tail = idx.dbr.view(torch.uint8)[npad * lib.ia_db_rot_slots() * 2:]
    ask_dec = askip * tail[al(4 * nseg):][:nseg].cpu().numpy().astype(np.float64) / 255.0
    assert len(idx.dbk) == lib.ia_db_rotk_bytes(N) == npad * 64 + al(4 * nseg) + al(nseg) + 256
    tk = idx.dbk.view(torch.uint8)[npad * 64:]
    R_seg = tk[:4 * nseg].view(torch.float32).cpu().numpy().astype(np.float64)
    codes = tk[al(4 * nseg):][:nseg].cpu().numpy().astype(np.float64)
    rmax = float(tk[al(4 * nseg) + al(nseg):][:4].view(torch.float32).cpu().numpy()[0])
    rest = np.sqrt((rho[:, RK_C:] ** 2).sum(1))
    assert (rest[order].reshape(nseg, seg).max(1) <= R_seg).all() and R_seg.max() == rmax
    R_dec = rmax * codes / 255.0
    assert (R_dec >= R_seg).all() and (codes <= 255).all()
    skn = np.sqrt((rho[:, R16_P:RK_C] ** 2).sum(1))
    assert (skn[order].reshape(nseg, seg).max(1) <= ask_dec * (1 + 1e-6)).all()
    # numpy's fp64 segment minima: e over all components, e_C over the kept ones
    kap = (Q - c) @ V
    E = np.einsum('ij,ij->i', a, a)[:, None] - 2.0 * (a @ (Q - c).T)
    EC = (rho[:, :RK_C] ** 2).sum(1)[:, None] - 2.0 * (rho[:, :RK_C] @ kap[:, :RK_C].T)
    exact = E[order].reshape(nseg, seg, M).min(axis=1).T
    exactC = EC[order].reshape(nseg, seg, M).min(axis=1).T

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
    worst, worst_lb = 0.0, -np.inf
    for m in range(M):
        assert nrest[m] == pytest.approx(float((kap[m, RK_C:] ** 2).sum()), rel=1e-9, abs=1e-300)
        assert nsks[m] == pytest.approx(float((kap[m, R16_P:] ** 2).sum()), rel=1e-9, abs=1e-300)
        ea, R, eq = _scales(amax, float(nqs[m]))
        mj = np.ldexp(got[m], -(ea + eq))
        eps = U32 * (360 * amax * math.sqrt(nqs[m]) + RK_EPS_A2 * amax * amax + 32 * nqs[m]) + \
            2.0 ** -9 * 1.01 * ask_dec * math.sqrt(nsks[m])
        worst = max(worst, (np.abs(mj - exactC[m]) / eps).max())
        k = math.sqrt(nrest[m])
        L = mj - eps - k * k + np.maximum(0.0, k - R_dec) ** 2
        # (numpy's own rounding of e: a few ulps of |a'|^2 + 2 |a'||q'|)
        worst_lb = max(worst_lb, (L - exact[m] - 1e-13 * (amax * amax + nqs[m])).max())
    print('compact screen %s%s: worst |m_j - min e_C| / eps_j = %.3g; max (L_j - min e) = %.3g'
          % (shape, ' reversed' if reverse else '', worst, worst_lb))
    assert worst < 1.0
    assert worst_lb <= 0.0


# ---- syntheses -----------------------------------------------------------------------------------

def _synth(pyr, compact_rows, compact):
    import _ia
    import image_analogies as ia
    from test_gpu_split16 import dev
    compact(compact_rows)
    A_pyr, Ap_list, B_pyr, Bp_pyr, L = pyr
    d = lambda p: [dev(x) for x in p]  # noqa: E731
    Bp = d(Bp_pyr)
    out = ia.synthesize_dev(d(A_pyr), [d(p) for p in Ap_list], d(B_pyr), Bp, L, 0.5,
                            _ia.to_dev(o.compute_weights(3, 5, 12, 1)))
    return {l: (Bp[l].cpu().numpy(), s.cpu().numpy(), im.cpu().numpy()) for l, (s, im) in out.items()}


@pytest.mark.gpu
@pytest.mark.parametrize('shape_A,shape_B', [((128, 128), (37, 41)), ((32, 256), (24, 50))])
def test_compact_synthesis_equals_oracle_and_compact_off(gpu, compact, monkeypatch, shape_A, shape_B):
    """A whole synthesis with the compact form on (threshold 1, the rotated screen on levels of
    any size: the finest, strip-order level takes it on its clean waves; every border class and
    t mod 3) equals the oracle's and the compact form off, B', s and im of every level; the
    library counts at least the finest level's clean waves as compact, and none with it off."""
    import _ia
    import algorithms
    from test_gpu_split16 import dev
    monkeypatch.setenv('IA_ROT_MIN_ROWS', '1')
    waves = _ia.lib().ia_diag_compact_waves
    A, Aps, B = analogy_inputs(57, shape_A, shape_B, n_ap=1)
    pyr = o.setup_luminance(A, Aps, B, cap=2, seed=57)
    A_pyr, Ap_list, B_pyr, Bp_pyr, L = pyr
    ref = oc.synthesize(A_pyr, Ap_list, B_pyr, [b.copy() for b in Bp_pyr], L, 0.5, o.compute_weights(3, 5, 12, 1))
    n0 = waves()
    on = _synth(pyr, 1, compact)
    H, W = shape_B
    clean = sum(1 for t in range(W, W + 3 * (H - 1)) if t % 3)
    assert waves() - n0 >= clean > 0
    # (the compact DB is what the level took: built under this threshold, not without it)
    index = lambda: algorithms.level_index([dev(p) for p in A_pyr], [[dev(p) for p in q] for q in Ap_list],  # noqa: E731
                                           L - 1, rot=True)
    assert index().dbk is not None
    n0 = waves()
    off = _synth(pyr, 0, compact)
    assert index().dbk is None and waves() == n0
    assert set(on) == set(off) == set(ref)
    for l in sorted(ref):
        for got in (on[l], off[l]):
            assert np.array_equal(got[1], ref[l][1]) and np.array_equal(got[2], ref[l][2]), l
            assert np.array_equal(got[0], ref[l][0]), l


@pytest.mark.gpu
@pytest.mark.parametrize('name', ['const_exact@strip', 'over'])
def test_compact_ties_and_full_scan_vs_oracle(gpu, compact, name):
    """Constant A / A' (every segment ties, amax == 0: the forced full scan) and the label map
    whose flat queries tie over more than 1024 segments (the candidate list's overflow), with the
    compact form on: B', s, im and the approximate picks equal the oracle's, and the overflow
    case reports at least the reference count of full scans."""
    import _ia
    from test_gpu_fallback import SEGCAP, lum_case, run_profiled
    case = lum_case(name)
    compact(1)
    n0 = _ia.lib().ia_diag_compact_waves()
    rec = run_profiled(case)
    H, W = case.pyr[2][case.L - 1].shape
    assert _ia.lib().ia_diag_compact_waves() - n0 >= sum(1 for t in range(W, W + 3 * (H - 1)) if t % 3) > 0
    if name == 'over':
        ties, nseg = case.ties()
        assert rec['full_scans'] >= int((ties > SEGCAP).sum()) > 0

