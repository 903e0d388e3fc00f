"""Column-0 waves on the compact screen (DESIGN.md §4d "Which waves"), host side only: the basis
that keeps the own-row axes inside the compact span (algorithms.compact_axes_basis) and the wave
classes (ia_diag_wave_compact / ia_diag_wave_compact_col)."""
import ctypes

import numpy as np
import pytest


def _span():
    import algorithms
    kept, axes = algorithms.rotk_span()
    assert kept > len(axes) == 2 and all(0 <= k < 55 for k in axes) and axes[0] != axes[1]
    return kept, axes


def _pca(C):
    w, V = np.linalg.eigh(C)
    return V[:, ::-1].copy(), w[::-1].copy()


def _inputs(kept, axes):
    """name -> (C, V, var, axes expected to be kept)."""
    rs = np.random.RandomState(5)
    X = rs.standard_normal((55, 55))
    spd = X @ X.T / 55 + 0.01 * np.eye(55)
    eye = np.eye(55)
    var = np.linspace(2.0, 1.0, 55)
    # one axis inside the leading columns (its unit vector is column 0) and one outside: the other
    # axis's unit vector sits past the compact span
    P = np.eye(55)
    order = [axes[0]] + [k for k in range(55) if k not in axes] + [axes[1]]
    one = P[:, order]
    return {
        'spd': (spd,) + _pca(spd) + (list(axes),),
        # (the unit matrix: both axes are columns 53 and 54, outside the span)
        'identity': (np.diag(var), eye.copy(), var.copy(), list(axes)),
        # (reversed: the axes are columns 0 and 1)
        'reversed': (np.diag(var[::-1]), eye[:, ::-1].copy(), var.copy(), []),
        'one_in_one_out': (one @ np.diag(var) @ one.T, one.copy(), var.copy(), [axes[1]]),
    }


@pytest.mark.parametrize('name', ['spd', 'identity', 'reversed', 'one_in_one_out'])
def test_compact_axes_basis(name):
    """V' is orthonormal to 1e-12, leaves the leading kept - 2 columns of V untouched, holds every
    kept axis inside its first `kept` columns to 1e-12, reports the axes it kept, gives var' =
    diag(V'^T C V') with the complement's directions by decreasing variance, and is deterministic;
    with both axes already inside the leading columns V comes back unchanged."""
    import algorithms
    kept, axes = _span()
    C, V, var, want = _inputs(kept, axes)[name]
    V0, var0 = V.copy(), var.copy()
    Vn, varn, n = algorithms.compact_axes_basis(C, V, var, kept, axes)
    assert np.array_equal(V, V0) and np.array_equal(var, var0)          # the inputs are not written
    assert n == len(want)
    assert Vn.shape == (55, 55) and varn.shape == (55,)
    err = np.linalg.norm(Vn.T @ Vn - np.eye(55))
    print('%s: kept %d axes, |V^T V - I| = %.3g' % (name, n, err))
    assert err <= 1e-12
    assert np.array_equal(Vn[:, :kept - 2], V0[:, :kept - 2])
    assert np.array_equal(Vn[:, :kept - n], V0[:, :kept - n])
    K = Vn[:, :kept]
    for k in want:
        e = np.zeros(55)
        e[k] = 1.0
        assert np.linalg.norm(e - K @ (K.T @ e)) <= 1e-12, k
    if n == 0:
        assert np.array_equal(Vn, V0) and np.array_equal(varn, var0)
    else:
        assert np.allclose(varn, np.diag(Vn.T @ C @ Vn), rtol=0, atol=1e-12 * np.abs(C).max())
        assert (np.diff(varn[kept:]) <= 1e-12 * np.abs(C).max()).all()
        # the complement's columns diagonalise C there
        G = Vn[:, kept:].T @ C @ Vn[:, kept:]
        assert np.abs(G - np.diag(np.diag(G))).max() <= 1e-12 * np.abs(C).max()
    V2, var2, n2 = algorithms.compact_axes_basis(C, V0.copy(), var0.copy(), kept, axes)
    assert n2 == n and np.array_equal(V2, Vn) and np.array_equal(var2, varn)


@pytest.mark.parametrize('H', [1, 2, 3, 7, 128])
@pytest.mark.parametrize('W', [1, 2, 3, 7, 128])
def test_wave_classes(H, W):
    """Over every wave of an H x W level (ia_diag_wave_rows): a column-compact wave holds no row-0
    pixel and, while t = 3y names a row of the level (t <= 3 (H - 1)), exactly one pixel with
    x = 0, (t / 3, 0) with y >= 1; past the last row (W >= 5: t = 3 H .. W + 3 H - 4) it holds no
    border pixel at all.  Every wave with t >= W is exactly one of clean-compact and
    column-compact; no wave before it is either."""
    import _ia
    lib = _ia.lib()
    out = (ctypes.c_int * 5)()
    _ia.check(lib.ia_diag_wave_rows(H, W, 0, 0, 0, out), 'ia_diag_wave_rows')
    nw, ncol = out[2], 0
    for t in range(nw):
        _ia.check(lib.ia_diag_wave_rows(H, W, t, 0, 0, out), 'ia_diag_wave_rows')
        px = [(y, t - 3 * y) for y in range(out[0], out[0] + out[1])]
        clean, col = lib.ia_diag_wave_compact(W, t), lib.ia_diag_wave_compact_col(W, t)
        assert clean in (0, 1) and col in (0, 1)
        assert clean + col == (1 if t >= W else 0), (H, W, t)
        if col:
            ncol += 1
            assert all(y >= 1 for y, x in px), (H, W, t)
            x0 = [(y, x) for y, x in px if x == 0]
            assert x0 == ([(t // 3, 0)] if t <= 3 * (H - 1) else []), (H, W, t)
        if clean:
            assert all(y >= 1 and x >= 1 for y, x in px), (H, W, t)
    assert ncol == sum(1 for t in range(W, nw) if t % 3 == 0)
    if H >= 7 and W >= 7:
        assert ncol > 0
