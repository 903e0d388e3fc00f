"""CPU study (no GPU): candidate segments per query of a COMPACT R16 screen on c4's finest
database: only the leading C principal components are screened (P of them as split f16
pairs, C - P as single f16), 2P + 1 + C + 1 = 32 operand slots at C = 24, P = 3, one
v_mfma_f32_16x16x32_f16 per 16x16 block and 64 B per row.

With rho = V^T a', kappa = V^T q' split into the kept (C) and the rest components,

  e(r)   = |a'|^2 - 2 a'.q'                     the exact value (D(r) - |q'|^2)
  e_C(r) = |rho_C|^2 - 2 rho_C.kappa_C          what the compact screen carries
  e(r)   = e_C(r) - |kappa_rest|^2 + |rho_rest - kappa_rest|^2
        >= e_C(r) - |kappa_rest|^2 + max(0, |kappa_rest| - R_j)^2,   R_j = max over segment j of |rho_rest|

so with m_j the compact minimum of segment j and eps_j its rounding bound (ia_rot16.h rk_eps0:
u (360 A|q'| + 110 A^2 + 32 |q'|^2), plus the skipped cross terms per segment; the skip norms here
are those of components P..C-1, the shipped codes bound them by those of P..54), every row of
segment j has

  e(r) >= L_j = m_j - eps_j - |kappa_rest|^2 + rest_j,   rest_j = max(0, |kappa_rest| - R_j)^2 (or 0).

The compact minima are lower bounds only, so the exact stage rescores the segment with the
least L_j first, takes U = its exact minimum, and selects  L_j <= U.

Proxy as in askip_study.py: the screen's minima are replaced by their exact fp64 values.
Queries: the 512 real finest-level queries of tests/golden/c4_queries.npz with their pixels;
"clean" = y >= 1 and x >= 1 (no B' initialisation noise in the window's causal part).
Segments: 4 scanlines x 128 columns (512 rows).

Kept axes (--axes): the C screened components are C - n principal directions and n feature
axes (algorithms.compact_axes_basis, DESIGN.md §4d "Which waves"): `col` = 53, 54, the own-row B'
samples a column-0 pixel reflects onto pixels not yet synthesised; `row` = 43..47, 50, 51, 52, the
samples of rows y - 2 (all five) and y - 1 (x .. x + 2) a row-0 pixel reflects onto such pixels;
`both`; or a comma-separated list.

Border queries (--border N, default 64): N column-0 queries (y, 0) and N row-0 queries (0, x),
evenly spaced, rebuilt from tests/golden/c4_full.npz: B' of level l is A'[s_l]; the state at pixel
p is the final values before p in scanline order and initialize_Bp's values from p on.  The
captured border queries of c4_queries.npz are rebuilt the same way first and must come out equal.
The report is per class: clean / column-0 / row-0.

usage: python tools/compact_study.py [C [P]] [--axes col|row|both|k,k,...] [--border N]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'oracle'))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'image-analogies-python_amd'))

import ia_oracle as o  # noqa: E402
import make_config_fixtures as mf  # noqa: E402

U32 = 2.0 ** -24
E2 = 110.0         # ia_rot16.h RK_EPS_A2


def report(name, arr, rs):
    if not len(arr):
        return
    mx = [arr[rs.randint(0, len(arr), 342)].max() for _ in range(400)]
    print('    %-34s n %3d  mean %8.2f  p90 %6d  p99 %6d  max %6d   E[max of 342] %8.1f'
          % (name, len(arr), arr.mean(), *np.percentile(arr, [90, 99]).astype(int), arr.max(), np.mean(mx)))


AXES = {'col': [53, 54], 'row': [43, 44, 45, 46, 47, 50, 51, 52]}
AXES['both'] = AXES['row'] + AXES['col']


def border_query(B_pyr, Bp_init, Bp_final, level, px):
    """The query row of pixel px of a level: B' final before px in scanline order, initial from it on."""
    r, c = px
    W = B_pyr[level].shape[1]
    cur = Bp_init[level].copy()
    cur.flat[:r * W + c] = Bp_final[level].flat[:r * W + c]
    return np.hstack([o.extract_pixel_feature(B_pyr[level - 1], B_pyr[level], px, True),
                      o.extract_pixel_feature(Bp_final[level - 1], cur, px, False)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('C', type=int, nargs='?', default=24)
    ap.add_argument('P', type=int, nargs='?', default=3)
    ap.add_argument('--axes', default='')
    ap.add_argument('--border', type=int, default=64)
    args = ap.parse_args()
    C, P = args.C, args.P
    axes = AXES.get(args.axes) or [int(x) for x in args.axes.split(',') if x]
    t0 = time.time()
    A, Aps, B, k, cap, seed = mf.workload('c4')
    A_pyr, Ap_list, B_pyr, Bp_pyr, L = o.setup_luminance(A, Aps, B, cap=cap, seed=seed)
    As = o.create_index(A_pyr, Ap_list, L)[L - 1]
    H, W = A_pyr[L - 1].shape
    c = np.concatenate([np.full(34, A_pyr[L - 1].mean()), np.full(21, Ap_list[0][L - 1].mean())])
    a = As - c
    del As
    na = np.einsum('ij,ij->i', a, a)
    rs = np.random.RandomState(0)
    sub = a[rs.choice(len(a), 65536, replace=False)]
    w, V = np.linalg.eigh(sub.T @ sub / len(sub))
    V = V[:, ::-1]
    if axes:
        import algorithms
        Cov = sub.T @ sub / len(sub)
        V, _, nk = algorithms.compact_axes_basis(Cov, V, w[::-1].copy(), C, axes)
        print('kept span: %d principal directions + %d of the axes %s' % (C - nk, nk, axes))
    rho = a @ V
    var = (rho ** 2).sum(0)
    print('c4 finest DB %d rows built in %.0f s; leading 8/16/23/24/32 components hold %s of the energy'
          % (len(a), time.time() - t0, ' / '.join('%.5f' % (var[:n].sum() / var.sum()) for n in (8, 16, 23, 24, 32))))
    yy, xx = np.divmod(np.arange(len(a)), W)
    seg = (yy // 4) * (W // 128) + xx // 128
    nseg = seg.max() + 1
    order = np.argsort(seg, kind='stable')
    del yy, xx, seg

    rhoC = np.ascontiguousarray(rho[:, :C])
    naC = np.einsum('ij,ij->i', rhoC, rhoC)
    AC, Amax = np.sqrt(naC.max()), np.sqrt(na.max())
    rest = np.sqrt((rho[:, C:] ** 2).sum(1))
    skn = np.sqrt((rho[:, P:C] ** 2).sum(1))
    R_seg = rest[order].reshape(nseg, -1).max(1)
    ask_seg = skn[order].reshape(nseg, -1).max(1)
    print('C = %d, P = %d: %d slots; A_C %.4g; rest norm of the rows max %.4g median %.4g; per-segment R_j '
          'p10/p50/p90/max %.4f / %.4f / %.4f / %.4f'
          % (C, P, 2 * P + 1 + C + 1, AC, rest.max(), np.median(rest), *np.percentile(R_seg, [10, 50, 90, 100])))
    del rho, rest, skn

    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'c4_queries.npz'))
    n = int(g['n_captured'])
    Q, px = g['q'][:n], g['pixels'][:n]
    clean = (px[:, 0] >= 1) & (px[:, 1] >= 1)
    if args.border:
        # B' of every level from the full run's maps, then the border queries
        full = np.load(os.path.join(ROOT, 'tests', 'golden', 'c4_full.npz'))
        Bp_fin = [b.copy() for b in Bp_pyr]
        for l in range(1, L):
            sl = full['s%d' % l].astype(np.int64)
            Bp_fin[l] = Ap_list[0][l][sl[:, 0], sl[:, 1]].reshape(B_pyr[l].shape)
        worst = max(np.abs(border_query(B_pyr, Bp_pyr, Bp_fin, L - 1, tuple(p)) - q).max()
                    for p, q in zip(px[~clean], Q[~clean]))
        print('the %d captured border queries rebuilt from c4_full.npz: largest difference %r'
              % ((~clean).sum(), worst))
        assert worst == 0.0
        Hb, Wb = B_pyr[L - 1].shape
        ys = np.linspace(1, Hb - 1, args.border).astype(int)
        xs = np.linspace(1, Wb - 1, args.border).astype(int)
        pcol = [(int(y), 0) for y in ys]
        prow = [(0, int(x)) for x in xs]
        Q = np.vstack([Q[clean]] + [border_query(B_pyr, Bp_pyr, Bp_fin, L - 1, p) for p in pcol + prow])
        px = np.vstack([px[clean], np.array(pcol + prow)])
        n = len(Q)
        clean = (px[:, 0] >= 1) & (px[:, 1] >= 1)
    col0 = (px[:, 1] == 0) & (px[:, 0] >= 1)
    row0 = px[:, 0] == 0
    cnt = {False: [], True: []}
    dwin = []
    for m0 in range(0, n, 32):
        qq = Q[m0:m0 + 32] - c
        kap = qq @ V
        E = na[:, None] - 2.0 * (a @ qq.T)                                # exact e, rows x m
        xseg = E[order].reshape(nseg, -1, len(qq)).min(axis=1)            # exact segment minima
        dwin += list(xseg.min(0) + (qq ** 2).sum(1))
        del E
        EC = naC[:, None] - 2.0 * (rhoC @ kap[:, :C].T)
        mseg = EC[order].reshape(nseg, -1, len(qq)).min(axis=1)           # compact segment minima
        del EC
        nsk = np.sqrt((kap[:, P:C] ** 2).sum(1))
        nr = np.sqrt((kap[:, C:] ** 2).sum(1))
        # the shipped rule's rounding terms (rk_eps0: A, |q'| and the 32 |q'|^2 of the rotation)
        nq = np.sqrt((qq ** 2).sum(1))
        eps = U32 * (360 * Amax * nq + E2 * Amax ** 2 + 32 * nq ** 2)[None, :] + \
            2.0 ** -9 * 1.01 * ask_seg[:, None] * nsk[None, :]
        for with_rest in (False, True):
            rterm = np.maximum(0.0, nr[None, :] - R_seg[:, None]) ** 2 if with_rest else 0.0
            Lb = mseg - eps - (nr ** 2)[None, :] + rterm
            assert (Lb <= xseg + 1e-12).all(), 'not a lower bound'
            j0 = Lb.argmin(0)
            Ub = xseg[j0, np.arange(len(qq))]
            cnt[with_rest] += list((Lb <= Ub[None, :]).sum(0))
    print('median winner distance %.4g (mean row distance to a query: see askip_study)' % np.median(dwin))
    for with_rest in (False, True):
        arr = np.array(cnt[with_rest])
        print('  candidate segments per query, %s rest-norm term:' % ('with the' if with_rest else 'without a'))
        report('all captured queries', arr, rs)
        report('clean-wave queries (y>=1, x>=1)', arr[clean], rs)
        report('column-0 queries (y>=1, x=0)', arr[col0], rs)
        report('row-0 queries (y=0)', arr[row0], rs)
        if with_rest:
            # the split tail (DESIGN.md §6b "split"): arr = 1 + n (the seed and the n listed
            # segments); both workgroups rescore the seed, the slower one then ceil(n / 2) of the list
            n = arr[clean] - 1
            report('clean: 1 + n', 1 + n, rs)
            report('clean: 1 + ceil(n / 2)', 1 + (n + 1) // 2, rs)
    print('total %.0f s' % (time.time() - t0))


if __name__ == '__main__':
    main()
