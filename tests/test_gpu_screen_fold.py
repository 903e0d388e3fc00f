"""The new fold and segment close of the 16x16x32 screens (csrc/ia_screen16r.hip: fold4, the lane-swap
close close_blocks_s16), in the two kernels that take them: the compact screen k_screen16c
(ia_diag_screen16k) and the 64-slot wave form k_screen16w (ia_diag_screen16r under
ia_diag_set_r16_form(1); k_screen16r and k_screen16rs keep the code they had and are not this
file's subject).  A (query, segment) minimum is the least of the segment's MFMA values whichever
accumulator element, lane group, row block, tile or chain holds it, and whichever query slot,
query block or wave carries the query.  So

* one query put into all M slots gives M equal rows of minima, bit for bit, at M = 32 .. 400
  (G = 1, 2, 5, 7, 11 and two query groups; the odd G cut the chain balance inside a row block);
* on a level of uniform white noise (distinct rows lie far apart) the database rows of one whole
  segment, taken as queries, put the segment's minimum at every row of the segment in turn: every
  (accumulator element, lane group, row block, tile, chain) position, the chains of the lagged
  tail included.  A position the fold dropped would return the second-best row, at least 4 eps_j
  away (asserted from numpy's fp64 values for every needle); the screen's minimum must lie within
  eps_j of the needle's own fp64 value.

The smallest level shape of test_gpu_compact_stream.py, the compact threshold lowered through
ia_diag_set_compact_min_rows as there.  On it every part is one stage and one segment, so a flush
writes a single segment per query: the compact form's 16-byte flush of full groups of 8 staged
segments is not run here; test_gpu_compact_stream.py's
test_compact_minima_do_not_depend_on_chunks_and_parts is the test that runs it (parts of 8 and
more segments, bit-equal minima)."""
import ctypes
import math

import numpy as np
import pytest

import ia_oracle as o
from test_gpu_compact import RK_C, RK_EPS_A2, U32, _bound_level
from test_gpu_compact_stream import SHAPES, _screen

pytestmark = pytest.mark.gpu

SHAPE = SHAPES[0]
WIDTHS = [32, 64, 160, 224, 342, 400]      # G = 1, 2, 5, 7, 11 and two query groups of 7 and 6
NEEDLE_SEED, NEEDLE_SEGMENT = 5, 17


def _screen_w(idx, N, Q):
    """64-slot minima of the rows of Q from the wave form k_screen16w (ia_diag_screen16r with the
    form switched for the call): (segmin with its NaN fill, nq, nsk)."""
    import _ia
    lib = _ia.lib()
    # launch_screen16r's condition for the wave form: whole blocks of spb segments
    seg = min(lib.ia_db_chunk_rows(N), 512)
    nseg, spb = lib.ia_db_rows_padded(N) // seg, 1
    while spb * (seg // 32) < 8:
        spb *= 2
    assert nseg % 16 == 0 and spb <= 16, 'the level takes the wave form (nseg a multiple of every spb)'
    prev = lib.ia_diag_set_r16_form(1)
    try:
        return _screen_r(idx, N, Q)
    finally:
        lib.ia_diag_set_r16_form(prev)


def _screen_r(idx, N, Q):
    """64-slot minima of the rows of Q (ia_diag_screen16r, the form in force)."""
    import torch
    import _ia
    from test_gpu_split16 import Q16_HALVES, dev
    lib = _ia.lib()
    M = len(Q)
    nseg = lib.ia_db_rows_padded(N) // min(lib.ia_db_chunk_rows(N), 512)
    qrows = lib.ia_diag_qp_rows(M)
    q64 = torch.zeros((M, _ia.IA_DP), dtype=torch.float64, device='cuda')
    q64[:, :55] = dev(Q)
    q16 = torch.zeros((qrows, Q16_HALVES), dtype=torch.float16, device='cuda')
    nq = torch.zeros(qrows, dtype=torch.float64, device='cuda')
    nsk = torch.zeros(qrows, dtype=torch.float64, device='cuda')
    segmin = torch.full((qrows, nseg), float('nan'), dtype=torch.float32, device='cuda')
    _ia.check(lib.ia_diag_screen16r(ctypes.byref(idx.src), idx.row0, N, _ia.ptr(idx.dbr), _ia.ptr(idx.rot),
                                    _ia.ptr(idx.amax), _ia.ptr(idx.center), _ia.ptr(q64), M, _ia.ptr(q16),
                                    _ia.ptr(nq), _ia.ptr(nsk), _ia.ptr(segmin), _ia.stream()), 'ia_diag_screen16r')
    torch.cuda.synchronize()
    return segmin.cpu().numpy(), nq.cpu().numpy()[:M], nsk.cpu().numpy()[:M]


@pytest.fixture(scope='module')
def level(gpu):
    """test_gpu_compact._bound_level's (64, 128) level with its compact DB, and its 48 queries."""
    import _ia
    lib = _ia.lib()
    prev = lib.ia_diag_set_compact_min_rows(-1)
    lib.ia_diag_set_compact_min_rows(1)
    try:
        idx, As, Q48 = _bound_level(31 + SHAPE[0], SHAPE, False, None)
    finally:
        lib.ia_diag_set_compact_min_rows(prev)
    yield idx, len(As), Q48


@pytest.mark.parametrize('form', ['compact', 'wave64'])
@pytest.mark.parametrize('M', WIDTHS)
def test_every_query_slot_sees_the_same_rows(level, M, form):
    """One query (a real wave query of the level) in all M slots: every query's row of minima is
    bit-equal to query 0's, and nothing is written past M."""
    idx, N, Q48 = level
    Q = np.repeat(Q48[20:21], M, axis=0)
    got = (_screen if form == 'compact' else _screen_w)(idx, N, Q)[0]
    assert np.isfinite(got[:M]).all() and np.isnan(got[M:]).all()
    bits = got[:M].view(np.int32)
    bad = np.nonzero((bits != bits[0]).any(axis=1))[0]
    assert len(bad) == 0, (form, M, bad[:16], np.nonzero(bits[bad[0]] != bits[0])[0][:16])


@pytest.fixture(scope='module')
def needles(gpu):
    """A (64, 128) level of uniform white noise (A, A' and the coarser level the oracle's pyramid
    makes of them), its compact DB, and as queries the database rows of segment NEEDLE_SEGMENT,
    composed from level_features_dev of A and of A' as bench.Job.lsh_quality composes a query.
    Returns what both forms' tests need; computed once, never modified."""
    import torch
    import _ia
    import algorithms
    from test_gpu_split16 import _segment_order, dev
    lib = _ia.lib()
    rs = np.random.RandomState(NEEDLE_SEED)
    A, Ap, B = rs.rand(*SHAPE), rs.rand(*SHAPE), rs.rand(9, 12)
    A_pyr, Ap_list, B_pyr, Bp_pyr, L = o.setup_luminance(A, [Ap], B, cap=2, seed=NEEDLE_SEED)
    Ad, Apd = [dev(p) for p in A_pyr], [dev(p) for p in Ap_list[0]]
    prev = lib.ia_diag_set_compact_min_rows(-1)
    lib.ia_diag_set_compact_min_rows(1)
    try:
        idx = algorithms.level_index(Ad, [Apd], L - 1, rot=True)
    finally:
        lib.ia_diag_set_compact_min_rows(prev)
    assert idx.dbr is not None and idx.dbk is not None
    As = o.create_index(A_pyr, Ap_list, L)[L - 1]
    N = len(As)
    npad = lib.ia_db_rows_padded(N)
    seg = min(lib.ia_db_chunk_rows(N), 512)
    nseg = npad // seg
    assert npad == N == SHAPE[0] * SHAPE[1]
    rows = _segment_order(idx, N, npad, seg).reshape(nseg, seg)[NEEDLE_SEGMENT]
    F = torch.cat([algorithms.level_features_dev(Ad[L - 2], Ad[L - 1], True),
                   algorithms.level_features_dev(Apd[L - 2], Apd[L - 1], False)], 1).cpu().numpy()
    assert F.shape == As.shape and np.abs(F - As).max() <= 1e-12
    Q = F[rows]                                   # needle i is the segment's row i
    amax, askip = (float(x) for x in idx.amax.cpu().numpy()[:2])
    c = idx.center.cpu().numpy()
    V = idx.rot.cpu().numpy()[:56 * 56].reshape(56, 56)[:55, :55].astype(np.float64)
    al = lambda n: (n + 255) // 256 * 256  # noqa: E731
    tail = idx.dbr.view(torch.uint8)[npad * lib.ia_db_rot_slots() * 2:]
    ask_dec = askip * float(tail[al(4 * nseg):][:nseg].cpu().numpy()[NEEDLE_SEGMENT]) / 255.0
    a = As[rows] - c                              # the segment's rows, centred
    return dict(idx=idx, N=N, Q=Q, a=a, kq=Q - c, V=V, amax=amax, ask_dec=ask_dec, seg=seg)


def _check_needles(nd, got, nqs, nsks, e, eps_a2, eps_q2, tag):
    """e[i][m]: fp64 value of segment row i for needle m; eps_j with the form's own terms in
    |a'|^2 and |q'|^2 (test_gpu_compact.py, test_gpu_rot16.py).  The input condition (gap >= 4
    eps_j) and the assertion |m_j - e(needle)| <= eps_j, for every needle."""
    from test_gpu_split16 import _scales
    seg, amax = nd['seg'], nd['amax']
    assert got.shape[0] >= seg and e.shape == (seg, seg)
    worst, tightest = 0.0, np.inf
    for m in range(seg):
        ea, R, eq = _scales(amax, float(nqs[m]))
        mj = float(np.ldexp(np.float64(got[m, NEEDLE_SEGMENT]), -(ea + eq)))
        eps = U32 * (360 * amax * math.sqrt(nqs[m]) + eps_a2 * amax * amax + eps_q2 * nqs[m]) + \
            2.0 ** -9 * 1.01 * nd['ask_dec'] * math.sqrt(nsks[m])
        col = np.sort(e[:, m])
        assert e[m, m] == col[0], (tag, m, 'the needle is its segment\'s best row')
        gap = col[1] - col[0]
        tightest = min(tightest, gap / eps)
        assert gap >= 4 * eps, (tag, m, gap, eps)
        worst = max(worst, abs(mj - e[m, m]) / eps)
        assert abs(mj - e[m, m]) <= eps, (tag, m, mj, e[m, m], eps)
    print('%s needles: least gap / eps_j = %.3g, worst |m_j - e(needle)| / eps_j = %.3g' % (tag, tightest, worst))


def test_every_row_position_is_folded_compact(needles):
    """The compact screen (k_screen16c<4>): e_C over the 24 kept components."""
    nd = needles
    got, nqs, nsks, _ = _screen(nd['idx'], nd['N'], nd['Q'])
    rho, kap = nd['a'] @ nd['V'], nd['kq'] @ nd['V']
    eC = (rho[:, :RK_C] ** 2).sum(1)[:, None] - 2.0 * (rho[:, :RK_C] @ kap[:, :RK_C].T)
    _check_needles(nd, got, nqs, nsks, eC, RK_EPS_A2, 32, 'compact')


def test_every_row_position_is_folded_wave64(needles):
    """The 64-slot wave form (k_screen16w<4>): e over all components."""
    import _ia
    nd = needles
    got, nqs, nsks = _screen_w(nd['idx'], nd['N'], nd['Q'])
    a = nd['a']
    e = np.einsum('ij,ij->i', a, a)[:, None] - 2.0 * (a @ nd['kq'].T)
    _check_needles(nd, got, nqs, nsks, e, _ia.lib().ia_db_rot_eps_a2(), 0, 'wave64')
