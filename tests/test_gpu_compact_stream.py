"""The compact screen's own stage geometry (csrc/ia_screen16r.hip k_screen16c: stage tiles, ring
depth and staged minima of its own; DESIGN.md §4d "compact").  Whatever the geometry, a (query,
segment) minimum is the minimum of the same single-MFMA values.  So

* the minima of a query do not depend on how many queries are screened with it (the kernel
  instance G, the query groups);
* the minima do not depend on the DB's chunking or on how the launcher cuts chunks into parts: a
  512-row segment's minimum is, bit for bit, the least of the minima of the four 128-row segments
  that hold its rows under the default chunking.  Chunk targets and query counts are chosen so
  that parts of 4 and more stages and of 1, of 2 to 7 and of 8 or more segments occur (asserted
  from the launcher's split arithmetic): later stages are issued into ring slots that were read
  before, the staged minima use several slots, and a part flushes short groups and full ones;
  512-row segments also take the 8-tile stages of a build that has them;
* they keep the bound of test_gpu_compact.py at the full width of 342 queries;
* nothing is written past the M rows asked for.

All through ia_diag_screen16k on test_gpu_compact._bound_level's levels and a third shape of the
same size class."""
import ctypes
import math

import numpy as np
import pytest

from test_gpu_compact import RK_C, RK_EPS_A2, R16_P, U32, _bound_level

SHAPES = [(64, 128), (40, 256)]
WIDTHS = [400, 342, 96, 16]        # two query groups (G = 7), G = 11, 3 and 1
MAX_G, OCC = 11, 4                 # ia_screen16r.hip: query tiles per group, blocks per CU
# the third shape, of the same size class, for the chunked test: at chunk targets 4 and 8 (4 is the
# least ia_set_chunk_target takes) its chunks hold 4 or more 512-row segments.  (chunk target, M):
# 33, 65 and 129 query groups of 11 tiles fill the grid, so the launcher stops splitting the chunks
# earlier and parts keep 2, 4, 8 or more segments
CHUNK_SHAPE = (128, 128)
CHUNKED = [(4, 342), (4, 64 * 352 + 32), (4, 128 * 352 + 32), (8, 342), (8, 32 * 352 + 32)]


def _screen(idx, N, Q):
    """Compact minima of the rows of Q: (segmin with its NaN fill, nq, nsk, |kappa_rest|^2)."""
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
    _ia.check(lib.ia_diag_screen16k(ctypes.byref(idx.src), idx.row0, N, _ia.ptr(idx.dbk), _ia.ptr(idx.rot),
                                    _ia.ptr(idx.amax), _ia.ptr(idx.center), _ia.ptr(q64), M, _ia.ptr(q16),
                                    _ia.ptr(nq), _ia.ptr(nsk), _ia.ptr(segmin), _ia.stream()), 'ia_diag_screen16k')
    torch.cuda.synchronize()
    return (segmin.cpu().numpy(), nq.cpu().numpy()[:M], nsk.cpu().numpy()[:M],
            q16[:M].view(torch.float64)[:, 24].cpu().numpy())      # byte 192 of each row


def _parts(N, M):
    """launch_screen16r's arithmetic for the chunking in force: (stages, segments) of a part."""
    import torch
    import _ia
    lib = _ia.lib()
    ch = lib.ia_db_chunk_rows(N)
    seg = min(ch, 512)
    nchunks, spc = lib.ia_db_rows_padded(N) // ch, ch // seg
    T = (M + 31) // 32
    groups = (T + MAX_G - 1) // MAX_G
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    split = 1
    while 2 * split <= spc and nchunks * 2 * split * groups <= cus * OCC:
        split *= 2
    return ch // split // 128, spc // split


@pytest.fixture(scope='module')
def levels(gpu):
    """Per shape: the level (compact DB built, threshold 1), the oracle's rows, its 48 queries and
    the minima of their tiling to 400 for every M of WIDTHS, default chunking; freed with the
    module."""
    import _ia
    lib = _ia.lib()
    prev = lib.ia_diag_set_compact_min_rows(-1)
    lib.ia_diag_set_compact_min_rows(1)
    out = {}
    try:
        for shape in SHAPES:
            idx, As, Q48 = _bound_level(31 + shape[0], shape, False, None)
            Q = np.tile(Q48, (9, 1))[:max(WIDTHS)]
            out[shape] = (idx, As, Q48, {M: _screen(idx, len(As), Q[:M]) for M in WIDTHS})
    finally:
        lib.ia_diag_set_compact_min_rows(prev)
    yield out
    out.clear()


@pytest.mark.gpu
@pytest.mark.parametrize('shape', SHAPES)
def test_compact_minima_do_not_depend_on_the_query_width(levels, shape):
    """The minima rows of the queries common to M = 400 (two query groups), 342 (G = 11), 96
    (G = 3) and 16 (G = 1) are equal bit for bit, and so are the rows of equal queries (the 48
    tiled): every kernel instance and query group computes and addresses the same minima.  (Default
    chunking: one-stage parts; the parts of many stages are the next test's.)"""
    runs = levels[shape][3]
    full = runs[400][0][:400].view(np.int32)
    for M in WIDTHS[1:]:
        assert np.array_equal(runs[M][0][:M].view(np.int32), full[:M]), M
    for m in range(48, 400):
        assert np.array_equal(full[m], full[m % 48]), m


@pytest.mark.gpu
def test_compact_minima_do_not_depend_on_chunks_and_parts(gpu):
    """A (128, 128) level built under the default chunking and under chunk targets 4 and 8, and
    screened with 342, 11,296, 22,560 and 45,088 queries (1, 33, 65 and 129 query groups): every
    512-row segment's minimum equals, bit for bit, the least of the default chunking's 128-row
    segment minima over the same rows.  The parts these launches cut (asserted) have 4 and more
    stages, so stages land in ring slots already read, and 1 segment, 2 to 7 and 8 or more, so the
    staged minima take several slots and leave in short groups as well as full ones.  A stage read
    before it landed, a slot refilled early, a wrong staging slot or a mis-addressed flush run
    would change some minimum."""
    import _ia
    from test_gpu_split16 import _segment_order
    lib = _ia.lib()
    shape = CHUNK_SHAPE
    seen = set()
    prev_rows = lib.ia_diag_set_compact_min_rows(-1)
    lib.ia_diag_set_compact_min_rows(1)
    try:
        idx0, As, Q48 = _bound_level(31 + shape[0], shape, False, None)
        N = len(As)
        assert lib.ia_db_chunk_rows(N) == 128 and lib.ia_db_rows_padded(N) == N
        ref = _screen(idx0, N, Q48)[0][:48]                     # [48][N / 128], default chunking
        assert np.isfinite(ref).all()
    finally:
        lib.ia_diag_set_compact_min_rows(prev_rows)
    seg0 = np.empty(N, dtype=np.int64)                          # row -> its default segment
    seg0[_segment_order(idx0, N, N, 128)] = np.arange(N) // 128
    lib.ia_diag_set_compact_min_rows(1)
    try:
        for target in sorted({t for t, _ in CHUNKED}):
            prev = lib.ia_set_chunk_target(target)
            try:
                assert lib.ia_set_chunk_target(target) == target, 'the target was taken'
                idx, As_t, Q_t = _bound_level(31 + shape[0], shape, False, None)
                assert np.array_equal(As_t, As) and np.array_equal(Q_t, Q48)
                ch, npad = lib.ia_db_chunk_rows(N), lib.ia_db_rows_padded(N)
                assert ch >= 2048 and min(ch, 512) == 512, 'chunks of several 512-row segments'
                order = _segment_order(idx, N, npad, 512).reshape(-1, 512)
                real = [s for s in range(len(order)) if order[s].max() < N]
                assert len(real) == N // 512
                want = np.empty((48, len(real)), dtype=np.float32)
                for i, s in enumerate(real):
                    parts0 = np.unique(seg0[order[s]])
                    assert len(parts0) == 4, 'a 512-row segment is four default segments'
                    want[:, i] = ref[:, parts0].min(axis=1)
                for M in [m for t, m in CHUNKED if t == target]:
                    seen.add(_parts(N, M))
                    got = _screen(idx, N, np.tile(Q48, ((M + 47) // 48, 1))[:M])[0]
                    assert np.isfinite(got[:M]).all() and np.isnan(got[M:]).all(), (target, M)
                    got = got[:M][:, real].view(np.int32)
                    assert np.array_equal(got[:48], want.view(np.int32)), (target, M)
                    for g in range(48, M, 48):                  # every tiling of the 48
                        n = min(48, M - g)
                        assert np.array_equal(got[g:g + n], got[:n]), (target, M, g)
            finally:
                lib.ia_set_chunk_target(prev)
    finally:
        lib.ia_diag_set_compact_min_rows(prev_rows)
    print('compact parts (stages, segments):', sorted(seen))
    stages, segs = {p[0] for p in seen}, {p[1] for p in seen}
    assert any(2 <= s < 8 for s in segs), 'a short flush group'
    assert any(s >= 8 for s in segs), 'a full flush group'
    assert 1 in segs and any(s >= 4 for s in stages), 'one-segment parts of several stages'
    assert len(stages) >= 3


@pytest.mark.gpu
@pytest.mark.parametrize('shape', SHAPES)
def test_compact_minima_leave_the_padding_alone(levels, shape):
    """Rows of segmin beyond M keep their NaN fill, and every row below M is finite."""
    for M, (segmin, _, _, _) in levels[shape][3].items():
        assert np.isfinite(segmin[:M]).all(), M
        assert np.isnan(segmin[M:]).all(), M


@pytest.mark.gpu
def test_compact_minima_are_lower_bounds_at_full_width(levels):
    """test_gpu_compact.py's two assertions at M = 342 (G = 11, the plateau instance) on the
    (64, 128) level: |m_j - min e_C| <= eps_j and L_j <= min e against numpy fp64, for every
    (query, segment)."""
    import torch
    import _ia
    from test_gpu_split16 import _scales, _segment_order
    shape, M = SHAPES[0], 342
    idx, As, Q48, runs = levels[shape]
    got, nqs, nsks, nrest = runs[M]
    got = got[:M].astype(np.float64)
    lib = _ia.lib()
    N = len(As)
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
    al = lambda n: (n + 255) // 256 * 256  # noqa: E731
    tail = idx.dbr.view(torch.uint8)[npad * lib.ia_db_rot_slots() * 2:]
    ask_dec = askip * tail[al(4 * nseg):][:nseg].cpu().numpy().astype(np.float64) / 255.0
    tk = idx.dbk.view(torch.uint8)[npad * 64:]
    codes = tk[al(4 * nseg):][:nseg].cpu().numpy().astype(np.float64)
    rmax = float(tk[al(4 * nseg) + al(nseg):][:4].view(torch.float32).cpu().numpy()[0])
    R_dec = rmax * codes / 255.0
    # numpy's fp64 segment minima of the 48 distinct queries: e over all components, e_C over the kept
    kap = (Q48 - c) @ V
    E = np.einsum('ij,ij->i', a, a)[:, None] - 2.0 * (a @ (Q48 - c).T)
    EC = (rho[:, :RK_C] ** 2).sum(1)[:, None] - 2.0 * (rho[:, :RK_C] @ kap[:, :RK_C].T)
    exact = E[order].reshape(nseg, seg, 48).min(axis=1).T
    exactC = EC[order].reshape(nseg, seg, 48).min(axis=1).T
    worst, worst_lb = 0.0, -np.inf
    for m in range(M):
        q = m % 48
        assert nrest[m] == pytest.approx(float((kap[q, RK_C:] ** 2).sum()), rel=1e-9, abs=1e-300)
        assert nsks[m] == pytest.approx(float((kap[q, R16_P:] ** 2).sum()), rel=1e-9, abs=1e-300)
        ea, R, eq = _scales(amax, float(nqs[m]))
        mj = np.ldexp(got[m], -(ea + eq))
        eps = U32 * (360 * amax * math.sqrt(nqs[m]) + RK_EPS_A2 * amax * amax + 32 * nqs[m]) + \
            2.0 ** -9 * 1.01 * ask_dec * math.sqrt(nsks[m])
        worst = max(worst, (np.abs(mj - exactC[q]) / eps).max())
        k = math.sqrt(nrest[m])
        L = mj - eps - k * k + np.maximum(0.0, k - R_dec) ** 2
        # (numpy's own rounding of e: a few ulps of |a'|^2 + 2 |a'||q'|)
        worst_lb = max(worst_lb, (L - exact[q] - 1e-13 * (amax * amax + nqs[m])).max())
    print('compact screen %s at M = %d: worst |m_j - min e_C| / eps_j = %.3g; max (L_j - min e) = %.3g'
          % (shape, M, worst, worst_lb))
    assert worst < 1.0
    assert worst_lb <= 0.0
