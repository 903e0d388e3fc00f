"""Training pairs (A_i, A'_i) on the device against the pair oracle (tests/pairs_oracle.py):
row (i, r, c) of a level's database is [full(A_i) | half(A'_i)].  Every comparison is
np.array_equal on B', s and im of every level; the LSH cases compare as tests/test_gpu_lsh.py
and tests/test_gpu_lsh3.py do for one A."""
import ctypes
import functools
import os
import types

import numpy as np
import pytest
import torch

import ia_oracle as o
import ia_oracle_c as oc
import lsh3_ref as r3
import pairs_oracle as po

pytestmark = pytest.mark.gpu

LUM = {2: (2, (40, 52), (37, 41)), 3: (3, (33, 47), (24, 50))}
COL = {2: (2, (40, 52), (37, 41)), 3: (3, (33, 47), (24, 50))}


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to('cuda', dtype=torch.float64)


def dev_job(pyr):
    """Device copies of po.pyramids(...): (A pyramids, A' pyramids, B pyramid, B' pyramid)."""
    A_pyrs, Ap_list, B_pyr, Bp_pyr, _ = pyr
    up = lambda q: [dev(p) for p in q]  # noqa: E731
    return [up(q) for q in A_pyrs], [up(q) for q in Ap_list], up(B_pyr), up(Bp_pyr)


def assert_ref(out, Bp_dev, ref):
    assert set(out) == set(ref) and len(ref) >= 2
    for l in ref:
        assert np.array_equal(out[l][0].cpu().numpy(), ref[l][1]), ('s', l)
        assert np.array_equal(out[l][1].cpu().numpy(), ref[l][2]), ('im', l)
        assert np.array_equal(Bp_dev[l].cpu().numpy(), ref[l][0]), ("B'", l)


def run(pyr, channels=1, k=po.KAPPA, **kw):
    import image_analogies as ia
    A_d, Ap_d, B_d, Bp_d = dev_job(pyr)
    out = ia.synthesize_dev(A_d, Ap_d, B_d, Bp_d, pyr[4], k, po.weights(channels), **kw)
    torch.cuda.synchronize()
    return out, Bp_d


# ---- 1. row form, luminance --------------------------------------------------------------------

@pytest.mark.parametrize('rot', [False, True], ids=['split16', 'r16'])
@pytest.mark.parametrize('pipeline', [True, False], ids=['pipelined', 'level'])
@pytest.mark.parametrize('n', [2, 3])
def test_luminance_pairs_vs_oracle(gpu, monkeypatch, n, pipeline, rot):
    """2 pairs A 40x52 / B 37x41 and 3 pairs A 33x47 / B 24x50 (a 17x24 coarse level: its stride
    is not hw / 4; three pairs: an image index clamped to 1 shows), pipelined and one level at a
    time, with the R16 screen on the row form (IA_ROT_MIN_ROWS=1) and without."""
    if rot:
        monkeypatch.setenv('IA_ROT_MIN_ROWS', '1')
    ref = po.reference(*LUM[n])
    out, Bp_d = run(po.pyramids(*LUM[n]), pipeline=pipeline)
    assert_ref(out, Bp_d, ref)


@functools.lru_cache(maxsize=None)
def debug_reference():
    """o.synthesize_level(debug=...) over the stacked rows of the 2-pair case."""
    A_pyrs, Ap_list, B_pyr, Bp_pyr, L = po.pyramids(*LUM[2])
    Bp = [b.copy() for b in Bp_pyr]
    out = {}
    for l in range(1, L):
        dbg = {}
        s, im = o.synthesize_level(l, L, A_pyrs[0], Ap_list, B_pyr, Bp, po.stacked_rows(l, A_pyrs, Ap_list),
                                   po.weights(), po.KAPPA, debug=dbg)
        out[l] = (s, im, dbg)
    return out


def test_luminance_pairs_debug_record(gpu):
    import image_analogies as ia
    ref, dref = po.reference(*LUM[2]), debug_reference()
    out, Bp_d = run(po.pyramids(*LUM[2]), debug=True)
    assert_ref(out, Bp_d, ref)
    for l in ref:
        s, im, dbg = out[l]
        rec = ia.debug_record(s, im, dbg, ref[l][0].shape[:2])
        assert np.array_equal(dref[l][0], ref[l][1]) and np.array_equal(dref[l][1], ref[l][2])
        for key in ('sa', 'sc', 'rstars'):
            assert rec[key] == dref[l][2][key], (l, key)
        assert np.array_equal(rec['app_dist'], dref[l][2]['app_dist']), l
        assert np.array_equal(rec['coh_dist'], dref[l][2]['coh_dist']), l


# ---- 2. builders ---------------------------------------------------------------------------------

def queries(rows, n, seed=3, M=64):
    """M queries: stacked rows of n images plus 1e-3 noise, half of them rows of images >= 1."""
    rs = np.random.RandomState(seed)
    per = rows.shape[0] // n
    ix = np.concatenate([rs.randint(0, per, M // 2), rs.randint(per, rows.shape[0], M - M // 2)])
    return rows[ix] + rs.randn(M, rows.shape[1]) * 1e-3


@pytest.mark.parametrize('n', [2, 3])
def test_level_index_rows_and_match(gpu, n):
    import algorithms
    pyr = po.pyramids(*LUM[n])
    A_d, Ap_d, _, _ = dev_job(pyr)
    for l in range(1, pyr[4]):
        rows = po.stacked_rows(l, pyr[0], pyr[1])
        index = algorithms.level_index(A_d, Ap_d, l)
        assert index.nA == n and index.src.nA == n and index.dbi is None and index.db is not None
        assert np.array_equal(index.features().cpu().numpy(), rows), l
        Q = queries(rows, n)
        gi, gd = index.match(Q)
        ri, rd = oc.nn_batch(oc._d(rows), rows.shape[0], Q)
        assert np.array_equal(gi.cpu().numpy(), ri) and np.array_equal(gd.cpu().numpy(), rd), l
        assert (ri >= rows.shape[0] // n).sum() >= 16


def scan(rows, Q):
    """LevelDB.scan's brute force over a rows buffer."""
    Q = np.ascontiguousarray(Q, dtype=np.float64)
    idx, d = np.empty(len(Q), np.int64), np.empty(len(Q), np.float64)
    oc.lib().ia_oracle_nn_n_batch(oc._d(rows), rows.shape[0], rows.shape[1], oc._d(Q), len(Q),
                                  idx.ctypes.data_as(ctypes.POINTER(ctypes.c_long)), oc._d(d))
    return idx, d


@pytest.mark.parametrize('n', [2, 3])
def test_level_index3_rows_and_match(gpu, n):
    import algorithms
    pyr = po.pyramids(*COL[n], channels=3)
    A_d, Ap_d, _, _ = dev_job(pyr)
    l = pyr[4] - 1
    rows = po.stacked_rows(l, pyr[0], pyr[1])
    A_sm, A_lg, nA = algorithms.a_level(A_d, n, l)
    index = algorithms.LevelIndex3(A_sm, A_lg, torch.stack([p[l - 1] for p in Ap_d]),
                                   torch.stack([p[l] for p in Ap_d]), nA=nA)
    assert nA == n and index.src.nA == n and rows.shape[1] == 165
    assert np.array_equal(index.features().cpu().numpy(), rows)
    Q = queries(rows, n)
    gi, gd = index.match(Q)
    ri, rd = scan(rows, Q)
    assert np.array_equal(gi.cpu().numpy(), ri) and np.array_equal(gd.cpu().numpy(), rd)


# ---- 3. the bound covers every A -----------------------------------------------------------------

@pytest.mark.parametrize('rows_form', [False, True], ids=['default', 'rows'])
@pytest.mark.parametrize('rot', [False, True], ids=['split16', 'r16'])
def test_bound_covers_every_A(gpu, monkeypatch, rot, rows_form):
    """Pair 0 (A_0 and A'_0) times 1/64, pair 1 as it is: a bound from image 0 alone would be 64
    times too small and the screen no longer exact.  amax[0] >= the fp64 maximum over all
    stacked rows of |row - centre|, and the synthesis equals the oracle."""
    import algorithms
    import image_analogies as ia
    if rot:
        monkeypatch.setenv('IA_ROT_MIN_ROWS', '1')
    pyr = po.pyramids(*LUM[2], scale0=1.0 / 64)
    A_pyrs, Ap_list, B_pyr, Bp_pyr, L = pyr
    ref = po.synthesize(A_pyrs, Ap_list, B_pyr, Bp_pyr, L, po.KAPPA, po.weights())
    A_d, Ap_d, B_d, Bp_d = dev_job(pyr)
    w = dev(po.weights())
    out = {}
    for l in range(1, L):
        index = algorithms.level_index(A_d, Ap_d, l, rows=rows_form or None)
        rows = po.stacked_rows(l, A_pyrs, Ap_list)
        need = np.sqrt(((rows - index.center.cpu().numpy()[None, :]) ** 2).sum(1)).max()
        one = np.sqrt(((rows[:rows.shape[0] // 2] - index.center.cpu().numpy()[None, :]) ** 2).sum(1)).max()
        amax = float(index.amax[0].item())
        print('level %d: amax %.6g, max |row - centre| %.6g (image 0 alone: %.6g)' % (l, amax, need, one))
        assert amax >= need
        assert (index.dbr is not None) == rot
        out[l] = ia.synthesize_level_dev(l, L, index, B_d[l - 1], B_d[l], Bp_d[l - 1], Bp_d[l], w, po.KAPPA)
    torch.cuda.synchronize()
    assert_ref(out, Bp_d, ref)


# ---- 4. form fallback ----------------------------------------------------------------------------

def finest_plan(A_d, Ap_d, B_d, Bp_d, L):
    import _ia
    import algorithms
    import image_analogies as ia
    l = L - 1
    index = algorithms.level_index(A_d, Ap_d, l)
    call = ia._LevelCall(l, L, index, B_d[l - 1], B_d[l], Bp_d[l - 1], Bp_d[l], dev(po.weights()), po.KAPPA)
    return index, _ia.level_plan(call.args)


def test_pairs_take_the_row_form_at_128_wide(gpu):
    """2 pairs A 128x128 / B 37x41: no image form, the fused kernel's row form (no compact waves,
    no split candidates), by itself; the same shapes with one A and 2 A' keep the strip form."""
    import _ia
    pyr = po.pyramids(2, (128, 128), (37, 41))
    A_d, Ap_d, B_d, Bp_d = dev_job(pyr)
    index, plan = finest_plan(A_d, Ap_d, B_d, Bp_d, pyr[4])
    assert index.dbi is None and index.db is not None
    assert plan['xw'] and plan['form'] == _ia.XW_ROWS and not plan['rk'] and not plan['split']
    one, plan1 = finest_plan(A_d[0], Ap_d, B_d, Bp_d, pyr[4])
    assert one.dbi is not None and plan1['form'] == _ia.XW_STRIP
    ref = po.reference(2, (128, 128), (37, 41))
    out, Bp_o = run(pyr)
    assert_ref(out, Bp_o, ref)


# ---- 5. shards -----------------------------------------------------------------------------------

@pytest.mark.parametrize('G', [2, 3])
def test_pairs_in_process_shards(gpu, G):
    """ia_diag_synth_level_shards over G contiguous row ranges of n h w (G = 3: the middle
    shard straddles the two images)."""
    import _ia
    import algorithms
    import image_analogies as ia
    pyr, ref = po.pyramids(*LUM[2]), po.reference(*LUM[2])
    A_d, Ap_d, B_d, Bp_d = dev_job(pyr)
    L, w = pyr[4], dev(po.weights())
    out = {}
    for l in range(1, L):
        full = algorithms.level_index(A_d, Ap_d, l)
        shards = [algorithms.level_index(A_d, Ap_d, l, lambda lv, N, g=g: ia.shard_rows(N, g, G)) for g in range(G)]
        if G == 3:
            hw = full.N // 2
            assert shards[1].row0 < hw < shards[1].row0 + shards[1].nrows
        call = ia._LevelCall(l, L, full, B_d[l - 1], B_d[l], Bp_d[l - 1], Bp_d[l], w, po.KAPPA)
        arr = (_ia.IaShardDb * G)(*[_ia.IaShardDb(_ia.ptr(x.db).value, x.row0, x.nrows, _ia.ptr(x.amax).value,
                                                  x.dbi_ptr()) for x in shards])
        _ia.check(_ia.lib().ia_diag_synth_level_shards(ctypes.byref(call.args), arr, G, _ia.stream()),
                  'ia_diag_synth_level_shards')
        out[l] = call.result()
    torch.cuda.synchronize()
    assert_ref(out, Bp_d, ref)


def with_exchanges(kind, L, fn):
    import _ia
    comms = [_ia.exchange(0, 1, kind) for _ in range(1, L)]
    try:
        res = fn(comms)
        torch.cuda.synchronize()
        for cm in comms:
            _ia.exchange_status(cm)
        return res
    finally:
        torch.cuda.synchronize()
        for cm in comms:
            _ia.check(_ia.lib().ia_comm_destroy(cm), 'ia_comm_destroy')


@pytest.mark.parametrize('kind,xwave', [('peer', None), ('rccl', None), ('peer', 0)],
                         ids=['peer', 'rccl', 'peer-unfused'])
def test_pairs_over_a_one_rank_exchange(gpu, kind, xwave):
    """Every level sharded over a 1-rank exchange: the fused peer tail, the RCCL gather, and
    the unfused peer tail (ia_diag_set_xwave(0), restored)."""
    import _ia
    pyr, ref = po.pyramids(*LUM[2]), po.reference(*LUM[2])
    prev = _ia.xwave(xwave) if xwave is not None else None
    try:
        out, Bp_d = with_exchanges(kind, pyr[4], lambda comms: run(pyr, comm=comms, rank=0, nranks=1))
    finally:
        if prev is not None:
            _ia.xwave(prev)
    assert_ref(out, Bp_d, ref)


# ---- 6. colour -----------------------------------------------------------------------------------

@pytest.mark.parametrize('variant', ['default', 'rot0', 'color16-0', 'peer'])
@pytest.mark.parametrize('n', [2, 3])
def test_colour_pairs_vs_oracle(gpu, monkeypatch, n, variant):
    """2 pairs 40x52x3 / 37x41x3 and 3 pairs 33x47x3 / 24x50x3: the default (R16c, fused), the
    split-f16 screen (IA_DB_ROT=0), the exhaustive search (ia_diag_set_color16(0)) and a 1-rank
    peer exchange (k_peer_finish3 gathers the coherence rows from the pyramids: acc8_feat)."""
    import _ia
    pyr, ref = po.pyramids(*COL[n], channels=3), po.reference(*COL[n], channels=3)
    if variant == 'rot0':
        monkeypatch.setenv('IA_DB_ROT', '0')
    prev = _ia.lib().ia_diag_set_color16(0) if variant == 'color16-0' else None
    try:
        if variant == 'peer':
            out, Bp_d = with_exchanges('peer', pyr[4],
                                       lambda comms: run(pyr, 3, comm=comms, rank=0, nranks=1))
        else:
            out, Bp_d = run(pyr, 3)
    finally:
        if prev is not None:
            _ia.lib().ia_diag_set_color16(prev)
    assert_ref(out, Bp_d, ref)


# ---- 7. LSH --------------------------------------------------------------------------------------

LSH = dict(tables=8, hashes=3, width=1.0, seed=7)


def test_lsh_luminance_pairs(gpu):
    """As tests/test_gpu_lsh.py for one A: each level against o.synthesize_level driven by
    o.LshIndex over the stacked rows with the index's own centre, width and projections."""
    import algorithms
    import image_analogies as ia
    pyr = po.pyramids(*LUM[2])
    A_pyrs, Ap_list, B_pyr, Bp_pyr, L = pyr
    A_d, Ap_d, B_d, Bp_d = dev_job(pyr)
    Bp_ref = [b.copy() for b in Bp_pyr]
    w = po.weights()
    for l in range(1, L):
        rows = po.stacked_rows(l, A_pyrs, Ap_list)
        index = algorithms.level_index(A_d, Ap_d, l, lsh=LSH)
        # the centre and the width take their statistics over all A images
        A_lg = np.stack([p[l] for p in A_pyrs])
        Ap_lg = np.stack([p[l] for p in Ap_list])
        assert np.allclose(index.center.cpu().numpy()[[0, 54]], [A_lg.mean(), Ap_lg.mean()], rtol=1e-12)
        var = (34 * A_lg.var(ddof=1) + 21 * Ap_lg.var(ddof=1)) / 55.0
        assert np.isclose(index.lsh.w, np.sqrt(var), rtol=1e-6)
        s, im = ia.synthesize_level_dev(l, L, index, B_d[l - 1], B_d[l], Bp_d[l - 1], Bp_d[l], dev(w), po.KAPPA)
        h = index.lsh
        lsh = o.LshIndex(rows, index.center.cpu().numpy(), index.lsh_proj_host, h.L, h.k, np.float32(h.w))
        rs_, rim = o.synthesize_level(l, L, A_pyrs[0], Ap_list, B_pyr, Bp_ref, rows, w, po.KAPPA,
                                      matcher=lambda q: lsh.match(q)[0][0])
        assert np.array_equal(s.cpu().numpy(), rs_), l
        assert np.array_equal(im.cpu().numpy(), rim), l
        assert np.array_equal(Bp_d[l].cpu().numpy(), Bp_ref[l]), l
        assert set(rim.tolist()) == {0, 1}


def lsh3_tables_of(pyr, A_d, Ap_d):
    """level -> the restatement (lsh3_ref.LshIndexD) over the stacked rows with the device
    index's own centre, width and projections."""
    import algorithms

    def tables(l):
        A_sm, A_lg, nA = algorithms.a_level(A_d, len(Ap_d), l)
        index = algorithms.LevelIndex3(A_sm, A_lg, torch.stack([p[l - 1] for p in Ap_d]),
                                       torch.stack([p[l] for p in Ap_d]), nA=nA).build_lsh(**LSH)
        h = index.lsh
        return r3.LshIndexD(po.stacked_rows(l, pyr[0], pyr[1]), index.center.cpu().numpy(),
                            index.lsh_proj_host, h.L, h.k, np.float32(h.w))
    return tables


def test_lsh_colour_pairs(gpu):
    """As tests/test_gpu_lsh3.py for one A: synthesize_dev(lsh=...) against the scanline oracle
    driven by the restatement over the stacked rows."""
    pyr = po.pyramids(*COL[2], channels=3)
    A_pyrs, Ap_list, B_pyr, Bp_pyr, L = pyr
    A_d, Ap_d, _, _ = dev_job(pyr)
    tables = lsh3_tables_of(pyr, A_d, Ap_d)
    Bp_ref = [b.copy() for b in Bp_pyr]
    ref = {}
    for l in range(1, L):
        tab = tables(l)
        s, im = o.synthesize_level(l, L, A_pyrs[0], Ap_list, B_pyr, Bp_ref, tab.As, po.weights(3), po.KAPPA,
                                   matcher=tab.pick)
        ref[l] = (Bp_ref[l].copy(), s, im)
    out, Bp_d = run(pyr, 3, lsh=LSH)
    assert_ref(out, Bp_d, ref)


# ---- 8. batches ----------------------------------------------------------------------------------

@pytest.mark.parametrize('lsh', [None, LSH], ids=['exact', 'lsh'])
@pytest.mark.parametrize('channels', [1, 3], ids=['luminance', 'colour'])
def test_pair_batches_equal_single_runs(gpu, monkeypatch, channels, lsh):
    """Four jobs in two DB groups (two pair sets, each with two B images and two kappas):
    synthesize_batch_dev equals the four synthesize_dev runs bit for bit."""
    import image_analogies as ia
    monkeypatch.setenv('IA_ROT_MIN_ROWS', '1')      # (luminance batches of this size: the R16 screen too)
    shapes = ((30, 40), (28, 33)) if channels == 3 else ((40, 52), (37, 41))
    w = po.weights(channels)
    ks = [0.5, 1.0, 0.5, 1.0]
    sets = []
    for seed in (po.SEED, po.SEED + 100):
        base = po.pyramids(2, shapes[0], shapes[1], seed, channels)
        other = po.pyramids(2, shapes[0], shapes[1], seed, channels, b_seed=seed + 5)
        A_d, Ap_d, _, _ = dev_job(base)
        sets.append((A_d, Ap_d, base, other))

    def jobs():
        out = []
        for A_d, Ap_d, base, other in sets:
            for pyr in (base, other):
                out.append((A_d, Ap_d, [dev(p) for p in pyr[2]], [dev(p) for p in pyr[3]]))
        return out
    L = sets[0][2][4]
    extra = {} if lsh is None else {'lsh': lsh}
    batch = jobs()
    assert ia.db_groups(batch) == [0, 0, 1, 1]
    got = ia.synthesize_batch_dev(batch, L, ks, w, **extra)
    torch.cuda.synchronize()
    single = jobs()
    for q, (job, k) in enumerate(zip(single, ks)):
        ref = ia.synthesize_dev(*job, L, k, w, **extra)
        torch.cuda.synchronize()
        for l in ref:
            assert torch.equal(got[q][l][0], ref[l][0]) and torch.equal(got[q][l][1], ref[l][1]), (q, l)
            assert torch.equal(batch[q][3][l], job[3][l]), (q, l)
    if lsh is None:     # the exact runs are the pair oracle's
        for q, (A_d, Ap_d, base, other) in enumerate(sets):
            ref = po.synthesize(base[0], base[1], base[2], base[3], L, ks[2 * q], w)
            assert_ref(got[2 * q], batch[2 * q][3], ref)


# ---- 9. end to end -------------------------------------------------------------------------------

def config(**kw):
    c = types.SimpleNamespace(convert=False, remap_lum=False, init_rand=True, AB_weight=1, k=po.KAPPA, n_sm=3,
                              levels=2, seed=po.SEED, matcher='brute')
    c.__dict__.update(kw)
    return c


def pair_files(tmp_path, rgb):
    from test_gpu_outputs import _write_png
    As, Aps, B = po.pair_images(2, (40, 52), (37, 41))
    lift = (lambda x: np.dstack([x, 0.3 + 0.5 * x * x, 1 - x])) if rgb else (lambda x: x)
    files = {}
    for name, img in (('A0', As[0]), ('A1', As[1] * 0.8), ('Ap0', Aps[0]), ('Ap1', Aps[1]), ('B', B)):
        files[name] = str(tmp_path / (name + '.png'))
        _write_png(files[name], lift(img), 'RGB' if rgb else 'L')
    return files


def reference_pairs_setup(files, c):
    """The oracle's setup per pair from the decoded files (as tests/test_gpu_setup.py's
    reference_setup for one A): the 0-1 scale per A image, the A' scale from the first row of the
    last A', remap_lum per pair with A_i's own statistics, AB_weight on every A_i."""
    import matplotlib.pyplot as plt
    dec = {n: plt.imread(p).astype(np.float64) for n, p in files.items()}
    dec = {n: x[..., :3] if x.ndim == 3 else x for n, x in dec.items()}
    sc = lambda x: 255. if np.max(x) > 1.0 else 1.0  # noqa: E731
    lum = (lambda x: o.convert_to_YIQ(x)[..., 0]) if c.convert else (lambda x: x)
    sAp = sc(dec['Ap1'][0])
    B = dec['B'] / sc(dec['B'])
    per = [o.setup_luminance(lum(dec['A%d' % i] / sc(dec['A%d' % i])), [lum(dec['Ap%d' % i] / sAp)], lum(B),
                             c.AB_weight, c.remap_lum, cap=c.levels, init_rand=c.init_rand, seed=c.seed)
           for i in range(2)]
    return [p[0] for p in per], [p[1][0] for p in per], per[0][2], per[0][3], per[0][4]


@pytest.mark.parametrize('convert,remap', [(False, False), (True, False), (True, True)],
                         ids=['plain', 'convert', 'convert-remap'])
def test_main_with_pairs(gpu, tmp_path, convert, remap):
    import image_analogies as ia
    files = pair_files(tmp_path, convert)
    c = config(convert=convert, remap_lum=remap, AB_weight=0.5 if remap else 1)
    A_names, Ap_names = [files['A0'], files['A1']], [files['Ap0'], files['Ap1']]
    A_pyrs, Ap_list, B_pyr, Bp_pyr, L = reference_pairs_setup(files, c)
    got = ia.setup_dev(ia._read_A(A_names, 2), [ia._read(f) for f in Ap_names], ia._read(files['B']), config(**vars(c)))
    assert isinstance(got[0][0], list) and len(got[0]) == 2
    for mine, theirs in zip(got[0] + got[1] + [got[2], got[3]], A_pyrs + Ap_list + [B_pyr, Bp_pyr]):
        assert len(mine) == len(theirs) == L
        for x, y in zip(mine, theirs):
            assert np.array_equal(x.cpu().numpy(), y)
    ref = po.synthesize(A_pyrs, Ap_list, B_pyr, Bp_pyr, L, c.k, po.weights())
    out = {}
    Bp = ia.image_analogies_main(A_names, Ap_names, files['B'], str(tmp_path / 'out') + '/', c, outputs=out)
    assert c.max_levels == L and sorted(out) == sorted(ref)
    for l in ref:
        assert np.array_equal(out[l]['s'], ref[l][1]) and np.array_equal(out[l]['im'], ref[l][2]), l
        assert np.array_equal(Bp[l], ref[l][0]), l
    assert set(ref[L - 1][2].tolist()) == {0, 1}
    # a 1-element list is the single A
    one = {}
    ia.image_analogies_main([files['A0']], Ap_names, files['B'], str(tmp_path / 'one') + '/', config(**vars(c)),
                            outputs=one)
    same = {}
    ia.image_analogies_main(files['A0'], Ap_names, files['B'], str(tmp_path / 'same') + '/', config(**vars(c)),
                            outputs=same)
    assert all(np.array_equal(one[l]['s'], same[l]['s']) and np.array_equal(one[l]['im'], same[l]['im']) for l in same)
    assert any(not np.array_equal(one[l]['s'], out[l]['s']) for l in out)


def test_multi_main_batches_pair_runs(gpu, tmp_path):
    """multi_main(batch=2) of two pair runs (two kappas) writes the bytes of the unbatched loop."""
    import image_analogies as ia
    files = pair_files(tmp_path, True)
    A_names, Ap_names = [files['A0'], files['A1']], [files['Ap0'], files['Ap1']]

    def runs(tag):
        # (a run's <name>.jpg is named after its directory: the same leaf names under both)
        return [(A_names, Ap_names, files['B'], str(tmp_path / tag / ('run%d' % j)) + '/', {'k': k})
                for j, k in enumerate((0.5, 2.0))]
    ia.multi_main(runs('loop'), config(convert=True), rank=0, world=1)
    ia.multi_main(runs('batch'), config(convert=True), rank=0, world=1, batch=2)
    n = 0
    for j in range(2):
        a, b = str(tmp_path / 'loop' / ('run%d' % j)), str(tmp_path / 'batch' / ('run%d' % j))
        assert sorted(os.listdir(a)) == sorted(os.listdir(b))
        for f in os.listdir(a):
            if f.endswith('.jpg'):
                assert open(os.path.join(a, f), 'rb').read() == open(os.path.join(b, f), 'rb').read(), (j, f)
                n += 1
    assert n >= 4
