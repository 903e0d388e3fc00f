"""Host-side checks of training pairs (A_i, A'_i): the pair oracle's recipe
(tests/pairs_oracle.py) against the oracle's own runs, the C-ABI's nA field and what the host
entries answer for it, and the Python entries' argument checks.  No device."""
import ctypes
import os

import numpy as np
import pytest

import ia_oracle as o
import ia_oracle_c as oc
import pairs_oracle as po


# ---- the recipe ------------------------------------------------------------------------------

@pytest.mark.parametrize('channels,A_shape,B_shape', [(1, (20, 26), (18, 21)), (3, (16, 20), (14, 17))])
def test_recipe_with_equal_A_is_the_oracle(channels, A_shape, B_shape):
    """With every A_i the same image the stacked rows are today's database: the recipe equals
    oc.synthesize of one A and n A' images."""
    A_pyrs, Ap_list, B_pyr, Bp_pyr, L = po.pyramids(2, A_shape, B_shape, channels=channels)
    w = po.weights(channels)
    same = [A_pyrs[0], A_pyrs[0]]
    got = po.synthesize(same, Ap_list, B_pyr, Bp_pyr, L, po.KAPPA, w)
    ref = oc.synthesize(A_pyrs[0], Ap_list, B_pyr, [b.copy() for b in Bp_pyr], L, po.KAPPA, w)
    assert set(got) == set(ref) and len(ref) >= 2
    for l in ref:
        for x, y in zip(got[l], ref[l]):
            assert np.array_equal(x, y), l


def test_recipe_equals_python_oracle_over_stacked_rows():
    """Luminance: the recipe equals o.synthesize_level(..., As_level=the stacked rows), which
    takes every row from As_level too; and it differs from the single-A run."""
    A_pyrs, Ap_list, B_pyr, Bp_pyr, L = po.pyramids(2, (20, 26), (18, 21))
    w = po.weights()
    got = po.synthesize(A_pyrs, Ap_list, B_pyr, Bp_pyr, L, po.KAPPA, w)
    Bp = [b.copy() for b in Bp_pyr]
    for l in range(1, L):
        rows = po.stacked_rows(l, A_pyrs, Ap_list)
        s, im = o.synthesize_level(l, L, A_pyrs[0], Ap_list, B_pyr, Bp, rows, w, po.KAPPA)
        assert np.array_equal(s, got[l][1]) and np.array_equal(im, got[l][2]), l
        assert np.array_equal(Bp[l], got[l][0]), l
    single = oc.synthesize(A_pyrs[0], Ap_list, B_pyr, [b.copy() for b in Bp_pyr], L, po.KAPPA, w)
    assert any(not np.array_equal(single[l][1], got[l][1]) or not np.array_equal(single[l][2], got[l][2])
               for l in got)


def test_stacked_rows_layout():
    """Row (i, r, c) of the stacked rows is [full(A_i) | half(A'_i)] at (r, c)."""
    A_pyrs, Ap_list, _, _, L = po.pyramids(3, (13, 17), (12, 14))
    l = L - 1
    rows = po.stacked_rows(l, A_pyrs, Ap_list)
    h, w = A_pyrs[0][l].shape
    assert rows.shape == (3 * h * w, 55)
    for i in range(3):
        full = o.level_features(A_pyrs[i][l - 1], A_pyrs[i][l], True)
        half = o.level_features(Ap_list[i][l - 1], Ap_list[i][l], False)
        assert np.array_equal(rows[i * h * w:(i + 1) * h * w], np.hstack([full, half]))


# ---- the C-ABI ---------------------------------------------------------------------------------

def src(Ah, Aw, nAp, nA):
    """An IaSrcLevel of that geometry over fake (never dereferenced) pointers."""
    import _ia
    s = _ia.IaSrcLevel()
    s.A_sm, s.A_lg, s.Ap_sm, s.Ap_lg = 0x1000, 0x2000, 0x3000, 0x4000
    s.A_hs, s.A_ws, s.Ah, s.Aw, s.nAp, s.nA = (Ah + 1) // 2, (Aw + 1) // 2, Ah, Aw, nAp, nA
    return s


def test_src_level_keeps_its_size():
    import _ia
    assert ctypes.sizeof(_ia.IaSrcLevel) == 56
    assert 'nA' in [f[0] for f in _ia.IaSrcLevel._fields_]
    assert _ia.IaSrcLevel.nA.offset == _ia.IaSrcLevel.nAp.offset + 4 == 52
    assert _ia.IaSynthArgs.db.offset == 56 and _ia.IaMatchArgs.db.offset == 56


def test_image_form_is_one_A_only():
    """A 128 x 128 level of two A' images: the image form with nA 0 and 1, none for two pairs;
    no compact rotated database for pairs; the rotated rows apply to both."""
    import _ia
    lib = _ia.lib()
    N = 2 * 128 * 128
    for nA in (0, 1):
        assert lib.ia_db_image_bytes(ctypes.byref(src(128, 128, 2, nA)), 0, N) > 0
    assert lib.ia_db_image_bytes(ctypes.byref(src(128, 128, 2, 2)), 0, N) == 0
    assert lib.ia_db_image_bytes(ctypes.byref(src(128, 128, 3, 2)), 0, N) == 0     # (a bad nA)
    for nA in (0, 1, 2):
        assert lib.ia_db_rot_applies(ctypes.byref(src(128, 128, 2, nA)), 0, N) == 1
    assert lib.ia_db_rot_applies(ctypes.byref(src(128, 128, 3, 2)), 0, N) == 0
    # a level large enough for the compact form with one A
    big = 2 * 512 * 512
    prev = lib.ia_diag_set_compact_min_rows(-1)
    try:
        lib.ia_diag_set_compact_min_rows(1 << 18)
        if lib.ia_db_rotk_bytes(big):
            assert lib.ia_db_rotk_applies(ctypes.byref(src(512, 512, 2, 1)), 0, big) == 1
        assert lib.ia_db_rotk_applies(ctypes.byref(src(512, 512, 2, 2)), 0, big) == 0
    finally:
        lib.ia_diag_set_compact_min_rows(prev)


def test_bad_nA_is_refused_by_name():
    """nA other than 0, 1 or nAp: IA_E_ARG with a message naming nA, before any device call."""
    import _ia
    lib = _ia.lib()
    bad = src(32, 32, 3, 2)
    N = 3 * 32 * 32
    fake = ctypes.c_void_p(0x5000)
    calls = {
        'ia_db_build': lambda: lib.ia_db_build(ctypes.byref(bad), 0, N, fake, fake, fake, None),
        'ia_db_build_image': lambda: lib.ia_db_build_image(ctypes.byref(bad), 0, N, fake, None, fake, fake, None),
        'ia_db_cov': lambda: lib.ia_db_cov(ctypes.byref(bad), 0, N, fake, fake, None),
        'ia_db_build_rot': lambda: lib.ia_db_build_rot(ctypes.byref(bad), 0, N, fake, fake, fake, fake, None),
        'ia_db3_build': lambda: lib.ia_db3_build(ctypes.byref(bad), 0, N, fake, None),
    }
    lsh = _ia.IaLsh()
    lsh.mem, lsh.proj, lsh.L, lsh.k, lsh.w = 0x6000, 0x7000, 2, 2, 1.0
    calls['ia_lsh_build'] = lambda: lib.ia_lsh_build(ctypes.byref(bad), 0, N, fake, ctypes.byref(lsh), None)
    a = _ia.IaSynthArgs()
    a.src, a.db, a.nrows, a.N_total = bad, 0x8000, N, N
    out4 = (ctypes.c_int * 4)()
    plan = (ctypes.c_int * len(_ia.PLAN_KEYS))()
    grp = (ctypes.c_int * 1)()
    calls['ia_level_resources'] = lambda: lib.ia_level_resources(ctypes.byref(a), out4)
    calls['ia_level3_resources'] = lambda: lib.ia_level3_resources(ctypes.byref(a), out4)
    calls['ia_diag_level_plan'] = lambda: lib.ia_diag_level_plan(ctypes.byref(a), 1, plan)
    calls['ia_batch_groups'] = lambda: lib.ia_batch_groups(ctypes.byref(a), 1, grp)
    calls['ia_batch3_groups'] = lambda: lib.ia_batch3_groups(ctypes.byref(a), 1, grp)
    for who, call in calls.items():
        assert call() == _ia.IA_E_ARG, who
        assert 'nA' in lib.ia_last_error().decode(), (who, lib.ia_last_error())
    # the image form and the compact form of pairs: refused by name too
    pairs = src(128, 128, 2, 2)
    assert lib.ia_db_build_image(ctypes.byref(pairs), 0, 2 * 128 * 128, fake, None, fake, fake, None) == _ia.IA_E_ARG
    assert 'nA' in lib.ia_last_error().decode()
    if lib.ia_db_rotk_bytes(1 << 19):
        assert lib.ia_db_build_rotk(ctypes.byref(src(512, 512, 2, 2)), 0, 1 << 19, fake, fake, fake, fake,
                                    None) == _ia.IA_E_ARG
        assert 'nA' in lib.ia_last_error().decode()


def groups(fn, nAs):
    """ia_batch_groups / ia_batch3_groups over jobs x, y, x, y, x, z (fake database pointers)
    whose sources carry the given nA."""
    import _ia
    ptrs = (0x7000, 0x8000, 0x7000, 0x8000, 0x7000, 0x9000)
    arr = (_ia.IaSynthArgs * len(ptrs))()
    for a, p, nA in zip(arr, ptrs, nAs):
        a.dbr = p
        a.src = src(32, 32, 2, nA)
    out = (ctypes.c_int * len(ptrs))(*([-1] * len(ptrs)))
    return getattr(_ia.lib(), fn)(arr, len(ptrs), out), list(out)


@pytest.mark.parametrize('fn', ['ia_batch_groups', 'ia_batch3_groups'])
def test_batch_groups_do_not_depend_on_nA(fn):
    want = (3, [0, 1, 0, 1, 0, 2])
    for nAs in ([0] * 6, [1] * 6, [2] * 6, [2, 1, 2, 1, 2, 0]):
        assert groups(fn, nAs) == want, nAs


# ---- the Python entries' argument checks (before any device work) --------------------------

def test_a_images_counts():
    import image_analogies as ia
    x = np.zeros((4, 4))
    assert ia.a_images(x, 3) == ([x], False)
    assert ia.a_images([x], 3)[1] is False and ia.a_images((x,), 1)[1] is False
    got, pairs = ia.a_images([x, x, x], 3)
    assert pairs and len(got) == 3
    for n in (2, 4):
        with pytest.raises(ValueError, match='one A per A'):
            ia.a_images([x] * n, 3)


def test_setup_refuses_mismatches_before_the_device(monkeypatch, tmp_path):
    import types
    import _ia
    import image_analogies as ia

    def no_device(*a, **kw):
        raise AssertionError('device work before the argument checks')
    monkeypatch.setattr(_ia, 'require_device', no_device)
    c = types.SimpleNamespace(convert=False, remap_lum=False)
    x, y = np.zeros((8, 9)), np.zeros((8, 10))
    with pytest.raises(ValueError, match='one A per A'):
        ia.setup_dev([x, x, x], [x, x], x, c)
    with pytest.raises(ValueError, match='one shape'):
        ia.setup_dev([x, y], [x, x], x, c)
    with pytest.raises(ValueError, match='one shape'):
        ia.setup_dev([x, x], [x, y], x, c)
    # the file entries: refused before a file is read or the output directory is made
    out = str(tmp_path / 'out') + '/'
    with pytest.raises(ValueError, match='one A per A'):
        ia.image_analogies_main(['a.png', 'b.png', 'c.png'], ['ap.png', 'bp.png'], 'b.png', out, c)
    with pytest.raises(ValueError, match='one A per A'):
        ia.img_setup(['a.png', 'b.png'], ['ap.png'], 'b.png', out, c)
    with pytest.raises(ValueError, match='one A per A'):
        ia.multi_main([(['a.png', 'b.png', 'c.png'], ['ap.png', 'bp.png'], 'b.png', out)], c, rank=0, world=1, batch=2)
    assert not os.path.exists(out)


def test_a_level_and_pyramid_lists():
    import torch
    import algorithms
    p = [torch.zeros(2, 3), torch.zeros(4, 6)]
    q = [torch.ones(2, 3), torch.ones(4, 6)]
    assert algorithms.a_pyramids(p) == [p] and algorithms.a_pyramids([p, q]) == [p, q]
    sm, lg, nA = algorithms.a_level(p, 2, 1)
    assert nA == 1 and sm is p[0] and lg is p[1]
    assert algorithms.a_level([p], 2, 1)[2] == 1
    sm, lg, nA = algorithms.a_level([p, q], 2, 1)
    assert nA == 2 and sm.shape == (2, 2, 3) and lg.shape == (2, 4, 6) and float(lg[1].min()) == 1.0
    with pytest.raises(ValueError, match='one A per A'):
        algorithms.a_level([p, q], 3, 1)


def test_src_level_takes_nA_from_its_argument():
    """A luminance stack (n, h, w) and a colour image (h, w, 3) have the same rank: nA is what
    the caller states."""
    import torch
    import _ia
    Ap_sm, Ap_lg = torch.zeros(3, 2, 3), torch.zeros(3, 4, 6)
    s = _ia.src_level(torch.zeros(2, 3), torch.zeros(4, 6), Ap_sm, Ap_lg)
    assert (s.nA, s.nAp, s.Ah, s.Aw, s.A_hs, s.A_ws) == (1, 3, 4, 6, 2, 3)
    s = _ia.src_level(Ap_sm, Ap_lg, Ap_sm, Ap_lg, nA=3)
    assert (s.nA, s.nAp, s.Ah, s.Aw) == (3, 3, 4, 6)
    with pytest.raises(ValueError, match='nA'):
        _ia.src_level(Ap_sm, Ap_lg, Ap_sm, Ap_lg, nA=2)
    with pytest.raises(ValueError):
        _ia.src_level(torch.zeros(2, 3), torch.zeros(4, 6), Ap_sm, Ap_lg, nA=3)


def test_db_groups_and_run_key_see_the_pairs():
    import types
    import torch
    import image_analogies as ia
    p = [torch.zeros(2, 3), torch.zeros(4, 6)]
    q = [torch.ones(2, 3), torch.ones(4, 6)]
    r = [torch.ones(2, 3), torch.ones(4, 6)]
    B = [torch.zeros(2, 2), torch.zeros(4, 4)]
    jobs = [([p, q], [p, q], B, B), ([p, q], [p, q], B, B), (p, [p, q], B, B), ([p, r], [p, q], B, B), ([p], [p, q], B, B)]
    assert ia.db_groups(jobs) == [0, 0, 1, 2, 1]
    c = types.SimpleNamespace(num_ch=1, max_levels=2)
    k1, k2 = ia._run_key(c, p, [p, q], B), ia._run_key(c, [p, q], [p, q], B)
    assert k1 != k2 and k1 == ia._run_key(c, [p], [p, q], B) and k2 == ia._run_key(c, [p, r], [p, q], B)
