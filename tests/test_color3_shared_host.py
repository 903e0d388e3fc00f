"""Host-side checks of the colour batch's DB groups: ia_batch3_groups (pure pointer comparison,
no device call) on hand-made IaSynthArgs arrays, and image_analogies.db_groups (tensor identity,
no content comparison) on CPU tensors."""
import ctypes

import torch


def groups_of(dbrs):
    """ia_batch3_groups over jobs whose dbr fields are the given fake (never dereferenced)
    addresses: (return value, group_of_job)."""
    import _ia
    K = len(dbrs)
    arr = (_ia.IaSynthArgs * max(K, 1))()
    for a, p in zip(arr, dbrs):
        a.dbr = p
    out = (ctypes.c_int * max(K, 1))(*([-9] * max(K, 1)))
    return _ia.lib().ia_batch3_groups(arr, K, out), list(out)[:K]


def test_batch3_groups_by_pointer():
    X, Y = 0x1000, 0x2000
    assert groups_of([X, Y, X, Y, X]) == (2, [0, 1, 0, 1, 0])
    assert groups_of([0x100 * (k + 1) for k in range(6)]) == (6, list(range(6)))
    assert groups_of([X] * 7) == (1, [0] * 7)
    assert groups_of([Y, Y, X, Y, 0x3000, X]) == (3, [0, 0, 1, 0, 2, 1])
    assert groups_of([X]) == (1, [0])
    # a job without a rotated DB shares with nobody
    assert groups_of([0, 0, X, X]) == (3, [0, 1, 2, 2])


def test_batch3_groups_refuses_bad_arguments():
    import _ia
    lib = _ia.lib()
    arr = (_ia.IaSynthArgs * 2)()
    out = (ctypes.c_int * 2)()
    assert lib.ia_batch3_groups(arr, 0, out) == _ia.IA_E_ARG
    assert 'K' in lib.ia_last_error().decode()
    assert lib.ia_batch3_groups(arr, -1, out) < 0
    assert lib.ia_batch3_groups(arr, 129, out) < 0
    assert lib.ia_batch3_groups(None, 2, out) == _ia.IA_E_ARG
    assert lib.ia_batch3_groups(arr, 2, None) == _ia.IA_E_ARG


def test_headers_declare_the_new_entries():
    import _ia
    assert 'ia_batch3_groups' in _ia.declared_symbols()
    assert 'ia_diag_set_c3_shared_screen' in _ia.declared_symbols('all')
    assert 'ia_diag_set_c3_shared_screen' not in _ia.declared_symbols()
    assert {'ia_batch3_groups', 'ia_diag_set_c3_shared_screen'} <= set(_ia._SIGS)


def test_shared_screen_knob_reads_and_sets():
    import _ia
    lib = _ia.lib()
    prev = lib.ia_diag_set_c3_shared_screen(-1)
    try:
        assert prev in (0, 1)
        assert lib.ia_diag_set_c3_shared_screen(0) == prev
        assert lib.ia_diag_set_c3_shared_screen(-1) == 0
        assert lib.ia_diag_set_c3_shared_screen(7) == 0      # other values leave it
        assert lib.ia_diag_set_c3_shared_screen(1) == 0
        assert lib.ia_diag_set_c3_shared_screen(-1) == 1
    finally:
        lib.ia_diag_set_c3_shared_screen(prev)


def test_db_groups_is_tensor_identity():
    import image_analogies as ia

    def pyr():
        return [torch.zeros(4, 5, 3, dtype=torch.float64), torch.zeros(8, 10, 3, dtype=torch.float64)]
    A, Ap, Ap2, A_other, Ap_other = pyr(), pyr(), pyr(), pyr(), pyr()
    job = lambda a, aps: (a, aps, None, None)  # noqa: E731
    # the same objects, other list objects around the same tensors, equal contents elsewhere
    jobs = [job(A, [Ap]), job(A_other, [Ap_other]), job(list(A), [list(Ap)]), job(A, [Ap_other]),
            job(A, [Ap, Ap2]), job(A_other, [Ap_other]), job(A, [Ap, Ap2])]
    assert ia.db_groups(jobs) == [0, 1, 0, 2, 3, 1, 3]
    # a view of other strides over the same memory is another tensor
    base = torch.zeros(8, 10, 6, dtype=torch.float64)
    v = [torch.zeros(4, 5, 3, dtype=torch.float64), base[..., :3]]
    w = [v[0], base[..., :3]]
    c = [v[0], base[..., :3].contiguous()]
    assert ia.db_groups([job(v, [Ap]), job(w, [Ap]), job(c, [Ap])]) == [0, 0, 1]
