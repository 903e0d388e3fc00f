"""The 165-dim LSH matcher's host side: the numpy restatement tests/lsh3_ref.py against the
oracle's luminance LshIndex (the same definition at D = 55), what the restatement does on the
GPU tests' inputs (an LSH synthesis is far from the exact one, through both bucket paths), and
the host interface (projections for dim = 165, the C-ABI's new entry points)."""
import numpy as np
import pytest

import ia_oracle as o
import lsh3_ref as r


def test_restatement_equals_the_oracle_at_d55():
    """At D = 55 the helper's keys and match equal o.LshIndex's bit for bit: 500 random rows,
    100 queries (rows, perturbed rows, uniform), (L, k, w) = (8, 3, 0.3)."""
    rs = np.random.RandomState(11)
    As = rs.rand(500, 55)
    center = As.mean(0)
    L, k, w = 8, 3, np.float32(0.3)
    proj = r.projections(L, k, 0.3, 5, 55)
    assert proj.shape == (24, 56)
    Q = np.vstack([As[rs.randint(0, 500, 40)], As[rs.randint(0, 500, 40)] + rs.randn(40, 55) * 0.01,
                   rs.rand(20, 55)])
    ref = o.LshIndex(As, center, proj, L, k, w)
    got = r.LshIndexD(As, center, proj, L, k, w)
    X32 = (As - center[None, :]).astype(np.float32)
    assert np.array_equal(got.keys, o.lsh_hash_keys(X32, proj, L, k, w, ref.bits))
    for t in range(L):
        assert np.array_equal(got.order[t], ref.order[t])
    ri, rd = ref.match(Q)
    gi, gd = got.match(Q)
    assert np.array_equal(gi, ri)
    assert np.array_equal(gd, rd)
    assert got.lookups == len(Q) * L


@pytest.mark.parametrize('params', r.SYNTH_PARAMS, ids=lambda p: '%d-%d-%g-%d' % p)
def test_lsh_synthesis_is_far_from_the_exact_one(params):
    """On the GPU tests' inputs the oracle driven by the restatement differs from the exact
    oracle synthesis on at least half the pixels of every level (a pixel differs when its source
    (s, im) does): a device path that silently ran the exact matcher cannot pass the parity
    tests.  Both look-up paths matter: with (8, 3, 1.0, 7) at least one look-up in ten of the
    finest level meets an empty bucket, with (4, 1, 4.0, 1) a bucket of more than 32 rows."""
    case = r.case()
    A_pyr, Ap_list, _, _, L, As, _ = case
    exact, _, _ = exact_run()
    got, _, tabs = r.oracle_synthesis(
        case, 1.0, lambda level: r.host_tables(A_pyr, Ap_list, As[level], level, *params))
    for level in range(1, L):
        diff = np.any(got[level][0] != exact[level][0], axis=1) | (got[level][1] != exact[level][1])
        print('level %d: %.3f of the pixels differ from the exact synthesis' % (level, diff.mean()))
        assert diff.mean() >= 0.5, (level, diff.mean())
    t = tabs[L - 1]
    print('finest level: %.3f of the look-ups empty, %.3f capped' % (t.empty / t.lookups, t.capped / t.lookups))
    share = (t.empty if params == r.SYNTH_PARAMS[0] else t.capped) / t.lookups
    assert share >= 0.1, share


_EXACT = []


def exact_run():
    if not _EXACT:
        _EXACT.append(r.oracle_synthesis(r.case(), 1.0))
    return _EXACT[0]


def test_projections_for_165_dims_and_the_default():
    """lsh_projections(dim=165): rows of 168 floats (p, the offset in element 165, zeros), drawn
    as the restatement draws them; the default (dim = 55) stays the array it was."""
    import algorithms
    P = algorithms.lsh_projections(2, 3, 0.5, 1, dim=165)
    assert P.shape == (6, 168) and P.dtype == np.float32
    assert np.array_equal(P, r.projections(2, 3, 0.5, 1, 165))
    assert np.all(P[:, 166:] == 0) and np.all((0 <= P[:, 165]) & (P[:, 165] < 0.5))
    rs = np.random.RandomState(3)
    old = np.zeros((8, 56), dtype=np.float32)
    old[:, :55] = rs.standard_normal((8, 55))
    old[:, 55] = rs.uniform(0.0, 0.7, 8)
    assert np.array_equal(algorithms.lsh_projections(4, 2, 0.7, 3), old)
    assert np.array_equal(algorithms.lsh_projections(4, 2, 0.7, 3, dim=55), old)


def test_c_abi_declares_the_165_dim_lsh():
    import _ia
    names = _ia.declared_symbols()
    for name in ('ia_lsh3_build', 'ia_lsh3_bytes', 'ia_lsh3_match_batch'):
        assert name in names and name in _ia._SIGS, name
