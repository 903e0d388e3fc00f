"""The colour exact stage's fallback branch (ia_color3.hip: `full = full || nc > C3_CAND`,
64 candidate tiles of 32 rows) against the C oracle (nch = 3): colour label maps whose flat
queries tie over more than 64 tiles (every tile of the level is then rescored), over exactly
64 tiles (the last clist slot, no full scan), and a constant-colour A.  Both screens
(IA_DB_ROT 1 / 0), the levels pipelined or not; B' in all channels, s, im and the
approximate pick of every pixel equal the oracle's, and ia_diag_color16_stats proves the
branch ran."""
import ctypes

import numpy as np
import pytest

import ia_oracle as o
import ia_oracle_c as oc
from conftest import smooth_noise
from test_gpu_fallback import (C3_CAND, app_reference, colour_label_inputs, colour_pyramids, dev,
                               queries_from, tie_segments)

pytestmark = pytest.mark.gpu

CASES = {   # seed, A, B, n_ap, patch: rows, tiles
    'over': (90, (72, 90), (30, 34), 2, 24),     # 12,960 rows, 405 tiles
    'at1': (95, (32, 64), (16, 24), 1, 12),      # 2,048 rows, 64 tiles
    'at2': (96, (32, 32), (16, 24), 2, 6),       # 2,048 rows, 64 tiles over both images
}
K = 1.0


class ColourCase:
    """One colour input with its oracle run, computed once and shared by the forms."""

    def __init__(self, pyr, tie=True):
        self.pyr = pyr
        A_pyr, Ap_list, B_pyr, Bp_pyr, L = pyr
        self.L = L
        self.w = o.compute_weights(3, 5, 12, 3)
        Bp = [b.copy() for b in Bp_pyr]
        self.ref = oc.synthesize(A_pyr, Ap_list, B_pyr, Bp, L, K, self.w)
        self.app = {}
        for l in range(1, L):
            db = oc.LevelDB(l, A_pyr, Ap_list)
            Q = queries_from(l, B_pyr, Bp_pyr, Bp)
            nn, sa, d = app_reference(db, Q, self.ref[l][1], self.ref[l][2], B_pyr[l].shape[:2],
                                      A_pyr[l].shape[:2], self.w)
            self.app[l] = (sa, d)
            if tie and l == L - 1:    # tiles: 32 consecutive rows, the last tile padded with the last row
                self.ntiles = (db.N + 31) // 32
                self.ties = tie_segments(db.rows, nn, np.arange(self.ntiles * 32), 32)
        self.queries = sum(B_pyr[l].shape[0] * B_pyr[l].shape[1] for l in range(1, L))


_CASES = {}


def colour_case(name):
    if name not in _CASES:
        if name == 'const':     # A = (0.25, 0.5, 0.75), A' = 0.5 at 36 x 44, every level
            A = np.dstack([np.full((36, 44), v) for v in (0.25, 0.5, 0.75)])
            B = np.dstack([smooth_noise(98 + 17 * ch, (30, 34)) for ch in range(3)])
            A_pyr, Ap_list, B_pyr, _, L = colour_pyramids(A, [np.full((36, 44, 3), 0.5)], B)
            _CASES[name] = ColourCase((A_pyr, Ap_list, B_pyr, o.initialize_Bp(B_pyr, True, 98), L), tie=False)
        else:
            seed, A, B, n_ap, patch = CASES[name]
            _CASES[name] = ColourCase(colour_label_inputs(seed, A, B, n_ap, 0, patch, cap=1))
    return _CASES[name]


@pytest.fixture
def color16():
    """Select the 3-channel matcher (1 screen + exact stage, 0 exhaustive fp64)."""
    import _ia
    lib = _ia.lib()
    prev = lib.ia_diag_set_color16(1)
    yield lib.ia_diag_set_color16
    lib.ia_diag_set_color16(prev)


def run(case, pipeline):
    """One debug synthesis compared with the oracle -> (candidate tiles, full scans)."""
    import _ia
    import image_analogies as ia
    A_pyr, Ap_list, B_pyr, Bp_pyr, L = case.pyr
    st = (ctypes.c_ulonglong * 2)()
    _ia.check(_ia.lib().ia_diag_color16_stats(st), 'stats')       # (reading clears the counters)
    Bp_dev = [dev(b) for b in Bp_pyr]
    out = ia.synthesize_dev([dev(p) for p in A_pyr], [[dev(p) for p in q] for q in Ap_list],
                            [dev(p) for p in B_pyr], Bp_dev, L, K, case.w, debug=True, pipeline=pipeline)
    _ia.check(_ia.lib().ia_diag_color16_stats(st), 'stats')
    assert set(out) == set(case.ref)
    for l in sorted(case.ref):
        Bp, s, im = case.ref[l]
        assert np.array_equal(out[l][0].cpu().numpy(), s), l
        assert np.array_equal(out[l][1].cpu().numpy(), im), l
        assert np.array_equal(Bp_dev[l].cpu().numpy(), Bp), l
        rec = ia.debug_record(out[l][0], out[l][1], out[l][2], Bp.shape[:2])
        sa, d = case.app[l]
        assert rec['sa'] == sa, l
        assert np.array_equal(rec['app_dist'], d), l
    return int(st[0]), int(st[1])


@pytest.mark.parametrize('pipeline', [True, False])
@pytest.mark.parametrize('rot', ['1', '0'])
def test_colour_over_cap_full_scan_vs_oracle(gpu, color16, monkeypatch, rot, pipeline):
    """A 72 x 90, two A' images (12,960 rows, 405 tiles): the flat queries tie over more than
    64 tiles, so the exact stage rescores every tile of the level."""
    color16(1)
    monkeypatch.setenv('IA_DB_ROT', rot)
    case = colour_case('over')
    want = int((case.ties > C3_CAND).sum())
    assert case.ntiles == 405 and want >= 100, want
    tiles, full = run(case, pipeline)
    print('colour over cap [rot %s, pipeline %s]: reference %d queries over %d tiles (most %d), full scans '
          '%d, candidate tiles %d' % (rot, pipeline, want, C3_CAND, case.ties.max(), full, tiles))
    assert full >= want
    assert tiles >= case.ntiles * want


@pytest.mark.parametrize('pipeline', [True, False])
def test_colour_over_cap_exhaustive_vs_oracle(gpu, color16, pipeline):
    """The same input through the exhaustive fp64 search (ia_diag_set_color16(0))."""
    color16(0)
    run(colour_case('over'), pipeline)


@pytest.mark.parametrize('pipeline', [True, False])
@pytest.mark.parametrize('rot', ['1', '0'])
@pytest.mark.parametrize('name', ['at1', 'at2'])
def test_colour_at_cap_no_full_scan_vs_oracle(gpu, color16, monkeypatch, name, rot, pipeline):
    """2,048 rows = exactly 64 tiles, every one holding a tied row (A 32 x 64 with one A'; A
    32 x 32 with two A' images of one background, the winner row 0): the flat queries fill
    clist to its last slot and must NOT scan (`nc > C3_CAND`, not `>=`)."""
    color16(1)
    monkeypatch.setenv('IA_DB_ROT', rot)
    case = colour_case(name)
    want = int((case.ties == C3_CAND).sum())
    assert case.ntiles == C3_CAND and want >= 96 and case.ties.max() == C3_CAND, want
    tiles, full = run(case, pipeline)
    print('colour at cap %s [rot %s, pipeline %s]: reference %d queries over exactly %d tiles, full scans '
          '%d, candidate tiles %d' % (name, rot, pipeline, want, C3_CAND, full, tiles))
    assert full == 0
    assert tiles >= C3_CAND * want


@pytest.mark.parametrize('rot', ['1', '0'])
def test_colour_constant_A_vs_oracle(gpu, color16, monkeypatch, rot):
    """A constant-colour A (0.25, 0.5, 0.75) with A' = 0.5 at 36 x 44, every level: a zero
    amax and a zero covariance for the rotation; the oracle's result."""
    color16(1)
    monkeypatch.setenv('IA_DB_ROT', rot)
    run(colour_case('const'), True)
