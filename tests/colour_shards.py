"""Inputs and oracle runs of the sharded 3-channel tests (test_color3_shard_cases.py on the CPU,
test_gpu_color3_shards.py and its rank processes exchange_worker3.py on the GPU).  Not a test
module.

The label cases are colour label maps under a 1-level pyramid cap (one synthesised level, the
finest), kappa = 1: their flat queries equal the flat rows bit for bit, so whole tiles tie and
the cross-rank tie rule (the lowest global row) decides.  CASES gives per case the input and
the worlds it runs at as {world: pipelined}; `noise` is the smooth-noise input with every level
sharded."""
import numpy as np

import ia_oracle as o
import ia_oracle_c as oc

K_LABEL = 1.0
CASES = {   # seed, A, B, n_ap, band, patch; {world: pipelined}
    'at2': ((96, (32, 32), (16, 24), 2, 0, 6), {2: True, 3: False}),
    'tie_late': ((112, (60, 52), (16, 24), 1, 24, 0), {3: False}),
    'over': ((90, (72, 90), (30, 34), 2, 0, 24), {2: True}),
}
NOISE = (171, (26, 31), (20, 24), 2, 0.9)     # seed, A, B, n_ap, kappa
NOISE_WORLDS = {2: True, 3: False}


def shard_rows(N, rank, world):
    """image_analogies.shard_rows, restated for the CPU tests (no torch import)."""
    r0 = N * rank // world
    return r0, N * (rank + 1) // world - r0


def label_pyramids(name):
    from test_gpu_fallback import colour_label_inputs
    seed, A, B, n_ap, band, patch = CASES[name][0]
    return colour_label_inputs(seed, A, B, n_ap, band, patch, cap=1)


def noise_pyramids():
    from test_gpu_color3 import inputs
    seed, A, B, n_ap, _ = NOISE
    return inputs(seed, A, B, n_ap=n_ap)


def pyramids(name):
    """(pyramids, kappa) of a label case or of 'noise'."""
    if name == 'noise':
        return noise_pyramids(), NOISE[4]
    return label_pyramids(name), K_LABEL


class Reference:
    """One input's oracle run (nch = 3): per level (B', s, im) and the approximate picks and
    distances of the debug record; for the finest level its rows and every query's exact
    nearest row (the lowest among ties)."""

    def __init__(self, name):
        from test_gpu_fallback import app_reference, queries_from
        self.pyr, self.k = pyramids(name)
        A_pyr, Ap_list, B_pyr, Bp_pyr, L = self.pyr
        self.L = L
        self.w = o.compute_weights(3, 5, 12, 3)
        Bp = [b.copy() for b in Bp_pyr]
        self.ref = oc.synthesize(A_pyr, Ap_list, B_pyr, Bp, L, self.k, self.w)
        self.app = {}
        for l in range(1, L):
            db = oc.LevelDB(l, A_pyr, Ap_list)
            Q = queries_from(l, B_pyr, Bp_pyr, Bp)
            nn, sa, d = app_reference(db, Q, self.ref[l][1], self.ref[l][2], B_pyr[l].shape[:2],
                                      A_pyr[l].shape[:2], self.w)
            self.app[l] = (sa, d)
            if l == L - 1:
                self.rows, self.nn, self.N = db.rows.copy(), np.asarray(nn), db.N

    def shard(self, rank, world):
        """The finest level's shard of one rank: (row0, nrows, tiles, tied tiles per query,
        queries it wins).  A tile is 32 consecutive local rows, the last padded with the last
        row; a tied tile holds a row bit-identical to the query's nearest row of the level."""
        from test_gpu_fallback import tie_segments
        row0, nrows = shard_rows(self.N, rank, world)
        ntiles = (nrows + 31) // 32
        ties = tie_segments(self.rows[row0:row0 + nrows], self.nn, np.arange(ntiles * 32), 32, pool=self.rows)
        wins = int(((self.nn >= row0) & (self.nn < row0 + nrows)).sum())
        return row0, nrows, ntiles, ties, wins


_REFS = {}


def reference(name):
    if name not in _REFS:
        _REFS[name] = Reference(name)
    return _REFS[name]
