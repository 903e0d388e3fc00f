"""The oracle for training pairs (A_i, A'_i) (a helper module of test_pairs_host.py and
test_gpu_pairs.py, not a conftest).

With n pairs of one shape, level l's database is vstack_i [full(A_i) | half(A'_i)], row
ix = (i * Ah + r) * Aw + c.  The C oracle's ia_oracle_synth_level takes every database row
from the buffer it is given (the 1-NN, the coherence candidates and both kappa distances) and
reads only A' from the pyramids, for the B' update.  So the pair oracle is: per pair i the rows
oc.LevelDB(level, A_pyr_i, [Ap_pyr_i]).rows, stacked; then one oc.LevelJob over (A_pyr_0, all
A' pyramids) run through ia_oracle_synth_level with that buffer.  Nothing under oracle/ changes.
"""
import ctypes
import functools

import numpy as np

import ia_oracle as o
import ia_oracle_c as oc
from conftest import smooth_noise

SEED, CAP, KAPPA = 57, 2, 0.5


def colour(seed, shape):
    return np.dstack([smooth_noise(seed + 17 * ch, shape) for ch in range(3)])


def pyramid(img, cap=CAP):
    """The oracle's pyramid of a luminance (h, w) or colour (h, w, 3: per channel) image."""
    if img.ndim == 2:
        return o.compute_gaussian_pyramid(img, 3, cap)
    chans = [o.compute_gaussian_pyramid(img[..., ch], 3, cap) for ch in range(3)]
    return [np.dstack([c[l] for c in chans]) for l in range(len(chans[0]))]


def pair_images(n, A_shape, B_shape, seed=SEED, channels=1, scale0=1.0):
    """A_i = smooth_noise(seed + 10 i), A'_i = gaussian_filter(A_i, 1 + 0.5 i), B =
    smooth_noise(seed + 1) (3 channels: three differently seeded channels, filtered per
    channel).  scale0: pair 0 (A_0 and A'_0) times that factor."""
    from scipy.ndimage import gaussian_filter
    img = smooth_noise if channels == 1 else colour
    As = [img(seed + 10 * i, A_shape) for i in range(n)]
    sig = lambda i: (1.0 + 0.5 * i,) * 2 + ((0,) if channels == 3 else ())  # noqa: E731
    Aps = [gaussian_filter(A, sig(i)) for i, A in enumerate(As)]
    As[0], Aps[0] = As[0] * scale0, Aps[0] * scale0
    return As, Aps, img(seed + 1, B_shape)


@functools.lru_cache(maxsize=None)
def pyramids(n, A_shape, B_shape, seed=SEED, channels=1, scale0=1.0, cap=CAP, b_seed=None):
    """(A pyramids, A' pyramids, B pyramid, B' init pyramid, max_levels) of n pairs: computed
    once, never modified.  b_seed: another B image and B' init over the same pairs."""
    As, Aps, B = pair_images(n, A_shape, B_shape, seed, channels, scale0)
    if b_seed is not None:
        B = (smooth_noise if channels == 1 else colour)(b_seed, B_shape)
    A_pyrs = [pyramid(A, cap) for A in As]
    Ap_list = [pyramid(Ap, cap) for Ap in Aps]
    B_pyr = pyramid(B, cap)
    L = min(len(A_pyrs[0]), len(B_pyr))
    Bp_pyr = o.initialize_Bp(B_pyr, True, seed if b_seed is None else b_seed)
    return A_pyrs, Ap_list, B_pyr, Bp_pyr, L


def weights(channels=1):
    return o.compute_weights(3, 5, 12, channels)


def stacked_rows(level, A_pyrs, Ap_list):
    """As[level] of the pairs: vstack_i of the oracle's rows of (A_i, [A'_i]), fp64 (N x 55 C)."""
    dbs = [oc.LevelDB(level, A, [Ap]) for A, Ap in zip(A_pyrs, Ap_list)]   # (rows: views while they live)
    return np.ascontiguousarray(np.vstack([db.rows for db in dbs]))


def synthesize(A_pyrs, Ap_list, B_pyr, Bp_pyr, L, k, w, rows_of=None):
    """Every level in scanline order by the C oracle over the stacked rows (B' on a copy).
    Returns {level: (B' level, s, im)}.  rows_of: level -> rows (default stacked_rows)."""
    Bp = [np.array(b, dtype=np.float64) for b in Bp_pyr]
    out = {}
    for level in range(1, L):
        rows = rows_of(level) if rows_of else stacked_rows(level, A_pyrs, Ap_list)
        job = oc.LevelJob(level, A_pyrs[0], Ap_list, B_pyr, Bp, w, 1 + (2.0 ** (level - L)) * k)
        assert rows.shape == (len(Ap_list) * job.L.Ah * job.L.Aw, job.D) and rows.flags.c_contiguous
        n = oc.lib().ia_oracle_synth_level(ctypes.byref(job.L), oc._d(rows))
        assert n >= 0
        Bp[level] = job.Bp_lg.reshape(Bp[level].shape)
        out[level] = (Bp[level].copy(), job.s.copy(), job.im.copy())
    return out


@functools.lru_cache(maxsize=None)
def reference(n, A_shape, B_shape, channels=1, scale0=1.0, k=KAPPA, b_seed=None):
    """The pair oracle's run of pyramids(...) (shared by the tests, never modified), checked not
    to degenerate: every pair wins at least 10 % of the pixels of every level."""
    A_pyrs, Ap_list, B_pyr, Bp_pyr, L = pyramids(n, A_shape, B_shape, SEED, channels, scale0, CAP, b_seed)
    ref = synthesize(A_pyrs, Ap_list, B_pyr, Bp_pyr, L, k, weights(channels))
    for level, (_, _, im) in ref.items():
        share = np.bincount(im, minlength=n) / float(len(im))
        assert share.min() >= 0.10, (level, share)
    return ref
