"""Generate tests/golden/ref_setup_golden.npz from the REFERENCE itself: its pyramids of images
outside [0, 1] (where skimage's clip to the blurred range engages) and one remap_luminance +
compress_values + pyramid chain.

Run with the image's Python 3.9 environment (numpy 1.26.4, scipy 1.7.1, scikit-image 0.18.3),
as tests/golden/make_golden.py:

    OPENBLAS_CORETYPE=SkylakeX /opt/conda/bin/python3.9 tests/golden/make_setup_golden.py

skimage's resize fits its sampling map with an SVD, so the last bits of the map, and with them
of every level, follow the BLAS kernels numpy runs.  That environment's OpenBLAS 0.3.23 does
not know recent CPUs and falls back to its SSE3 kernels; OPENBLAS_CORETYPE selects the AVX-512
kernels, which the OpenBLAS of current numpy wheels picks by itself on such CPUs and whose
results ref_golden.npz holds (under the fallback neither fixture is reproduced by the oracle
of this tree, whose fit runs on the tests' numpy).

It imports the reference's own ``img_preprocess.py`` from /root/reference (read-only; nothing is
copied) and records its OUTPUTS.  Only data is written (allow_pickle=False).  The inputs are
not stored: they come from the seeded generators below (numpy's legacy RandomState and IEEE
arithmetic, the same on every numpy), which the tests import from this file; the fixture
holds the SHA-256 of every input instead, and a pyramid's finest level (the input itself) is
left out.
"""
import hashlib
import os
import sys

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'ref_setup_golden.npz')

# (hi, lo) plateau constants whose resampled plateaus round outside the blurred range on odd
# sizes: mixed sign, both above 1, and one bound exactly 0.0 on either side
PLATEAUS = {'mixed': (0.44, -0.68), 'u8': (255.0, 3.0), 'zero_hi': (0.0, -0.68), 'zero_lo': (0.44, 0.0)}
NOISE = ('signed', 'negative', 'u8', 'wide')
GOLDEN_SHAPES = ((45, 61), (21, 37))
CHAIN_SHAPES = ((40, 52), (24, 31))
CHAIN_WEIGHT = 0.25


def plateau(shape, hi, lo, seed):
    """Columns [0, int(0.4 W)) equal hi, columns [int(0.6 W), W) equal lo, the middle columns
    lo + (hi - lo) (0.98 rand + 0.01): two flat regions that hold the image's extremes."""
    H, W = shape
    a, b = int(0.4 * W), int(0.6 * W)
    img = np.empty(shape)
    img[:, :a] = hi
    img[:, b:] = lo
    img[:, a:b] = lo + (hi - lo) * (0.98 * np.random.RandomState(seed).rand(H, b - a) + 0.01)
    return img


def noise_image(kind, shape, seed):
    """Uniform noise outside [0, 1]: 'signed' 2.5 rand - 1.2, 'negative' -0.1 - rand, 'u8'
    255 rand, 'wide' 1.7 (rand - 0.45) + 0.3."""
    r = np.random.RandomState(seed).rand(*shape)
    if kind == 'signed':
        return 2.5 * r - 1.2
    if kind == 'negative':
        return -0.1 - r
    if kind == 'u8':
        return 255 * r
    assert kind == 'wide'
    return 1.7 * (r - 0.45) + 0.3


def golden_images():
    """{name: image} of the fixture's pyramid inputs."""
    out = {}
    for shape in GOLDEN_SHAPES:
        tag = '%dx%d' % shape
        for name, (hi, lo) in PLATEAUS.items():
            out['plateau_%s_%s' % (name, tag)] = plateau(shape, hi, lo, sum(shape))
        for kind in NOISE:
            out['noise_%s_%s' % (kind, tag)] = noise_image(kind, shape, sum(shape) + 1)
    return out


def chain_inputs():
    """(A, A', B) of the remap chain: A of a narrow range, A' and B of the full one, so the
    remapped A' leaves [0, 1] on both sides (about -0.7 .. 1.7)."""
    rs = np.random.RandomState(4052)
    A = 0.3 + 0.4 * rs.rand(*CHAIN_SHAPES[0])
    Ap = rs.rand(*CHAIN_SHAPES[0])
    B = rs.rand(*CHAIN_SHAPES[1])
    return A, Ap, B


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float64).tobytes()).hexdigest()


def main():
    import warnings
    warnings.filterwarnings('ignore')
    sys.path.insert(0, '/root/reference')
    import img_preprocess as ref_ip        # (reference img_preprocess.py)

    g = {}
    for name, img in golden_images().items():
        pyr = ref_ip.compute_gaussian_pyramid(img, 3)
        assert np.array_equal(pyr[-1], img)
        g[name + '_sha'] = np.array(sha(img))
        g[name + '_n'] = np.array(len(pyr))
        for l, lvl in enumerate(pyr[:-1]):
            g['%s_l%d' % (name, l)] = lvl
    A, Ap, B = chain_inputs()
    g['chain_sha'] = np.array([sha(A), sha(Ap), sha(B)])
    Ar, Apr = ref_ip.remap_luminance(A, [Ap], B)
    Ac, Bc = ref_ip.compress_values(Ar, B, CHAIN_WEIGHT)
    for name, img in (('A', Ac), ('Ap', Apr[0]), ('B', Bc)):
        pyr = ref_ip.compute_gaussian_pyramid(img, 3)
        g['chain_%s_n' % name] = np.array(len(pyr))
        for l, lvl in enumerate(pyr):      # (the finest level is the chain's elementwise result)
            g['chain_%s_l%d' % (name, l)] = lvl
    np.savez_compressed(OUT, **g)
    print('wrote', OUT, 'keys', len(g), 'bytes', os.path.getsize(OUT))


if __name__ == '__main__':
    main()
