"""The LSH matcher's definition restated in numpy for rows of any length D (a helper module
of test_lsh3_ref.py and test_gpu_lsh3.py, not a conftest).

oracle/ia_oracle.py:LshIndex states the definition for the 55-value luminance rows; the
3-channel matcher (csrc/ia_lsh.hip ia_lsh3_build, csrc/ia_color3.hip k_lsh3_pixel) keeps it
with D = 165.  With D = 55 this restatement equals LshIndex bit for bit (test_lsh3_ref.py).

    centred value  fl32(a_k - c_k)
    projections    L k rows, p in elements 0..D-1, the offset b in element D
    hash           floorf(d / w), d from b through fmaf(p[e], a'[e], d), e = 0..D-1 in order
    key            the wrapped sum over a table's k hashes of mix(h, i), masked to lsh_bits(N)
    tables         per table a stable sort of (key, row)
    query          per table the first `cap` rows of its bucket, an empty bucket the 4 sorted
                   entries around its position; the lexicographic (distance, row) minimum, the
                   distance np.add.reduce((a - q)**2)
"""
import functools

import numpy as np

import ia_oracle as o
from conftest import smooth_noise

LSH_CAP = 32


def fma32(a, b, c):
    """fp32 fused multiply-add: the product of two fp32 values is exact in fp64."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def lsh_bits(N):
    b = 1
    while b < 29 and (1 << b) < N:
        b += 1
    return b + 1


def projections(L, k, w, seed, D):
    """The projections as algorithms.lsh_projections draws them: the normals first, then the
    offsets, from one RandomState(seed); rows padded to a multiple of 4 floats."""
    rs = np.random.RandomState(seed)
    n = L * k
    P = np.zeros((n, (D + 4) // 4 * 4), dtype=np.float32)
    P[:, :D] = rs.standard_normal((n, D))
    P[:, D] = rs.uniform(0.0, w, n)
    return P


def hash_keys(X32, proj, L, k, w, bits):
    """(n, L) uint32 keys of centred fp32 rows X32 (n, D)."""
    n, D = X32.shape
    w = np.float32(w)
    d = np.broadcast_to(proj[:L * k, D][None, :], (n, L * k)).astype(np.float32)
    for e in range(D):
        d = fma32(proj[None, :L * k, e], X32[:, e:e + 1], d)
    h = np.floor(d / w).astype(np.int64) & 0xffffffff
    i = np.arange(L * k, dtype=np.int64) % k
    mix = (h * ((0x9E3779B1 + 2 * i) & 0xffffffff) + 0x7F4A7C15 * i) & 0xffffffff
    keys = mix.reshape(n, L, k).sum(axis=2) & ((1 << bits) - 1)
    return keys.astype(np.uint32)


class LshIndexD:
    """The LSH tables of rows As (N, D) centred by ``center`` (D,).  Counters: ``lookups``
    (query, table) pairs so far, ``empty`` of them that met an empty bucket, ``capped`` that met
    one of more than ``cap`` rows."""

    def __init__(self, As, center, proj, L, k, w, cap=LSH_CAP):
        self.As, self.center, self.proj = As, np.asarray(center, dtype=np.float64), proj
        self.L, self.k, self.w, self.cap = L, k, np.float32(w), cap
        self.bits = lsh_bits(As.shape[0])
        self.keys = hash_keys((As - self.center[None, :]).astype(np.float32), proj, L, k, self.w,
                              self.bits)
        self.order = [np.argsort(self.keys[:, t], kind='stable') for t in range(L)]
        self.sorted_keys = [self.keys[self.order[t], t] for t in range(L)]
        self.lookups = self.empty = self.capped = 0

    def query_keys(self, Q):
        Q = np.atleast_2d(Q)
        return hash_keys((Q - self.center[None, :]).astype(np.float32), self.proj, self.L, self.k,
                         self.w, self.bits)

    def match(self, Q):
        """(idx, dist) of queries Q (M, D) or (D,)."""
        Q = np.atleast_2d(Q)
        N = self.As.shape[0]
        qk = self.query_keys(Q)
        idx = np.empty(len(Q), dtype=np.int64)
        dist = np.empty(len(Q))
        for m in range(len(Q)):
            cand = []
            for t in range(self.L):
                key = int(qk[m, t])
                lo = int(np.searchsorted(self.sorted_keys[t], key, 'left'))
                hi = int(np.searchsorted(self.sorted_keys[t], key + 1, 'left'))
                self.lookups += 1
                if lo == hi:   # empty bucket: neighbouring entries of the sorted table
                    self.empty += 1
                    lo = max(lo - 2, 0)
                    hi = min(lo + 4, N)
                elif hi - lo > self.cap:
                    self.capped += 1
                cand.append(self.order[t][lo:min(hi, lo + self.cap)])
            cand = np.unique(np.concatenate(cand))
            d = np.add.reduce((self.As[cand] - Q[m]) ** 2, axis=1)
            j = np.lexsort((cand, d))[0]
            idx[m], dist[m] = cand[j], d[j]
        return idx, dist

    def pick(self, q):
        """The matcher argument of o.synthesize_level: q -> row."""
        return int(self.match(q)[0][0])


# ---- inputs (as tests/test_gpu_color3.py builds them) ---------------------------------------

def colour(seed, shape):
    return np.dstack([smooth_noise(seed + 17 * ch, shape) for ch in range(3)])


def pyr3(img, cap=None):
    chans = [o.compute_gaussian_pyramid(img[..., ch], 3, cap) for ch in range(3)]
    return [np.dstack([c[l] for c in chans]) for l in range(len(chans[0]))]


def inputs(seed, A_shape, B_shape, n_ap=1, cap=None):
    from scipy.ndimage import gaussian_filter
    A = colour(seed, A_shape)
    Aps = [np.dstack([gaussian_filter(A[..., ch], 1.0 + 0.5 * i) for ch in range(3)])
           for i in range(n_ap)]
    B = colour(seed + 1, B_shape)
    A_pyr, B_pyr = pyr3(A, cap), pyr3(B, cap)
    Ap_list = [pyr3(x, cap) for x in Aps]
    L = min(len(A_pyr), len(B_pyr))
    Bp_pyr = o.initialize_Bp(B_pyr, True, seed + 2)
    return A_pyr, Ap_list, B_pyr, Bp_pyr, L


# the parameter sets (tables, hashes, width, seed) of the synthesis tests: the first meets mostly
# empty buckets, the second mostly buckets of more than LSH_CAP rows
SYNTH_PARAMS = ((8, 3, 1.0, 7), (4, 1, 4.0, 1))
MATCH_PARAMS = ((16, 4, 1.0, 0),) + SYNTH_PARAMS


@functools.lru_cache(maxsize=None)
def case(seed=91, A_shape=(30, 40), B_shape=(28, 33), n_ap=2, twice=False):
    """The tests' inputs, the rows As of every level and the weights: computed once, never
    modified.  twice: the A' pyramid listed twice (every row exists twice: exact ties)."""
    A_pyr, Ap_list, B_pyr, Bp_pyr, L = inputs(seed, A_shape, B_shape, n_ap=n_ap)
    if twice:
        Ap_list = [Ap_list[0], Ap_list[0]]
    return A_pyr, Ap_list, B_pyr, Bp_pyr, L, o.create_index(A_pyr, Ap_list, L), o.compute_weights(3, 5, 12, 3)


def host_tables(A_pyr, Ap_list, As_level, level, tables, hashes, width, seed):
    """A level's LshIndexD with the centre and width of LevelIndex3.build_lsh computed on the
    host (numpy's mean and unbiased variance)."""
    A_lg = A_pyr[level]
    Ap_lg = np.stack([p[level] for p in Ap_list])
    c = np.empty(165)
    c[:102] = A_lg.mean()
    c[102:] = Ap_lg.mean()
    var = (102 * A_lg.var(ddof=1) + 63 * Ap_lg.var(ddof=1)) / 165.0
    w = float(width) * max(np.sqrt(var), 1e-6)     # (the offsets are drawn with the fp64 width)
    return LshIndexD(As_level, c, projections(tables, hashes, w, seed, 165), tables, hashes,
                     np.float32(w))


def oracle_synthesis(case_, kappa, tables_of=None):
    """The oracle's scanline run of every level of case_ (B' on a copy).  tables_of: None (the
    exact matcher) or level -> LshIndexD.  Returns ({level: (s, im, debug)}, B' pyramid,
    {level: LshIndexD})."""
    A_pyr, Ap_list, B_pyr, Bp_pyr, L, As, w = case_
    Bp = [b.copy() for b in Bp_pyr]
    out, used = {}, {}
    for level in range(1, L):
        dbg = {}
        tab = tables_of(level) if tables_of else None
        s, im = o.synthesize_level(level, L, A_pyr, Ap_list, B_pyr, Bp, As[level], w, kappa,
                                   matcher=tab.pick if tab else None, debug=dbg)
        out[level], used[level] = (s, im, dbg), tab
    return out, Bp, used
