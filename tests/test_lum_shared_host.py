"""Host-side checks of the luminance batch's DB groups: ia_batch_groups (pure pointer
comparison), the shared-screen switch and the partition of a DB group's query tiles into query
groups (ia_diag_shared_screen_groups), db_groups on luminance pyramids, synthesize_batch_dev's
one index per group and level (device calls faked) and the build's resource report of
ia_screen16r.hip.  No device."""
import ctypes
import hashlib
import os
import re

import pytest
import torch

from conftest import ROOT

QG_INTS = 25        # IA_SHARED_QG_INTS (include/ia_diag.h)
MAX_G = 11


def groups_of(fields):
    """ia_batch_groups over jobs whose db / dbi / dbr are the given fake (never dereferenced)
    pointers: (return value, group_of_job)."""
    import _ia
    K = len(fields)
    arr = (_ia.IaSynthArgs * max(K, 1))()
    for a, f in zip(arr, fields):
        a.db, a.dbi, a.dbr = f.get('db', 0), f.get('dbi', 0), f.get('dbr', 0)
    out = (ctypes.c_int * max(K, 1))(*([-1] * max(K, 1)))
    return _ia.lib().ia_batch_groups(arr, K, out), list(out)[:K]


def test_batch_groups_by_pointer():
    assert groups_of([{'dbr': 0x1000 * (k + 1), 'db': 0x50} for k in range(5)]) == (5, [0, 1, 2, 3, 4])
    assert groups_of([{'dbr': 0x1000, 'db': 0x100 * k} for k in range(5)]) == (1, [0] * 5)
    x, y, z = 0x7000, 0x8000, 0x9000
    assert groups_of([{'dbr': p} for p in (x, y, x, y, x, z)]) == (3, [0, 1, 0, 1, 0, 2])
    # a level with the image form only, and one with the rows only
    assert groups_of([{'dbi': p} for p in (x, y, x, y, x, z)]) == (3, [0, 1, 0, 1, 0, 2])
    assert groups_of([{'db': p} for p in (x, y, x, y, x, z)]) == (3, [0, 1, 0, 1, 0, 2])
    # the rotated rows decide where a level has them: equal db under distinct dbr are apart
    assert groups_of([{'dbr': x, 'db': z}, {'dbr': y, 'db': z}]) == (2, [0, 1])
    # jobs without any database never share
    assert groups_of([{}, {}, {}]) == (3, [0, 1, 2])
    assert groups_of([{'dbr': x}]) == (1, [0])
    assert groups_of([{'dbr': x}] * 128) == (1, [0] * 128)
    assert groups_of([{'dbr': x + 64 * k} for k in range(128)]) == (128, list(range(128)))


def test_batch_groups_refuses_bad_arguments():
    import _ia
    lib = _ia.lib()
    arr = (_ia.IaSynthArgs * 129)()
    out = (ctypes.c_int * 129)()
    assert lib.ia_batch_groups(arr, 0, out) == _ia.IA_E_ARG
    assert 'K out of range' in lib.ia_last_error().decode()
    assert lib.ia_batch_groups(arr, -1, out) < 0
    assert lib.ia_batch_groups(arr, 129, out) == _ia.IA_E_ARG
    assert lib.ia_batch_groups(None, 2, out) == _ia.IA_E_ARG
    assert lib.ia_batch_groups(arr, 2, None) == _ia.IA_E_ARG


def test_symbols_declared_and_bound():
    import _ia
    diag = {'ia_diag_set_shared_screen', 'ia_diag_shared_screen_waves', 'ia_diag_shared_screen_groups'}
    assert 'ia_batch_groups' in _ia.declared_symbols()
    assert diag <= set(_ia.declared_symbols('all'))
    assert not diag & set(_ia.declared_symbols())
    assert diag | {'ia_batch_groups'} <= set(_ia._SIGS)
    assert _ia.lib().ia_diag_shared_screen_waves() >= 0


def test_shared_screen_switch_reads_and_sets():
    import _ia
    lib = _ia.lib()
    prev = lib.ia_diag_set_shared_screen(-1)
    assert prev in (0, 1)
    try:
        assert lib.ia_diag_set_shared_screen(0) == prev
        assert lib.ia_diag_set_shared_screen(-1) == 0
        assert lib.ia_diag_set_shared_screen(7) == 0      # other values leave it
        assert lib.ia_diag_set_shared_screen(-2) == 0
        assert lib.ia_diag_set_shared_screen(1) == 0
        assert lib.ia_diag_set_shared_screen(-1) == 1
    finally:
        lib.ia_diag_set_shared_screen(prev)
    assert lib.ia_diag_set_shared_screen(-1) == prev


def query_groups(counts, M):
    """[(DB group, first tile, [(job, tile), ...])] of ia_diag_shared_screen_groups."""
    import _ia
    lib = _ia.lib()
    arr = (ctypes.c_int * len(counts))(*counts)
    n = lib.ia_diag_shared_screen_groups(arr, len(counts), M, None)
    assert n > 0
    out = (ctypes.c_int * (n * QG_INTS))(*([-9] * (n * QG_INTS)))
    assert lib.ia_diag_shared_screen_groups(arr, len(counts), M, out) == n
    res = []
    for i in range(n):
        o = out[i * QG_INTS:(i + 1) * QG_INTS]
        g, first, cnt = o[:3]
        assert 1 <= cnt <= MAX_G
        assert all(v == -1 for v in o[3 + 2 * cnt:])      # spare slots
        res.append((g, first, [(o[3 + 2 * t], o[4 + 2 * t]) for t in range(cnt)]))
    return res


def check_partition(counts, M):
    T = (M + 31) // 32
    qgs = query_groups(counts, M)
    assert [g for g, _, _ in qgs] == sorted(g for g, _, _ in qgs)       # launch order: group order
    for g, n in enumerate(counts):
        mine = [(first, tiles) for gg, first, tiles in qgs if gg == g]
        assert len(mine) == -(-n * T // MAX_G)
        flat = [jt for _, tiles in mine for jt in tiles]
        # every (job, tile) exactly once, in (job, tile) order
        assert flat == [(j, t) for j in range(n) for t in range(T)], (counts, M, g)
        sizes = [len(tiles) for _, tiles in mine]
        assert max(sizes) <= MAX_G and max(sizes) - min(sizes) <= 1, (counts, M, sizes)
        pos = 0
        for first, tiles in mine:
            assert first == pos
            pos += len(tiles)


@pytest.mark.parametrize('M', [1, 32, 33, 34, 64, 172, 342])
def test_query_groups_partition_the_tile_list(M):
    for n in range(1, 25):
        check_partition([n], M)
    for counts in ([3, 2, 1], [1, 1, 7], [12, 1], [1] * 6, [24, 5, 24], [2, 9]):
        check_partition(counts, M)


def test_query_groups_of_the_device_cases():
    """The partitions the GPU tests rely on: 7 jobs x 2 tiles = two groups of 7, the first ending
    with job 3's first tile; 12 jobs x 1 tile = two groups of 6."""
    a = query_groups([7], 34)
    assert [len(t) for _, _, t in a] == [7, 7]
    assert a[0][2][-1] == (3, 0) and a[1][2][0] == (3, 1)
    b = query_groups([12], 30)
    assert [len(t) for _, _, t in b] == [6, 6]


def test_query_groups_refuse_bad_arguments():
    import _ia
    lib = _ia.lib()
    one = (ctypes.c_int * 2)(3, 0)
    assert lib.ia_diag_shared_screen_groups(None, 1, 32, None) == _ia.IA_E_ARG
    assert lib.ia_diag_shared_screen_groups(one, 0, 32, None) == _ia.IA_E_ARG
    assert lib.ia_diag_shared_screen_groups(one, 1, 0, None) == _ia.IA_E_ARG
    assert lib.ia_diag_shared_screen_groups(one, 2, 32, None) == _ia.IA_E_ARG     # an empty group
    big = (ctypes.c_int * 2)(100, 29)
    assert lib.ia_diag_shared_screen_groups(big, 2, 32, None) == _ia.IA_E_ARG     # 129 jobs


def lum_job(A=None):
    """CPU luminance pyramids (3 levels); A: (A_pyr, Ap_list) to share, else fresh ones."""
    shapes = [(5, 6), (10, 12), (20, 24)]
    mk = lambda: [torch.zeros(s, dtype=torch.float64) for s in shapes]  # noqa: E731
    A_pyr, Ap_list = A if A is not None else (mk(), [mk()])
    return A_pyr, Ap_list, mk(), mk()


def test_db_groups_identity_not_equality():
    import image_analogies as ia
    x, y = lum_job(), lum_job()         # equal contents, tensors of their own
    jobs = [x, lum_job(x[:2]), y, lum_job(x[:2]), lum_job(y[:2])]
    assert ia.db_groups(jobs) == [0, 0, 1, 0, 1]
    # the same A with another A' list, and with an A' more, are groups of their own
    other_ap = (x[0], [[t.clone() for t in x[1][0]]])
    two_ap = (x[0], [x[1][0], x[1][0]])
    assert ia.db_groups([x, lum_job(other_ap), lum_job(two_ap)]) == [0, 1, 2]


class FakeIndex:
    """What _LevelCall reads of an algorithms.LevelIndex, over CPU tensors."""

    def __init__(self, level, nrows):
        import _ia
        self.level = level
        self.src = _ia.IaSrcLevel()
        self.row0, self.nrows, self.N = 0, nrows, nrows
        self.db = torch.zeros(16, dtype=torch.uint8)
        self.dbr = torch.zeros(16, dtype=torch.uint8)
        self.rot = torch.zeros(16, dtype=torch.float32)
        self.dbk = None
        self.center = torch.zeros(56, dtype=torch.float64)
        self.amax = torch.zeros(2, dtype=torch.float32)

    def dbi_ptr(self):
        return None

    def lsh_ptr(self):
        return None


class FakeLib:
    def __init__(self):
        self.log = []
        self.target = 512

    def ia_synth_workspace_bytes(self, H, W, nrows, nranks):
        return 256

    def ia_set_chunk_target(self, t):
        self.log.append(('target', t))
        prev, self.target = self.target, t
        return prev

    def ia_synth_levels_batch(self, arr, n, K, st):
        self.log.append(('batch', n, K, self.target))
        self.args = [(a.db, a.dbr, a.rot, a.center, a.amax, a.workspace, a.s, a.Bp_lg, a.kappa_factor, a.tag)
                     for a in arr]
        return 0

    def ia_synth_status(self, arr, n, st):
        self.log.append(('status', n))
        return 0


@pytest.fixture
def faked(monkeypatch):
    """synthesize_batch_dev with algorithms.level_index and every library call faked: yields
    (library log, list of the (A' data_ptr, level) of each index built)."""
    import _ia
    import algorithms
    fake, built = FakeLib(), []

    def level_index(A_pyr, Ap_list, level, row_range=None, lsh=None, **kw):
        built.append((Ap_list[0][-1].data_ptr(), level))
        return FakeIndex(level, Ap_list[0][level].numel())
    monkeypatch.setattr(algorithms, 'level_index', level_index)
    monkeypatch.setattr(_ia, 'lib', lambda: fake)
    monkeypatch.setattr(_ia, 'stream', lambda: None)
    monkeypatch.setattr(_ia, 'workspace', lambda n: torch.empty(max(int(n), 256), dtype=torch.uint8))
    monkeypatch.delenv('IA_BATCH_CHUNKS', raising=False)
    return fake, built


def test_batch_builds_one_index_per_group_and_level(faked):
    import image_analogies as ia
    fake, built = faked
    x, y = lum_job(), lum_job()
    jobs = [x, y, lum_job(x[:2]), lum_job(y[:2]), lum_job(x[:2]), lum_job()]      # X Y X Y X Z
    group = [0, 1, 0, 1, 0, 2]
    assert ia.db_groups(jobs) == group
    w = torch.zeros(55, dtype=torch.float64)
    outs = ia.synthesize_batch_dev(jobs, 3, [0.5, 1.0, 2.0, 3.0, 4.0, 5.0], w)
    assert len(outs) == 6 and all(sorted(o) == [1, 2] for o in outs)
    key = lambda j: j[1][0][-1].data_ptr()  # noqa: E731
    # one index per group and level, at the group's first job, in job order
    assert built == [(key(jobs[q]), level) for level in (1, 2) for q in (0, 1, 5)]
    K = 6
    assert fake.log == [('target', max(64, 512 // K)), ('batch', 2, K, max(64, 512 // K)), ('status', 2 * K),
                        ('target', 512)]
    for j in range(2):
        rows = fake.args[j * K:(j + 1) * K]
        for q in range(K):
            for p in range(q):
                same = rows[q][:5] == rows[p][:5]       # db, dbr, rot, center, amax
                assert same == (group[q] == group[p]), (j, p, q)
                assert rows[q][5:8] != rows[p][5:8]     # workspace, s, B' stay per job
        assert [r[9] for r in rows] == [j + 1] * K
    assert len({r[8] for r in fake.args[K:]}) == K      # each job's own kappa


def test_batch_of_distinct_pyramids_builds_as_before(faked):
    import image_analogies as ia
    fake, built = faked
    jobs = [lum_job() for _ in range(4)]
    assert ia.db_groups(jobs) == [0, 1, 2, 3]
    ia.synthesize_batch_dev(jobs, 3, 1.0, torch.zeros(55, dtype=torch.float64))
    key = lambda j: j[1][0][-1].data_ptr()  # noqa: E731
    assert built == [(key(j), level) for level in (1, 2) for j in jobs]     # K (L - 1), today's order
    assert fake.log[0] == ('target', 128) and fake.log[-1] == ('target', 512)
    assert len({a[0] for a in fake.args}) == 8 and len({a[1] for a in fake.args}) == 8


# (VGPRs, TotalSGPRs, LDS bytes) of k_screen16r<1..11> in the parent commit's report
PARENT_R16 = {1: (52, 68, 33024), 2: (59, 70, 33280), 3: (68, 68, 33536), 4: (68, 70, 33792),
              5: (75, 72, 34048), 6: (75, 72, 34304), 7: (84, 72, 34560), 8: (86, 70, 34816),
              9: (95, 70, 35072), 10: (94, 70, 35328), 11: (102, 70, 35584)}


def kernel_resources():
    """{(kernel, G): {figure: value}} of the templated screens in the build's report of
    ia_screen16r.hip."""
    csrc = os.path.join(ROOT, 'image-analogies-python_amd', 'csrc')
    path = os.path.join(csrc, '_build', 'ia_screen16r.res')
    assert os.path.exists(path), 'no resource report: build with make -C image-analogies-python_amd/csrc'
    text = open(path).read()
    m = re.search(r'source-sha1: ([0-9a-f]{40})', text)
    src = open(os.path.join(csrc, 'ia_screen16r.hip'), 'rb').read()
    assert m and hashlib.sha1(src).hexdigest() == m.group(1), 'resource report older than ia_screen16r.hip'
    out, name = {}, None
    for line in text.splitlines():
        m = re.search(r'Function Name: (\S+)', line)
        if m:
            m = re.match(r'_ZN2ia\d+_GLOBAL__N_1\d+(k_screen16[a-z]+)ILi(\d+)E', m.group(1))
            name = (m.group(1), int(m.group(2))) if m else None
            if name:
                out[name] = {}
            continue
        m = re.search(r'remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)', line)
        if m and name:
            out[name].setdefault(m.group(1), int(m.group(2)))
    return out


def test_screen_resources():
    """Every k_screen16rs instance: no scratch, no spills, the occupancy 4 of its launch bounds,
    at most 40,960 B of LDS; k_screen16r<1..11> keep the parent's VGPRs, SGPRs and LDS."""
    res = kernel_resources()
    for G in range(1, 12):
        rs = res[('k_screen16rs', G)]
        assert rs['ScratchSize'] == 0 and rs['VGPRs Spill'] == 0 and rs['SGPRs Spill'] == 0, (G, rs)
        assert rs['Occupancy'] >= 4 and rs['LDS Size'] <= 40960, (G, rs)
        r = res[('k_screen16r', G)]
        assert (r['VGPRs'], r['TotalSGPRs'], r['LDS Size']) == PARENT_R16[G], (G, r)
        assert r['ScratchSize'] == 0 and r['Occupancy'] >= 4, (G, r)
