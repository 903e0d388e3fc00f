"""The path a multi-GPU run takes (xw_wave with a->comm set: the sharded screen, k_xwave /
k_xstrip with px.nranks > 0, the (distance, row) merge of the ranks' records in ia_finish.h)
on the inputs the one-GPU suite runs the exact stage on: label maps whose flat rows tie
across the ranks' shards (the winner on rank 0, or on rank 1 with no tied row on rank 0), a
candidate list that overflows per shard, strip-form shards with row0 > 0 that straddle two A'
images (under the R16 and the split-f16 screen), padded row-form shards, image-form shards in
linear order, constant / near-constant / huge A with one amax per rank, the unfused form
(IA_XWAVE=0: k_peer_finish) and the default shard policy.  2 and 3 rank processes share
the box's GPU (tests/exchange_worker.py --cases); five launches in all, each running its cases
one after the other.  Every rank's B', s, im and approximate picks equal the oracle's bit for
bit, the exchange stayed device-side, the levels are sharded as the launch says and in the
form named here, and each rank's profile counters reach the floors the oracle alone gives for
its shard (shard_ties).  The inputs' own preconditions run on the CPU in test_oracle.py."""
import os
import time

import numpy as np
import pytest

import test_gpu_fallback as fb

pytestmark = pytest.mark.gpu

SEGCAP = fb.SEGCAP
B_SHAPE = (16, 48)

# name -> (the case it reuses (one of these, or a lum_case of test_gpu_fallback.py) or None, the
# case's own environment)
CASES = {
    'tie2@small': (None, {}),
    'tie_late@small': (None, {}),
    'straddle@strip': (None, {'IA_ROT_MIN_ROWS': '1'}),
    'over@shards': (None, {}),
    'padded@shards': ('padded', {}),
    'const_exact@small': ('const_exact@small', {}),
    'near@small': ('near@small', {}),
    'huge@small': ('huge@small', {}),
    'near@strip': ('near@strip', {'IA_ROT_MIN_ROWS': '1'}),
    # beyond the forms above: the split-f16 screen (no R16) over the straddling strip shards, and
    # image-form shards in linear order (whole chunks, but half a scanline each: row0 % Aw != 0)
    'straddle@split16': ('straddle@strip', {'IA_DB_ROT': '0'}),
    'linear@image': (None, {}),
}
TIE_CASES = ('tie2@small', 'tie_late@small', 'straddle@strip', 'over@shards', 'padded@shards',
             'straddle@split16', 'linear@image')

# the finest level's form per case, as the ranks must report it: (strip order, image form, R16).
# (A padded shard has no image form, ia_internal.h img_db_applies: padded@shards is row form.)
FORMS = {
    'tie2@small': (False, False, False), 'tie_late@small': (False, False, False),
    'straddle@strip': (True, True, True), 'over@shards': (True, True, True),
    'padded@shards': (False, False, False), 'const_exact@small': (False, False, False),
    'near@small': (False, False, False), 'huge@small': (False, False, False),
    'near@strip': (True, True, True), 'straddle@split16': (True, True, False),
    'linear@image': (False, True, False),
}

# world, pipelined, environment on top of run_ranks' (None: unset, the product's 2^19 rows),
# cases, each rank's time limit (s).  Measured on an MI355X, launch start to the last rank's
# exit: w2 3.9-5.6 s, w3 3.7-4.0 s, policy 3.2-3.6 s, w3over 3.3-4.2 s, unfused 2.9-3.0 s, nearly
# all of it process start-up (a rank's slowest case takes 0.9 s); the first launch of a run pays
# a cold start (the 5.6 s), and any launch can be first under -k.  The two over@shards launches
# get about three times that; the small ones keep run_ranks' 100 s.
LAUNCHES = {
    'w2': (2, 1, {}, ('tie2@small', 'padded@shards', 'near@strip', 'linear@image'), 100),
    'w3': (3, 0, {}, ('tie2@small', 'tie_late@small', 'straddle@strip', 'const_exact@small', 'near@small',
                      'huge@small', 'straddle@split16'), 100),
    'policy': (2, 1, {'IA_SHARD_MIN_ROWS': None}, ('over@shards',), 20),
    'w3over': (3, 0, {}, ('over@shards',), 20),
    'unfused': (2, 1, {'IA_XWAVE': '0'}, ('tie2@small', 'tie_late@small'), 100),
}


def _alias(name):
    """The case of this table whose inputs and oracle run `name` shares, or None."""
    reuse = CASES[name][0]
    return reuse if reuse in CASES and reuse != name else None


def shard_spec(name):
    """(LumCase arguments, the case's environment) of a named case; the rank processes build
    their pyramids from the same call."""
    reuse, env = CASES[name]
    if reuse:
        return (shard_spec(reuse)[0] if _alias(name) else fb.lum_spec(reuse)), env
    label = fb.label_inputs
    if name == 'tie2@small':      # flat rows bit-identical in image 0 and image 1
        images, seed = label(101, (40, 52), B_SHAPE, n_ap=2, patch=16, same_bg=True), 101
    elif name == 'tie_late@small':  # 3 ranks: scanlines 0-19 all texture, the lowest flat row on rank 1
        images, seed = label(102, (60, 52), B_SHAPE, n_ap=1, band=24), 102
    elif name == 'linear@image':    # 2 ranks: 16,896 rows = 16.5 scanlines each, flat rows on both
        images, seed = label(105, (33, 1024), B_SHAPE, n_ap=1, patch=16), 105
    elif name == 'straddle@strip':  # 3 ranks: the middle shard = image 0 lines 128-191 + image 1 lines 0-63
        images, seed = label(103, (192, 256), B_SHAPE, n_ap=2, patch=64, same_bg=True), 103
    else:
        assert name == 'over@shards'    # 2 ranks: 1152 segments each; 3 ranks: 768, a straddling shard
        images, seed = label(104, (768, 768), B_SHAPE, n_ap=2, band=10, patch=96, same_bg=True), 104
    return dict(images=images, cap=2, k=1.0, seed=seed), env


def shard_case(name):
    """The case with its oracle run, once per process (shared with test_gpu_fallback's cases)."""
    reuse = CASES[name][0]
    if reuse:
        return shard_case(reuse) if _alias(name) else fb.lum_case(reuse)
    if 'shards:' + name not in fb._CASES:
        fb._CASES['shards:' + name] = fb.LumCase(**shard_spec(name)[0])
    return fb._CASES['shards:' + name]


def shard_rows(N, rank, world):
    return N * rank // world, N * (rank + 1) // world - N * rank // world


_TIES = {}


def shard_ties(name, rank, world, keep=None):
    """(ties, segments): per finest-level query the segments of rank's shard, in the shard's own
    segment order, holding a row bit-identical to the query's nearest row of the whole level (0:
    the shard holds no copy).  From the oracle and the host geometry alone.  keep(first global
    row of each segment) -> mask: count those segments only."""
    case = shard_case(name)
    name = _alias(name) or name
    if (name, rank, world) not in _TIES or keep is not None:
        A_lg = case.pyr[0][case.L - 1]
        N = len(case.rows)
        row0, nrows = shard_rows(N, rank, world)
        order, seg = fb.segment_order(N, A_lg.shape[0], A_lg.shape[1], row0, nrows)
        if keep is not None:
            sel = np.repeat(keep(row0 + order[::seg]), seg)
            return fb.tie_segments(case.rows[row0:row0 + nrows], case.nn, order[sel], seg, pool=case.rows)
        _TIES[name, rank, world] = (fb.tie_segments(case.rows[row0:row0 + nrows], case.nn, order, seg,
                                                    pool=case.rows), len(order) // seg)
    return _TIES[name, rank, world]


# ---- the launches ----------------------------------------------------------------------------

def run_launch(key, out_dir):
    """The launch's rank processes, once: {(case, rank): the rank's file}; prints the wall time
    and each rank's seconds per case."""
    from test_gpu_exchange import run_ranks
    world, pipe, env, cases, limit = LAUNCHES[key]
    t0 = time.time()
    outs = run_ranks(world, ['--cases', out_dir, pipe] + list(cases), timeout=limit, env=env)
    wall = time.time() - t0
    print('launch %s: world %d, %d cases, wall %.1f s' % (key, world, len(cases), wall))
    for txt in outs:
        print(''.join(line + '\n' for line in txt.splitlines() if line.startswith('rank ')), end='')
    return {(c, r): dict(np.load(os.path.join(out_dir, 'rank%d_%s.npz' % (r, c))))
            for c in cases for r in range(world)}


def _launch(key):
    @pytest.fixture(scope='module', name='launch_' + key)
    def fixture(gpu, tmp_path_factory):
        return run_launch(key, str(tmp_path_factory.mktemp('shards_' + key)))
    return fixture


launch_w2, launch_w3, launch_policy = _launch('w2'), _launch('w3'), _launch('policy')
launch_w3over, launch_unfused = _launch('w3over'), _launch('unfused')


def check(files, key, name):
    """Every rank's file of one case against the oracle (module docstring)."""
    world, _, env, _, _ = LAUNCHES[key]
    case = shard_case(name)
    A_pyr, Ap_list = case.pyr[0], case.pyr[1]
    min_rows = 0 if env.get('IA_SHARD_MIN_ROWS', '0') == '0' else 1 << 19
    fin = case.L - 1
    strip, image, r16 = FORMS[name]
    forced = name.split('@')[0] if name.split('@')[0] in fb.FORCED else None
    for r in range(world):
        got = files[name, r]
        assert str(got['exchange_kind']) == 'peer', r
        assert int(got['xwave']) == int(env.get('IA_XWAVE', 2)), r
        levels = sorted(case.ref)
        fb.assert_case(case, {l: (got['s%d' % l], got['im%d' % l], (got['dbgpx%d' % l], got['dbgd%d' % l]))
                              for l in levels}, {l: got['bp%d' % l] for l in levels})
        for l in levels:
            Ah, Aw = A_pyr[l].shape
            N = len(Ap_list) * Ah * Aw
            assert bool(got['sharded%d' % l]) == (N >= min_rows), (r, l)
            want = shard_rows(N, r, world) if N >= min_rows else (0, N)
            assert tuple(got['shard%d' % l]) == want, (r, l)
            prof = dict(zip(('full_scans', 'candidate_segments', 'rows_rescored', 'jobs'), got['prof%d' % l]))
            assert prof['jobs'] == 1
            if forced:
                fb.assert_forced(case, forced, prof, l)
        # the finest level's form, from what the rank reports
        db, dbi, dbr = (bool(x) for x in got['forms%d' % fin])
        smap = got['stage_map%d' % fin]
        Aw = A_pyr[fin].shape[1]
        ints = lambda a: tuple(int(x) for x in a)  # noqa: E731
        print('%s [%s] rank %d: shard %s, stage map %s, db %d dbi %d dbr %d, full_scans %d, candidate '
              'segments %d' % (name, key, r, ints(got['shard%d' % fin]), ints(smap), db, dbi, dbr,
                               got['prof%d' % fin][0], got['prof%d' % fin][1]))
        assert smap[0] == (Aw if strip else 0), (r, smap)
        assert dbi == image and db == (not image) and dbr == r16, (r, db, dbi, dbr)
        if name in TIE_CASES:
            ties, nseg = shard_ties(name, r, world)
            full, cand = int(got['prof%d' % fin][0]), int(got['prof%d' % fin][1])
            over = int((ties > SEGCAP).sum())
            print('%s [%s] rank %d: %d segments, oracle floors: candidate segments %d, queries tied over > %d '
                  'segments %d (most %d)' % (name, key, r, nseg, ties.sum(), SEGCAP, over, ties.max()))
            assert cand >= int(ties.sum()), r
            if ties.max() <= SEGCAP:
                assert full == 0, r
            else:
                assert full >= over, r


@pytest.mark.parametrize('name', LAUNCHES['w2'][3])
def test_two_ranks_pipelined_vs_oracle(launch_w2, name):
    """World 2, every level sharded, pipelined: tie2@small (the shard boundary is the image
    boundary; every flat query's tied rows lie on both ranks, the winner on rank 0),
    padded@shards (78,336 rows per rank in 306 chunks padded to 308: the padding of each shard
    repeats a tied row), near@strip (strip-form R16 shards of 65,536 rows, every query
    full-scans under the exchange), linear@image (image-form shards in linear chunk order, the
    second starting in the middle of a scanline)."""
    check(launch_w2, 'w2', name)


@pytest.mark.parametrize('name', LAUNCHES['w3'][3])
def test_three_ranks_level_by_level_vs_oracle(launch_w3, name):
    """World 3, every level sharded, one level at a time: ragged row-form shards (tie2@small,
    the degenerate kinds with one amax per rank), the winner on rank 1 while rank 0 holds no
    tied row and rank 2's rows are all identical (tie_late@small), a strip-form R16 shard with
    row0 > 0 that straddles the two A' images (straddle@strip; straddle@split16: the same under
    the split-f16 screen, IA_DB_ROT=0)."""
    check(launch_w3, 'w3', name)


def test_default_shard_policy_full_scans_on_both_ranks(launch_policy):
    """World 2 under the product's IA_SHARD_MIN_ROWS (2^19), pipelined: over@shards' level 1
    (294,912 rows) runs replicated, its finest level sharded into 589,824 rows = 1152 segments
    per rank: flat queries overflow the candidate list on both ranks, each scans its shard,
    publishes, and the ranks tie with each other."""
    got = launch_policy['over@shards', 0]
    assert not bool(got['sharded1']) and bool(got['sharded2'])
    for r in range(2):
        ties, nseg = shard_ties('over@shards', r, 2)
        assert nseg == 1152 and int((ties > SEGCAP).sum()) >= 100
    check(launch_policy, 'policy', 'over@shards')


def test_three_ranks_straddling_strip_shard_below_the_cap(launch_w3over):
    """World 3, over@shards one level at a time: 393,216 rows = 768 segments per rank, the
    middle shard image 0 lines 512-767 + image 1 lines 0-255; no rank scans."""
    for r in range(3):
        ties, nseg = shard_ties('over@shards', r, 3)
        assert nseg == 768 and ties.max() <= SEGCAP
    check(launch_w3over, 'w3over', 'over@shards')


@pytest.mark.parametrize('name', LAUNCHES['unfused'][3])
def test_two_ranks_unfused_exchange_vs_oracle(launch_unfused, name):
    """World 2 with IA_XWAVE=0 (launch_match publishes, k_peer_finish collects and merges):
    the cross-rank ties of tie2@small (the winner on rank 0) and tie_late@small."""
    check(launch_unfused, 'unfused', name)
