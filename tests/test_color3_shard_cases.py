"""The per-shard properties of the sharded 3-channel test cases (colour_shards.CASES), from
the oracle alone (no GPU): which rank holds each query's winner, how many of a shard's 32-row
tiles tie with it, and whether a rank's exact stage must scan every tile (more than C3_CAND =
64 tied tiles).  test_gpu_color3_shards.py runs these cases on the GPU; the assertions here keep
each one exercising the branch it was chosen for."""
import numpy as np
import pytest

import colour_shards as cs

C3_CAND = 64         # ia_color3.hip: candidate tiles (32 rows) held per colour query


def shards(name, world):
    ref = cs.reference(name)
    return ref, [ref.shard(r, world) for r in range(world)]


def test_at2_world2_cross_rank_tie():
    """N = 2,048 over 2 ranks: each shard is one A' image of 32 tiles; the flat queries tie over
    all 32 tiles of BOTH shards (the lowest global row must win across ranks); no full scan."""
    ref, sh = shards('at2', 2)
    assert ref.N == 2048 and ref.nn.size == 16 * 24
    assert [(s[0], s[1], s[2]) for s in sh] == [(0, 1024, 32), (1024, 1024, 32)]
    both = (sh[0][3] == 32) & (sh[1][3] == 32)
    assert both.sum() >= 96, both.sum()
    assert max(s[3].max() for s in sh) <= C3_CAND
    assert [s[4] for s in sh] == [197, 187]


def test_at2_world3_ragged_shards():
    """Three ragged shards, none starting on a tile boundary but the first; the middle one
    straddles the two A' images."""
    ref, sh = shards('at2', 3)
    assert [s[1] for s in sh] == [682, 683, 683]
    assert [s[0] % 32 for s in sh] == [0, 10, 21]
    assert sh[1][0] < 1024 < sh[1][0] + sh[1][1]
    assert [s[4] for s in sh] == [189, 28, 167]
    assert max(s[3].max() for s in sh) <= 22


def test_tie_late_world3():
    """N = 3,120 over 3 ranks: rank 0 is all texture (the flat queries have no tied row there),
    rank 1 holds the winner of the 197 flat queries, rank 2 ties over all its tiles and wins
    nothing."""
    ref, sh = shards('tie_late', 3)
    assert ref.N == 3120
    assert sh[0][1] == 1040 and sh[1][0] % 32 == 16 and sh[2][2] == 33
    flat = (ref.nn >= sh[1][0]) & (ref.nn < sh[1][0] + sh[1][1])     # the queries rank 1 wins
    assert flat.sum() == sh[1][4] == 197
    assert sh[0][3][flat].max() == 0 and sh[0][3].max() == 1
    assert 1 < sh[1][3].max() <= 17
    whole = sh[2][3] == 33                                           # tied over all of rank 2's tiles
    assert whole.sum() >= 100 and flat[whole].all() and sh[2][4] == 0
    assert max(s[3].max() for s in sh) <= C3_CAND
    # rank 2's rows are one flat row 1,040 times: a zero range, so its bound A is 0 and the
    # scale clamp (split16_db_clamped) makes its exact stage scan every tile for every query
    r2 = ref.rows[sh[2][0]:]
    assert (r2 == r2[0]).all()
    assert all(len(np.unique(ref.rows[s[0]:s[0] + s[1]], axis=0)) > 1 for s in sh[:2])


def test_over_world2_full_scans_on_both_ranks():
    """N = 12,960 over 2 ranks of 203 tiles: 360 queries tie over more than C3_CAND tiles on
    both ranks, so each rank publishes after a full scan."""
    ref, sh = shards('over', 2)
    assert ref.N == 12960
    assert [s[2] for s in sh] == [203, 203] and sh[1][0] % 32 == 16
    over = (sh[0][3] > C3_CAND) & (sh[1][3] > C3_CAND)
    assert over.sum() == 360
    assert max(s[3].max() for s in sh) == 198
    assert [s[4] for s in sh] == [736, 284]


@pytest.mark.parametrize('name', sorted(cs.CASES))
def test_winners_cover_every_query(name):
    ref = cs.reference(name)
    for world in cs.CASES[name][1]:
        assert sum(ref.shard(r, world)[4] for r in range(world)) == ref.nn.size


def test_colour_with_lsh_still_raises():
    """synthesize_dev passes comm / rank / nranks on for 3-channel pyramids; the LSH matcher
    stays refused for them, before any device call."""
    import torch
    import image_analogies as ia
    B = [torch.zeros(2, 2, 3), torch.zeros(4, 4, 3)]
    with pytest.raises(NotImplementedError, match='exact matcher'):
        ia.synthesize_dev([], [], B, [], 2, 1.0, None, comm=object(), rank=0, nranks=2, lsh=(4, 8))
