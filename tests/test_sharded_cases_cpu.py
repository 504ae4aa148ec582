"""CPU half of the sharded read-out tests: the runs of sharded_cases.py stepped through the oracle.  Everything
tests/test_gpu_sharded_readouts.py relies on to be more than a two-step check is proved here, on any machine: the counts,
the ranks that empty out, the ragged tails, the shrinking gather areas and the link of the group finding.  A change of
seed or field that makes a run vacuous fails here by name.

Two conditions are stated for the partitions that can meet them.  At upload every rank of every world owns bodies, and the
three ranks of the literal run never empty, so "a rank with nothing and a rank with a ragged count at every checkpoint" is
asserted for world 8 at every checkpoint past the upload, and "three sizes of the gather area" for world 3, whose areas
are the larger ones (8 ranks over at most 12 blocks have areas of one or two blocks)."""
import numpy as np
import pytest

import group_cases as gc
import oracle_lib as ol
import sharded_cases as sc

PRECISIONS = [pytest.param(0, id="f32"), pytest.param(1, id="f64")]
RUNS = pytest.mark.parametrize("run", sc.RUNS, ids=sc.RUN_IDS)


def counts_of(nb, run, world, precision=0):
    return {s.step: [cnt for _, cnt in s.ranges(nb, world)] for s in sc.trajectory(*run, precision)}


@RUNS
@pytest.mark.parametrize("precision", PRECISIONS)
def test_counts_are_the_table(run, precision):
    tr = sc.trajectory(*run, precision)
    assert len(tr) == sc.STEPS + 1 and tr[0].n == run[0]
    got = [s.n for s in tr[1:]]
    assert got == sc.COUNTS[run], "%r: the oracle counts %r" % (run, got)
    assert got[-1] < got[0] / 2                                  # below half the count after step 1
    assert [s.n_before for s in tr[1:]] == [run[0]] + got[:-1]
    for s in tr:                                                 # no NaN: plain equality of bits is the right comparison
        assert s.block.dtype == (np.float64 if precision else np.float32) and np.isfinite(s.block).all(), s.step
    assert max(sc.CHECKPOINTS) == sc.STEPS and sc.LAG in sc.CHECKPOINTS and sc.LAG + 1 in sc.CHECKPOINTS


def test_clean_run_goes_on_past_the_checkpoints():
    """The group state file test steps three more: the count still falls there."""
    tr = sc.trajectory(1000, ol.CLEAN, 0, sc.STEPS + 3)
    assert [s.n for s in tr[1:sc.STEPS + 1]] == sc.COUNTS[(1000, ol.CLEAN)] and tr[-1].n < tr[sc.STEPS].n


@pytest.mark.parametrize("key", sorted(sc.OWN), ids=lambda k: "n%d-world%d" % (k[0][0], k[1]))
def test_own_counts_are_the_table(nb, key):
    run, world = key
    for precision in (0, 1):
        got = counts_of(nb, run, world, precision)
        for step, want in sc.OWN[key].items():
            assert got[step] == want, (key, precision, step, got[step])


def test_the_gathering_rank_loses_its_range(nb):
    lit8 = counts_of(nb, (1500, ol.LITERAL), 8)
    assert lit8[0][0] > 0 and all(lit8[s][0] == 0 for s in (4, 8, 12))
    clean3 = counts_of(nb, (1000, ol.CLEAN), 3)
    assert clean3[12][0] == 0
    assert clean3[0][0] > 0 and clean3[0][1] > clean3[0][0]       # not because it started with less than a block


@RUNS
@pytest.mark.parametrize("world", sc.WORLDS)
def test_ranges_tile_and_fit_the_gather_areas(nb, run, world):
    tr = sc.trajectory(*run, 0)
    for s in tr:
        ranges = s.ranges(nb, world)
        assert ranges[0][0] == 0 and ranges[-1][0] + ranges[-1][1] == s.n
        assert all(ranges[r][0] + ranges[r][1] == ranges[r + 1][0] for r in range(world - 1))
        assert all(lo % sc.TILE == 0 for lo, cnt in ranges if cnt)
        # a gather laid out for the exact count, and a slot laid out for the count kLag steps back, hold every own range
        lagged = tr[max(s.step - sc.LAG, 0)].n
        assert max(cnt for _, cnt in ranges) <= sc.own_upper_of(s.n, world) <= sc.own_upper_of(lagged, world)


@RUNS
def test_world_8_has_an_empty_and_a_ragged_rank_at_every_checkpoint_past_the_upload(nb, run):
    own = counts_of(nb, run, 8)
    assert all(c > 0 for c in own[0])
    for step in sc.CHECKPOINTS[1:]:
        assert any(c == 0 for c in own[step]) and any(c % sc.TILE for c in own[step]), (step, own[step])
    moved = {step: tuple(r for r, c in enumerate(own[step]) if c) for step in sc.CHECKPOINTS}
    assert len(set(moved.values())) >= 3, moved                  # the ranges move from rank to rank


def test_own_upper_of():
    assert [sc.own_upper_of(n, 3) for n in (0, 1, 128, 129, 384, 385, 1500)] == [0, 128, 128, 128, 128, 256, 512]
    assert [sc.own_upper_of(n, 8) for n in (1, 1024, 1025, 1500)] == [128, 128, 256, 256]
    assert sc.own_upper_of(4096, 1) == 4096 and sc.own_upper_of(4097, 1) == 4224


@RUNS
def test_the_gather_areas_of_world_3_take_three_sizes(run):
    sizes = {sc.own_upper_of(s.n, 3) for s in sc.trajectory(*run, 0)}
    assert len(sizes) >= 3, sizes
    lagged = {sc.own_upper_of(sc.trajectory(*run, 0)[max(k - sc.LAG, 0)].n, 3) for k in range(sc.STEPS + 1)}
    assert len(lagged) >= 2, lagged                              # and the slots, four steps behind, shrink within the run


@RUNS
@pytest.mark.parametrize("precision", PRECISIONS)
def test_the_centre_link_finds_groups_at_every_checkpoint(run, precision):
    tr = sc.trajectory(*run, precision)
    got = []
    for k in sc.CHECKPOINTS:
        P, _, _, R = ol.carve(tr[k].block, tr[k].n)
        want = gc.model_groups(P.astype(np.float64), R.astype(np.float64), sc.CENTRE_LINK[run], 0.0)
        assert 1 < want["n_groups"] < tr[k].n and want["largest"] > 1, (k, want["n_groups"], tr[k].n)
        got.append(want["n_groups"])
        touching = gc.model_groups(P.astype(np.float64), R.astype(np.float64), 0.0, 1.0)
        assert 1 < touching["n_groups"] <= tr[k].n
    assert got == sc.CENTRE_GROUPS[run], got
