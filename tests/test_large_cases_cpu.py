"""CPU tests of the large-N states and references (tests/large_cases.py): what tests/test_gpu_large_queries.py relies on.

The thresholds of the size, the encounter classes, the giant component and the small groups of state A; no NaN or inf where a
window reference forbids it; every entry of large_cases.builders equal to its full n x n model on a 1500-body state of the same
generator with planted clusters; every cached reference of state A inside the budget of 10 s.

Measured (seconds, from test_references_within_budget's print; the whole file takes 18 s):
    pairs16 0.5   pairs256 0.6   pairs_below 0.4   pairs_points 0.6   touching 0.0   centres 0.7   enc_0 0.1   enc_dt 0.3
    enc_h 0.7   neighbors 1.3   knn32 5.5   neighbors_points 0.8   knn32_points 4.1
The stepped state B of the GPU file (the stock configuration of 100 003 bodies in a field of 300 000) holds 97 107, 97 008 and
96 819 bodies after its first three steps on the CPU oracle (7 s a step: not repeated here; the GPU test asserts the counts)."""
import numpy as np
import pytest

import encounter_cases as ec
import group_cases as gc
import knn_cases as kc
import large_cases as lg
import neighbor_cases as nc
import pair_cases as pc


# ---------------------------------------------------------------------------------------------------------------------
# 1. the size
# ---------------------------------------------------------------------------------------------------------------------
def test_thresholds_of_the_size():
    n = lg.N
    assert n > 92683 > 65536 and lg.PAIRS == 5000250003 > 2 ** 32
    assert 92683 * 92682 // 2 == 4295022903 > 2 ** 32 > 92682 * 92681 // 2     # the first size whose pair total passes 2^32
    assert 65537 * 65536 // 2 > 2 ** 31 > 65536 * 65535 // 2
    tiles = -(-n // lg.TILE)
    assert (tiles, n - (tiles - 1) * lg.TILE) == (782, 35)
    groups = -(-n // lg.WG)
    last = n - (groups - 1) * lg.WG
    assert (groups, last) == (391, 163) and groups > 256           # more workgroups than the chip has CUs
    assert divmod(last, lg.WAVE) == (2, 35) and lg.WG // lg.WAVE == 4   # two full waves, one of 35 rows, one with none
    assert lg.MANY == 70001 > 2 ** 16 and lg.MANY % lg.WAVE != 0 and lg.SMALL_N == lg.FEW == 300
    assert np.float64(np.float32(lg.DT)) == lg.DT                  # the fp32 and the fp64 context have one time step


def test_sampled_rows():
    rows, knn_rows = lg.rows_a()
    for r in (rows, knn_rows):
        assert (np.diff(r) > 0).all() and r[0] == 0 and r[-1] == lg.N - 1
        for want in (np.arange(130), np.arange(lg.N - 130, lg.N), np.arange(65530, 65546), [255, 256, 65279, 65280, 99839, 99840]):
            assert np.isin(want, r).all()
    assert np.isin(knn_rows, rows).all() and 300 < len(knn_rows) < 450 and 550 < len(rows) < 650
    assert not rows.flags.writeable and not lg.state_a()[0].flags.writeable


# ---------------------------------------------------------------------------------------------------------------------
# 2. state A
# ---------------------------------------------------------------------------------------------------------------------
def test_state_a_is_what_the_window_references_need():
    P, V, M, R = lg.state_a()
    assert P.shape == V.shape == (lg.N, 2) and R.shape == M.shape == (lg.N,)
    for a in (P, V, M, R):
        assert np.isfinite(a).all() and np.array_equal(a.astype(np.float32).astype(np.float64), a)
    assert np.abs(V).max() <= lg.VMAX and 0 <= R.min() and R.max() < 1.5
    assert P.min() >= 0 and P.max() <= lg.field_of(lg.N) + 2.0
    # the index order is unrelated to the geometry: neither coordinate is correlated with the index
    idx = np.arange(lg.N)
    assert abs(np.corrcoef(idx, P[:, 0])[0, 1]) < 0.02 and abs(np.corrcoef(idx, P[:, 1])[0, 1]) < 0.02
    pts = lg.points_a()
    assert pts.shape == (lg.FEW, 2) and np.isfinite(pts).all()


def test_state_a_has_every_encounter_class():
    enc, info = lg.reference("enc_h")
    now, end_only, missed = ec.classes(enc)
    print("state A at h = %g: pairs %d, now %d, end without now %d, missed %d" % (lg.H, info["pairs"], now, end_only, missed))
    assert info["pairs"] >= 1000 and min(now, end_only, missed) >= 100
    assert info["horizon"] == lg.H and info["n_bodies"] == lg.N
    far = np.abs(enc["i"].astype(np.int64) - enc["j"]) >= lg.WG    # the two bodies of a pair sit in different workgroups
    assert far.mean() > 0.9 and (enc["j"] > 65536).sum() >= 100 and (enc["i"] > 65536).sum() >= 100
    enc0, info0 = lg.reference("enc_0")
    assert info0["pairs"] == info0["now"] == info0["end"] == now and info0["missed"] == 0
    encd, infod = lg.reference("enc_dt")
    assert info0["pairs"] < infod["pairs"] < info["pairs"] and min(ec.classes(encd)) >= 10


def test_state_a_has_the_giant_component_and_the_small_groups():
    touching, centres = lg.reference("touching"), lg.reference("centres")
    print("touching: %d groups, largest %d, %d links; centres at %.1f: %d groups, largest %d, %d links"
          % (touching["n_groups"], touching["largest"], touching["links"], lg.CENTRE_LINK, centres["n_groups"],
             centres["largest"], centres["links"]))
    sizes = np.bincount(touching["label"])
    assert 2 <= touching["largest"] <= 8 and (sizes >= 2).sum() >= 500 and (sizes >= 3).sum() >= 100   # small and many
    assert centres["largest"] >= lg.N // 2 + 1 and centres["n_groups"] - 1 >= 100
    giant = np.flatnonzero(centres["label"] == np.argmax(np.bincount(centres["label"])))
    assert len(np.unique(giant // lg.WG)) == -(-lg.N // lg.WG)     # the one component has bodies in every workgroup


def test_state_a_fills_the_histograms():
    r16, r256, below, at = (lg.reference(k) for k in ("pairs16", "pairs256", "pairs_below", "pairs_points"))
    for r in (r16, r256, below):
        pc.check_sum(r, lg.PAIRS)
        assert r["rest"] > 2 ** 32                                 # the derived field is the one above 2^32
    assert r16["below"] == 0 and (r16["counts"] > 0).all() and np.count_nonzero(r256["counts"]) > 200
    assert below["below"] >= 1000 and (below["counts"] > 0).all()
    pc.check_sum(at, lg.FEW * lg.N)
    assert at["below"] > 0 and (at["counts"] > 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# 3. every reference equals its full model on 1500 bodies of the same generator
# ---------------------------------------------------------------------------------------------------------------------
def test_references_equal_the_full_models_on_1500_bodies():
    n = 1500
    P, V, M, R = lg.make_state(n, per_kind=20, seed=1500)
    rows, knn_rows = lg.sample_rows(n, random=60)
    assert rows[0] == 0 and rows[-1] == n - 1 and np.isin([255, 256, 1279, 1280], rows).all() and len(knn_rows) < len(rows) < n
    pts = lg.points_over(P, 70, lg.field_of(n), seed=3)
    got = {name: build() for name, build in lg.builders(P, V, R, rows, knn_rows, pts).items()}
    assert tuple(got) == lg.NAMES
    for name, e2 in (("pairs16", lg.E2_16), ("pairs256", lg.E2_256), ("pairs_below", lg.E2_BELOW)):
        pc.assert_same(got[name], pc.model_pair_counts(P, e2), name)
        assert got[name]["counts"].sum() > 0
    assert got["pairs_below"]["below"] >= 20
    pc.assert_same(got["pairs_points"], pc.model_pair_counts(P, lg.E2_BELOW, pts), "pairs_points")
    for name, link, scale in (("touching", 0.0, 1.0), ("centres", lg.CENTRE_LINK, 0.0)):
        gc.assert_same(got[name], gc.model_groups(P, R, link, scale), name)
    assert (np.bincount(got["touching"]["label"]) >= 2).sum() >= 20 and got["centres"]["largest"] >= n // 2
    for name, h in (("enc_0", 0.0), ("enc_dt", lg.DT), ("enc_h", lg.H)):
        ec.assert_same(got[name], ec.model_encounters(P, V, R, h), name)
    assert min(ec.classes(got["enc_h"][0])) >= 15                  # the planted clusters are in the subsample
    nc.assert_same(got["neighbors"], nc.model_neighbors(P, R)[rows], "neighbors")
    nc.assert_same(got["neighbors_points"], nc.model_neighbors(P, R, points=pts), "neighbors_points")
    full = kc.model_knn(P, 32)
    kc.assert_same(got["knn32"], kc.sliced(full, knn_rows), "knn32")
    kc.assert_same(got["knn32_points"], kc.model_knn(P, 32, points=pts), "knn32_points")
    for k in (1, 8, 32):                                           # the prefix the GPU file takes for k = 1 and 8
        kc.assert_same(lg.knn_prefix(got["knn32"], k), kc.model_knn(P, k, rows=knn_rows), "prefix %d" % k)
        kc.assert_same(lg.knn_prefix(got["knn32_points"], k), kc.model_knn(P, k, points=pts), "prefix %d, points" % k)


def test_many_points():
    pts, sample = lg.many_points()
    P, V, M, R = lg.small_system()
    assert pts.shape == (lg.MANY, 2) and len(sample) == 2000 and (np.diff(sample) > 0).all() and sample[-1] < lg.MANY
    assert (sample > 65536).sum() > 100 and np.array_equal(pts[:lg.SMALL_N], P[(np.arange(lg.SMALL_N) * 7) % lg.SMALL_N])
    for a in (P, M, R):
        assert np.array_equal(a.astype(np.float32).astype(np.float64), a) and np.isfinite(a).all()
    assert not pts.flags.writeable


# ---------------------------------------------------------------------------------------------------------------------
# 4. the budget
# ---------------------------------------------------------------------------------------------------------------------
def test_references_within_budget():
    """A condition, not a measurement: no cached reference of state A may take more than 10 s."""
    for name in lg.NAMES:
        ref = lg.reference(name)
        assert lg.reference(name) is ref                           # computed once
    print("seconds: " + "   ".join("%s %.1f" % (name, lg.TIMES[name]) for name in lg.NAMES))
    for name in lg.NAMES:
        assert lg.TIMES[name] <= lg.BUDGET_S, (name, lg.TIMES[name])
    with pytest.raises(ValueError):
        lg.reference("pairs16")["counts"][0] = 1                   # read-only
