"""The ordered family on the MI355X, across kernels: diag_potential, batch_diag_potential, track_potential, field_at,
tracers_advance, tides_at and group_potential sum over j = 0 .. n-1 in ascending order through one tile walk and redo a
flagged row through one exact walk (csrc/nbody_diag.hpp).  The per-query files state the bit contracts
one by one; this one asks every kernel about the same states (ordered_cases.py: a remainder, a ragged tile, a second
workgroup, coincident bodies in every position) and compares the answers with zero tolerance.  The accuracy of a flagged
row is field_cases.py's and tide_cases.py's, through their own checkers."""
import functools

import numpy as np
import pytest

import field_cases as fc
import ordered_cases as oc
import tide_cases as tc

pytestmark = pytest.mark.gpu

PRECISIONS = [pytest.param(0, id="f32"), pytest.param(1, id="f64")]
EVERYTHING = (np.inf, 1.0)              # group_potential: one group holds every body


def setup_module(module):
    fc.require_long_double()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_bits(got, want, what):
    assert np.shape(got) == np.shape(want), (what, np.shape(got), np.shape(want))
    bad = np.argwhere(bits(got) != bits(want))
    assert len(bad) == 0, (what, "%d values differ, first at %s" % (len(bad), bad[:4].tolist()))


def config(nb):
    return nb.stock_config(particleCount=max(oc.SIZES), fieldWidth=int(oc.FIELD), fieldHeight=int(oc.FIELD))


def bodies(nb, n, precision):
    P, V, M, R = oc.state(n)
    return nb.BodiesData.from_arrays(P, V, M, R, precision) if n else nb.BodiesData(0, precision)


def queries(st):
    """What the four queries that a batch has too say about the resident state."""
    return {"diag": st.diagnostics(potential=True), "field": st.field(), "tides": st.tides(jerk=True),
            "group": st.group_potential(*EVERYTHING)}


@functools.lru_cache(maxsize=None)
def answers(precision, n):
    """Every kernel's answer about state n, asked once and shared by the tests below; never written to."""
    import ppa_nbody_collisions_amd as nb
    cfg = config(nb)
    b = bodies(nb, n, precision)
    P, V, M, R = oc.state(n)
    pts, pv = oc.points(P)
    with nb.Stepper(cfg, precision=precision, track_ids=True) as st, nb.Stepper(cfg, precision=precision) as twin:
        st.upload(b)
        out = queries(st)
        out["tides_alone"] = st.tides()
        out["tides_pts"], out["tides_pts_jerk"] = st.tides(pts), st.tides(pts, pv, jerk=True)
        out["field_pts"] = st.field(pts)
        st.reserve_tracks(1, potential=True)                    # every identity: column k is body k of the upload
        st.record_tracks()
        out["tracks"] = st.tracks()
        twin.upload(b)                                          # the same start state, with tracers at the points
        twin.set_tracers(pts)
        twin.step(1)
        out["tracers"] = twin.tracers()
    return out


@pytest.mark.parametrize("n", oc.SIZES)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_one_potential(precision, n):
    a = answers(precision, n)
    phi = a["diag"]["phi"]
    assert phi.shape == (n,)
    assert_bits(a["field"]["phi"], phi, "field")
    assert_bits(a["group"]["phi"], phi, "group_potential")
    assert a["group"]["n_groups"] == 1 and a["group"]["largest"] == n
    t = a["tracks"]
    assert t["phi"].shape == (1, n) and np.array_equal(t["index"][0], np.arange(n))
    assert_bits(t["phi"][0], phi, "tracks")


@pytest.mark.parametrize("n", oc.SIZES)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_the_tensor_with_and_without_the_jerk(precision, n):
    a = answers(precision, n)
    assert a["tides_alone"]["tide"].shape == (n, 3) and "jerk" not in a["tides_alone"]
    assert_bits(a["tides_alone"]["tide"], a["tides"]["tide"], "own rows")
    assert a["tides_pts"]["tide"].shape == (n + oc.FREE_POINTS, 3)
    assert_bits(a["tides_pts"]["tide"], a["tides_pts_jerk"]["tide"], "points")
    assert a["tides_pts"]["coincident"] == a["tides_pts_jerk"]["coincident"] == a["field_pts"]["coincident"] \
        == n + oc.expected_coincident(n)


@pytest.mark.parametrize("n", oc.SIZES)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_tracer_has_the_field_of_a_point(precision, n):
    a = answers(precision, n)
    t, f = a["tracers"], a["field_pts"]
    assert t["steps"] == 1 and t["coincident"] == f["coincident"]
    assert_bits(t["acc"], f["acc"], "acc")
    assert_bits(t["phi"], f["phi"], "phi")


@pytest.mark.parametrize("n", oc.SIZES)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_coincident_counts_and_flagged_rows(precision, n):
    a = answers(precision, n)
    P, V, M, R = oc.state(n)
    rows = np.arange(n)
    acc, phi, mag, coin_field = fc.exact_field(P, M, rows=rows)
    tide, jerk, coin_tides, bt, bj = tc.exact_tides(P, V, M, rows=rows)
    counts = (a["diag"]["coincident_pairs"], a["field"]["coincident"], a["tides"]["coincident"], a["tides_alone"]["coincident"],
              a["group"]["coincident"], coin_field, coin_tides)
    assert set(counts) == {oc.expected_coincident(n)}, counts
    for k in ("acc", "phi"):
        assert np.isfinite(a["field"][k]).all(), k
    for k in ("tide", "jerk"):
        assert np.isfinite(a["tides"][k]).all(), k
    # every row, the flagged ones (oc.flagged_rows) among them, within the bounds of the two oracles
    fc.check_field(a["field"]["acc"], a["field"]["phi"], acc, phi, mag, n, "n %d own rows" % n)
    tc.check_tides(a["tides"]["tide"], a["tides"]["jerk"], tide, jerk, bt, bj, n, "n %d own rows" % n)
    f = oc.flagged_rows(n)
    fc.check_field(a["field"]["acc"][f], a["field"]["phi"][f], acc[f], phi[f], mag[f], n, "n %d flagged rows" % n)
    tc.check_tides(a["tides"]["tide"][f], a["tides"]["jerk"][f], tide[f], jerk[f], bt[f], bj[f], n, "n %d flagged rows" % n)
    # and the points: the first n lie on the bodies, every one of them a flagged row of the points' kernels
    pts, pv = oc.points(P)
    acc, phi, mag, coin = fc.exact_field(P, M, points=pts)
    fc.check_field(a["field_pts"]["acc"], a["field_pts"]["phi"], acc, phi, mag, n, "n %d points" % n)
    tide, jerk, coin, bt, bj = tc.exact_tides(P, V, M, points=pts, point_vel=pv)
    tc.check_tides(a["tides_pts_jerk"]["tide"], a["tides_pts_jerk"]["jerk"], tide, jerk, bt, bj, n, "n %d points" % n)


def test_a_batch_has_the_bits_of_its_steppers(nb):
    sizes = (0,) + oc.SIZES
    cfg = config(nb)
    cap = max(oc.SIZES)
    with nb.StepperBatch(len(sizes), cap, cfg=cfg) as batch:
        batch.upload([bodies(nb, n, nb.F32) for n in sizes])
        got = {"diag": batch.diagnostics(potential=True), "field": batch.field(), "tides": batch.tides(jerk=True),
               "group": batch.group_potential(*EVERYTHING)}
    for s, n in enumerate(sizes):
        if n:
            want = answers(0, n)
        else:
            with nb.Stepper(cfg) as st:
                st.upload(bodies(nb, 0, nb.F32))
                want = queries(st)
        what = "system %d, n %d: " % (s, n)
        d, w = got["diag"][s], want["diag"]
        assert d["n_bodies"] == n
        assert sorted(d) == sorted(w), what
        for k in ("step", "n_bodies", "coincident_pairs"):
            assert d[k] == w[k], what + k
        for k in ("mass", "momentum", "angular_momentum", "kinetic", "potential", "phi"):
            assert_bits(d[k], w[k], what + "diagnostics " + k)
        if n:
            assert_bits(d["center_of_mass"], w["center_of_mass"], what + "diagnostics center_of_mass")
        else:                                                   # an empty system has none: NaN, whose payload is no result
            assert np.isnan(d["center_of_mass"]).all() and np.isnan(w["center_of_mass"]).all(), what
        for k in ("acc", "phi"):
            assert_bits(got["field"][k][s, :n], want["field"][k], what + "field " + k)
            assert not bits(got["field"][k][s, n:]).any(), what + k
        for k in ("tide", "jerk"):
            assert_bits(got["tides"][k][s, :n], want["tides"][k], what + "tides " + k)
            assert not bits(got["tides"][k][s, n:]).any(), what + k
        assert got["field"]["coincident"][s] == want["field"]["coincident"], what
        assert got["tides"]["coincident"][s] == want["tides"]["coincident"], what
        g, w = got["group"][s], want["group"]
        assert_bits(g["phi"], w["phi"], what + "group_potential phi")
        assert np.array_equal(g["label"], w["label"]) and g["coincident"] == w["coincident"], what
