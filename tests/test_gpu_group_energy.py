"""Group energies (nbody_get_group_potential, nbody_batch_get_group_potential, nbody_group_catalog; Stepper.group_potential,
Stepper.group_energies and their StepperGroup / StepperBatch forms) on the MI355X.

What is compared with zero tolerance, product against product: the labels against groups(); with one group (link +inf) phi
against diagnostics(potential=True) - nothing is skipped; with no links every phi is -0.0 - everything is skipped; the
sub-state rule - phi of a group's members against the diagnostics of a fresh context that holds exactly those members in
ascending order; a batch against a Stepper; a rank of a group against a plain context; the catalogue against the numpy
model of group_energy_cases.py.  Against the long-double oracle every row is within (n_g + 4) u |phi_in| (group_energy_cases:
the diagnostics' bound with the number of terms actually summed), no sampling."""
import functools

import numpy as np
import pytest

import group_energy_cases as ge
import lineage_cases as lc
import oracle_lib as ol
import sharded_cases as sc

pytestmark = pytest.mark.gpu

INVALID, CAPACITY_ERR, STATE_ERR = -1, -7, -9
PRECISIONS = [pytest.param(0, id="f32"), pytest.param(1, id="f64")]
FIELD = 2000                                                    # holds standard_state(1500): 23 x 23 cells of 40


def small_stepper(nb, precision, capacity):
    return nb.Stepper(capacity=max(capacity, 1), precision=precision, timestep=0.2, growthRate=0.1, fieldWidth=FIELD, fieldHeight=FIELD)


def bodies_of(nb, state, precision, rows=None):
    P, V, M, R = state if rows is None else [a[rows] for a in state]
    return nb.BodiesData.from_arrays(P, V, M, R, precision) if len(M) else nb.BodiesData(0, precision)


@functools.lru_cache(maxsize=None)
def standard(n, precision):
    """standard_state(n) at the precision's dtype, shared and never written to."""
    state = ge.standard_state(n, ge.DTYPE_OF[precision])
    for a in state:
        a.setflags(write=False)
    return state


def widen(d):
    """A download -> (P, V, M, R) float64, exact."""
    return tuple(np.asarray(a, dtype=np.float64) for a in (d.Positions, d.Velocities, d.Masses, d.Radii))


def assert_same_potential(got, want, what):
    assert np.array_equal(got["label"], want["label"]) and got["label"].dtype == np.int32, what
    assert got["phi"].dtype == np.float64 and np.array_equal(ge.bits(got["phi"]), ge.bits(want["phi"])), what
    assert [got[k] for k in ("n_groups", "largest", "coincident")] == [want[k] for k in ("n_groups", "largest", "coincident")], what


def substate_phi(nb, state, precision, members):
    """diagnostics(potential=True)["phi"] of a fresh context that holds exactly `members` (ascending) of the state."""
    assert (np.diff(members) > 0).all()
    with small_stepper(nb, precision, len(members)) as sub:
        sub.upload(bodies_of(nb, state, precision, members))
        return sub.diagnostics(potential=True)["phi"]


def assert_substate_rule(nb, state, precision, got, members, what):
    want = substate_phi(nb, state, precision, members)
    have = got["phi"][members]
    bad = np.flatnonzero(ge.bits(have) != ge.bits(want))
    assert bad.size == 0, (what, "%d of %d members differ, first %d" % (bad.size, len(members), bad[0]), have[bad[:3]], want[bad[:3]])


# ---------------------------------------------------------------------------------------------------------------------
# 1. labels, and every row within the bound
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ge.GPU_N)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_labels_and_every_row_within_the_bound(nb, precision, n):
    ge.require_long_double()
    state = standard(n, precision)
    P, V, M, R = state
    with small_stepper(nb, precision, n) as st:
        st.upload(bodies_of(nb, state, precision))
        got = st.group_potential(ge.LINK, ge.SCALE)
        grp = st.groups(ge.LINK, ge.SCALE)
        assert np.array_equal(got["label"], grp["label"]) and np.array_equal(got["label"], ge.labels_of_plan(n))
        assert (got["n_groups"], got["largest"]) == (grp["n_groups"], grp["largest"]) and got["sweeps"] >= 1
        assert got["phi"].shape == (n,) and got["phi"].dtype == np.float64
        worst, coincident = ge.assert_rows_within_bound(got["phi"], P, M, got["label"], "n %d" % n)
        assert got["coincident"] == coincident == 0
        if n >= 131:
            assert (got["phi"][got["label"] == got["label"][np.argmax(np.bincount(got["label"])[got["label"]])]] < 0).all()
        again = st.group_potential(ge.LINK, ge.SCALE)               # the same call, the same bits
        assert_same_potential(again, got, "n %d again" % n)


# ---------------------------------------------------------------------------------------------------------------------
# 2. one group: nothing is skipped, the bits of the diagnostics.  No links: everything is skipped, -0.0
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ge.GPU_N)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_one_group_has_the_bits_of_the_diagnostics(nb, precision, n):
    state = standard(n, precision)
    with small_stepper(nb, precision, n) as st:
        st.upload(bodies_of(nb, state, precision))
        got = st.group_potential(np.inf, 1.0)
        want = st.diagnostics(potential=True)
        assert (got["label"] == 0).all() and (got["n_groups"], got["largest"]) == (1, n)
        bad = np.flatnonzero(ge.bits(got["phi"]) != ge.bits(want["phi"]))
        assert bad.size == 0, ("n %d" % n, bad.size, bad[:4], got["phi"][bad[:4]], want["phi"][bad[:4]])
        assert got["coincident"] == want["coincident_pairs"] == 0
        if n == 1:
            assert ge.bits(got["phi"]).tolist() == ge.bits(np.array([-0.0])).tolist()


@pytest.mark.parametrize("n", ge.GPU_N)
@pytest.mark.parametrize("precision", PRECISIONS)
def test_no_links_every_phi_is_minus_zero(nb, precision, n):
    state = standard(n, precision)                                # no coincident bodies: test_group_energy_cases_cpu.py
    with small_stepper(nb, precision, n) as st:
        st.upload(bodies_of(nb, state, precision))
        got = st.group_potential(0.0, 0.0)
        assert np.array_equal(got["label"], np.arange(n)) and (got["n_groups"], got["largest"], got["coincident"]) == (n, 1, 0)
        assert (ge.bits(got["phi"]) == ge.bits(np.float64(-0.0))).all()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the sub-state rule
# ---------------------------------------------------------------------------------------------------------------------
def chosen_groups(label, seed):
    """The largest group, a smaller group with members on both sides of the tile boundary at 128, one pair, and three more
    groups of two or more members by a fixed seed -> a list of (name, ascending members)."""
    n = len(label)
    size = np.bincount(label, minlength=n)
    members = {int(l): np.flatnonzero(label == l) for l in np.flatnonzero(size >= 2)}
    big = int(np.argmax(size))
    out = [("largest", members[big])]
    across = [l for l, m in members.items() if l != big and len(m) >= 3 and m[0] < 128 <= m[-1]]
    out.append(("across the tile boundary", members[across[0]]))
    pairs = [l for l, m in members.items() if len(m) == 2]
    out.append(("a pair", members[pairs[0]]))
    rest = [l for l in members if l not in (big, across[0], pairs[0])]
    for l in np.random.default_rng(seed).choice(rest, 3, replace=False):
        out.append(("group %d" % l, members[int(l)]))
    return out


@pytest.mark.parametrize("n", [300, 1500])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_sub_state_rule(nb, precision, n):
    state = standard(n, precision)
    with small_stepper(nb, precision, n) as st:
        st.upload(bodies_of(nb, state, precision))
        got = st.group_potential(ge.LINK, ge.SCALE)
    picks = chosen_groups(got["label"], seed=n)
    assert len(picks) == 6 and len(picks[0][1]) == ge.BIG
    big = picks[0][1]
    assert big[0] // 128 != big[-1] // 128 and big[0] // 256 != big[-1] // 256      # the largest straddles both boundaries
    for name, members in picks:
        assert_substate_rule(nb, state, precision, got, members, "n %d %s (%d members)" % (n, name, len(members)))


# ---------------------------------------------------------------------------------------------------------------------
# 4. hand cases
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", PRECISIONS)
def test_hand_cases(nb, precision):
    seen = []
    for name, only, P, V, M, R, link, scale, phi_want, label_want, coincident in ge.hand_cases():
        if only is not None and only != precision:
            continue
        seen.append(name[0])
        with small_stepper(nb, precision, len(M)) as st:
            st.upload(bodies_of(nb, (P, V, M, R), precision))
            got = st.group_potential(link, scale)
            assert got["label"].tolist() == label_want, name
            assert ge.bits(got["phi"]).tolist() == ge.bits(np.array(phi_want)).tolist(), (name, got["phi"])
            assert got["coincident"] == coincident, name
            cat = st.group_energies(link, scale)
            assert cat["label"].tolist() == sorted(set(label_want)) and cat["count"].sum() == len(M), name
            if name[0] == "c":
                assert np.isnan(cat["cx"]).all() and not cat["flags"].any(), name      # no mass: no centre
    assert seen == (["a", "b", "c", "d"] if precision == 1 else ["a", "c", "d"])


def test_coincident_members_inside_a_larger_group(nb):
    """Two coincident bodies inside the big group: their rows take the general code, each leaves the other out and counts
    it, and the sub-state rule still holds for every member."""
    n = 300
    P, V, M, R = [a.copy() for a in standard(n, 0)]
    label = ge.labels_of_plan(n)
    big = np.flatnonzero(label == label[40])
    P[big[70]] = P[big[3]]
    state = (P, V, M, R)
    with small_stepper(nb, 0, n) as st:
        st.upload(bodies_of(nb, state, 0))
        got = st.group_potential(ge.LINK, ge.SCALE)
    assert np.array_equal(got["label"], label) and got["coincident"] == 2
    worst, coincident = ge.assert_rows_within_bound(got["phi"], P, M, label, "coincident members")
    assert coincident == 2
    assert_substate_rule(nb, state, 0, got, big, "coincident members")


# ---------------------------------------------------------------------------------------------------------------------
# 5. a batch
# ---------------------------------------------------------------------------------------------------------------------
BATCH_COUNTS = [300, 129, 1, 0, 64]
BATCH_LINKS = ((ge.LINK, ge.SCALE), (0.0, 1.0), (np.inf, 0.0))


def check_batch(nb, batch, one, bodies, links, what):
    """Every system of the batch against `one` holding that system's state; the raw call leaves the slices' tails alone."""
    S, cap = batch.systems, batch.capacity
    counts = batch.counts()
    for link, scale in links:
        got = batch.group_potential(link, scale)
        cats = batch.group_energies(link, scale)
        label = np.full((S, cap), -77, dtype=np.int32)
        phi = np.full((S, cap), 7.5)
        info = np.zeros(S, dtype=ge.INFO_DTYPE)
        assert nb.lib.nbody_batch_get_group_potential(batch._b, link, scale, label.ctypes.data, phi.ctypes.data, info.ctypes.data) == 0
        for s in range(S):
            n = int(counts[s])
            w = "%s system %d (n %d) link %g scale %g" % (what, s, n, link, scale)
            assert info["n_bodies"][s] == n == len(got[s]["label"]), w
            assert np.array_equal(label[s, :n], got[s]["label"]) and (label[s, n:] == -77).all(), w
            assert np.array_equal(ge.bits(phi[s, :n]), ge.bits(got[s]["phi"])) and (phi[s, n:] == 7.5).all(), w
            assert (info["n_groups"][s], info["largest"][s], info["coincident"][s]) == (got[s]["n_groups"], got[s]["largest"], got[s]["coincident"]), w
            if n == 0:
                assert (got[s]["n_groups"], got[s]["largest"], got[s]["coincident"]) == (0, 0, 0) and len(cats[s]) == 0, w
                continue
            one.upload(bodies(s))
            assert_same_potential(got[s], one.group_potential(link, scale), w)
            P, V, M, R = widen(batch.download(s))
            ge.assert_same_catalog(cats[s], ge.model_catalog(P, V, M, got[s]["label"], got[s]["phi"]), w)
            ge.assert_same_catalog(cats[s], one.group_energies(link, scale), w)
    return counts


def test_batch_equals_stepper(nb):
    ge.require_long_double()
    S, cap = len(BATCH_COUNTS), 300
    states = [standard(n, 0) if n else None for n in BATCH_COUNTS]
    bodies = [bodies_of(nb, st, 0) if st is not None else nb.BodiesData(0) for st in states]
    with nb.StepperBatch(S, cap, params=[(0.2, 0.1, FIELD, FIELD)] * S) as batch, small_stepper(nb, 0, cap) as one:
        batch.upload(bodies)
        counts = check_batch(nb, batch, one, lambda s: bodies[s], BATCH_LINKS, "at upload")
        assert counts.tolist() == BATCH_COUNTS
        got = batch.group_potential(ge.LINK, ge.SCALE)
        for s, st in enumerate(states):
            if st is not None:
                assert np.array_equal(got[s]["label"], ge.labels_of_plan(BATCH_COUNTS[s]))
                ge.assert_rows_within_bound(got[s]["phi"], st[0], st[2], got[s]["label"], "system %d" % s)


def test_batch_after_steps_with_collisions(nb):
    """Two steps of the dense stock state: bodies merge, so every count comes from Meta on the device."""
    S, cap = len(BATCH_COUNTS), 300
    cfg, full = lc.dense_bodies(nb, cap)
    bodies = [nb.BodiesData.from_arrays(full.Positions[:n], full.Velocities[:n], full.Masses[:n], full.Radii[:n]) if n else nb.BodiesData(0)
              for n in BATCH_COUNTS]
    with nb.StepperBatch(S, cap, cfg=cfg) as batch, nb.Stepper(cfg) as one:
        batch.upload(bodies)
        batch.step(2)
        after = [batch.download(s) for s in range(S)]
        counts = check_batch(nb, batch, one, lambda s: after[s], ((0.0, 1.0), (150.0, 0.0)), "after two steps")
        assert counts[0] < 300 and counts[4] < 64 and counts[3] == 0, counts   # merged on the device: no host count is current
        got = batch.group_potential(150.0, 0.0)
        assert 1 < got[0]["n_groups"] < counts[0] and got[0]["largest"] > 1
        P, V, M, R = widen(after[0])
        ge.assert_rows_within_bound(got[0]["phi"], P, M, got[0]["label"], "system 0 after two steps")


# ---------------------------------------------------------------------------------------------------------------------
# 6. a ring-kernel context, at upload and after two steps
# ---------------------------------------------------------------------------------------------------------------------
def test_ring_kernel_context(nb):
    ge.require_long_double()
    n = 8269                                                        # ragged: 64 tiles and 77 bodies, 33 workgroups
    cfg = nb.stock_config(particleCount=n, fieldWidth=12000, fieldHeight=12000)
    b = nb.init_bodies(cfg)
    with nb.Stepper(cfg) as st:
        assert "ring" in st.force_kernel_name()
        st.upload(b)
        for what in ("at upload", "after two steps"):
            d = st.download()
            P, V, M, R = state = widen(d)
            got = st.group_potential(0.0, 1.0)
            grp = st.groups(0.0, 1.0)
            print("ring context %s: n %d, %d groups, largest %d, coincident %d" % (what, d.numBodies, got["n_groups"], got["largest"],
                                                                                    got["coincident"]))
            assert np.array_equal(got["label"], grp["label"]) and (got["n_groups"], got["largest"]) == (grp["n_groups"], grp["largest"])
            assert len(got["label"]) == d.numBodies and 1 < got["n_groups"] < d.numBodies
            worst, coincident = ge.assert_rows_within_bound(got["phi"], P, M, got["label"], "ring context " + what)
            assert got["coincident"] == coincident
            size = np.bincount(got["label"])
            members = np.flatnonzero(got["label"] == np.argmax(size))
            assert len(members) == got["largest"] >= 2
            assert_substate_rule(nb, state, 0, got, members, "ring context %s, the largest group" % what)
            cat = st.group_energies(0.0, 1.0)
            ge.assert_same_catalog(cat, ge.model_catalog(P, V, M, got["label"], got["phi"]), "ring context " + what)
            if what == "at upload":
                assert d.numBodies == n
                st.step(2)
            else:
                assert d.numBodies < n


# ---------------------------------------------------------------------------------------------------------------------
# 7. group_energies: the catalogue of the downloaded state
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [129, 300, 1500])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_group_energies_equal_the_model(nb, precision, n):
    state = standard(n, precision)
    with small_stepper(nb, precision, n) as st:
        st.upload(bodies_of(nb, state, precision))
        got = st.group_potential(ge.LINK, ge.SCALE)
        cat = st.group_energies(ge.LINK, ge.SCALE)
        P, V, M, R = widen(st.download())
        for a, b in zip((P, V, M, R), state):
            assert np.array_equal(a, b)
        want = ge.model_catalog(P, V, M, got["label"], got["phi"])
        ge.assert_same_catalog(cat, want, "n %d" % n)
        assert len(cat) == got["n_groups"] and cat["count"].max() == got["largest"]
        if n >= 300:
            assert (cat["energy"] < 0).any() and (cat["energy"] > 0).any()
            big = cat[cat["count"] == ge.BIG][0]
            assert big["flags"] & ge.BOUND and big["bound_members"] == ge.BIG - 1      # bound, with its one fast member


# ---------------------------------------------------------------------------------------------------------------------
# 8. not collective: either rank of a group, past the exchange lag
# ---------------------------------------------------------------------------------------------------------------------
def test_either_rank_of_a_group(nb):
    run = (1500, ol.LITERAL)
    cfg, bodies = lc.dense_bodies(nb, run[0])
    grp = nb.StepperGroup(2, cfg=cfg)
    plain = nb.Stepper(cfg)
    try:
        grp.upload(bodies)
        plain.upload(bodies)
        steps = sc.LAG + 1                                          # the layout has shrunk for the first time
        grp.step(steps)
        plain.step(steps)
        assert plain.body_count() == sc.COUNTS[run][steps - 1]
        for link, scale in ((0.0, 1.0), (sc.CENTRE_LINK[run], 0.0)):
            want = plain.group_potential(link, scale)
            assert 1 < want["n_groups"] < len(want["label"])
            for rank in (1, 0):                                     # each on its own
                assert_same_potential(grp.group_potential(link, scale, rank=rank), want, "rank %d link %g" % (rank, link))
        with pytest.raises(nb.NbodyError) as err:                   # a rank holds only its own velocities
            grp.ranks[1].group_energies(0.0, 1.0)
        assert err.value.status == STATE_ERR
    finally:
        grp.close()
        plain.close()


# ---------------------------------------------------------------------------------------------------------------------
# 9. errors on a live context
# ---------------------------------------------------------------------------------------------------------------------
def test_errors(nb):
    state = standard(300, 0)
    call = nb.lib.nbody_get_group_potential
    label = np.full(300, -7, dtype=np.int32)
    phi = np.full(300, 7.5)
    info = np.full(1, -7, dtype=ge.INFO_DTYPE)
    untouched = (label.tobytes(), phi.tobytes(), info.tobytes())
    with small_stepper(nb, 0, 300) as st:
        assert call(st._ctx, 1.0, 1.0, label.ctypes.data, phi.ctypes.data, 300, info.ctypes.data) == STATE_ERR   # before an upload
        assert b"before" in nb.lib.nbody_last_error_string()
        st.upload(bodies_of(nb, state, 0))
        assert call(st._ctx, 1.0, 1.0, label.ctypes.data, phi.ctypes.data, 299, info.ctypes.data) == CAPACITY_ERR
        assert call(st._ctx, 1.0, 1.0, label.ctypes.data, phi.ctypes.data, -1, info.ctypes.data) == INVALID
        assert call(st._ctx, 1.0, 1.0, None, phi.ctypes.data, 300, info.ctypes.data) == INVALID
        assert call(st._ctx, 1.0, 1.0, label.ctypes.data, None, 300, info.ctypes.data) == INVALID
        assert call(st._ctx, 1.0, 1.0, label.ctypes.data, phi.ctypes.data, 300, None) == INVALID
        assert call(None, 1.0, 1.0, label.ctypes.data, phi.ctypes.data, 300, info.ctypes.data) == INVALID
        for link, scale in ((-1.0, 1.0), (np.nan, 1.0), (1.0, np.inf), (1.0, -1.0), (1.0, np.nan)):
            assert call(st._ctx, link, scale, label.ctypes.data, phi.ctypes.data, 300, info.ctypes.data) == INVALID, (link, scale)
        assert (label.tobytes(), phi.tobytes(), info.tobytes()) == untouched
        assert call(st._ctx, ge.LINK, ge.SCALE, label.ctypes.data, phi.ctypes.data, 300, info.ctypes.data) == 0
        want = st.group_potential(ge.LINK, ge.SCALE)
        assert np.array_equal(label, want["label"]) and np.array_equal(ge.bits(phi), ge.bits(want["phi"]))
        assert tuple(info[0])[:3] == (300, want["n_groups"], want["largest"]) and info["sweeps"][0] >= 1 and info["coincident"][0] == 0
        st.upload(nb.BodiesData(0))                               # no bodies: nothing launched, a zero record
        assert call(st._ctx, 4.0, 1.0, label.ctypes.data, phi.ctypes.data, 0, info.ctypes.data) == 0
        assert tuple(info[0]) == (0, 0, 0, 0, 0) and np.array_equal(label, want["label"])
        assert len(st.group_energies(4.0)) == 0
    with nb.StepperBatch(2, 300, params=[(0.2, 0.1, FIELD, FIELD)] * 2) as batch:
        labels = np.full((2, 300), -7, dtype=np.int32)
        phis = np.full((2, 300), 7.5)
        infos = np.full(2, -7, dtype=ge.INFO_DTYPE)
        bcall = nb.lib.nbody_batch_get_group_potential
        assert bcall(batch._b, 1.0, 1.0, labels.ctypes.data, phis.ctypes.data, infos.ctypes.data) == STATE_ERR
        batch.upload([bodies_of(nb, state, 0), nb.BodiesData(0)])
        assert bcall(batch._b, 1.0, 1.0, None, phis.ctypes.data, infos.ctypes.data) == INVALID
        assert bcall(batch._b, 1.0, 1.0, labels.ctypes.data, None, infos.ctypes.data) == INVALID
        assert bcall(batch._b, 1.0, 1.0, labels.ctypes.data, phis.ctypes.data, None) == INVALID
        assert bcall(batch._b, 1.0, -2.0, labels.ctypes.data, phis.ctypes.data, infos.ctypes.data) == INVALID
        assert (labels == -7).all() and (phis == 7.5).all() and (infos["sweeps"] == -7).all()
    grp = nb.StepperGroup(2, capacity=300, timestep=0.2, growthRate=0.1, fieldWidth=FIELD, fieldHeight=FIELD)
    try:
        grp.upload(bodies_of(nb, state, 0))
        for r in grp.ranks:                                         # a rank holds only its own velocities
            with pytest.raises(nb.NbodyError) as err:
                r.group_energies(ge.LINK, ge.SCALE)
            assert err.value.status == STATE_ERR
            assert_same_potential(r.group_potential(ge.LINK, ge.SCALE), want, "a rank of two")   # the potential stays available
    finally:
        grp.close()
