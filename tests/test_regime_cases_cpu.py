"""CPU half of the regime tests: the numpy statement of the screen bookkeeping at its exact bounds, and - the condition
that keeps tests/test_gpu_regimes.py from passing vacuously - every mid-run case stepped through the oracle: the summary
sequence it declares is the one the oracle's trajectory shows, and every transition the GPU tests are there for occurs."""
import ctypes
import os

import numpy as np
import pytest

import oracle_lib as ol
import regime_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def _summary32(x=1.0, y=1.0, m=1.0, r=0.0):
    return rc.expected_summary(np.array([[1.0, 1.0], [x, y]], f32), np.array([1.0, m], f32), np.array([0.0, r], f32), rc.F32)


def test_expected_summary_at_the_exact_bounds_fp32():
    below = lambda v: np.nextafter(f32(v), f32(0))
    assert _summary32() == 0
    assert _summary32(x=2.0 ** 38) == rc.UNBOUNDED and _summary32(y=-2.0 ** 38) == rc.UNBOUNDED
    assert _summary32(x=below(2.0 ** 38)) == 0 and _summary32(y=-below(2.0 ** 38)) == 0
    assert _summary32(x=np.inf) == rc.UNBOUNDED and _summary32(y=-np.inf) == rc.UNBOUNDED
    assert _summary32(x=np.nan) == rc.UNBOUNDED | rc.SMALL          # a NaN coordinate is unbounded AND small
    assert _summary32(x=2.0 ** -16) == 0 and _summary32(y=-2.0 ** -16) == 0
    assert _summary32(x=below(2.0 ** -16)) == rc.SMALL and _summary32(y=-below(2.0 ** -16)) == rc.SMALL
    assert _summary32(x=0.0) == rc.SMALL and _summary32(y=-0.0) == rc.SMALL and _summary32(x=1e-42) == rc.SMALL
    assert _summary32(m=2.0 ** 90) == rc.MASS and _summary32(m=-2.0 ** 90) == rc.MASS
    assert _summary32(m=below(2.0 ** 90)) == 0 and _summary32(m=0.0) == 0 and _summary32(m=1e-42) == 0
    assert _summary32(m=np.inf) == rc.MASS and _summary32(m=np.nan) == rc.MASS
    assert _summary32(r=0.0) == 0
    for r in (-0.0, 1e-45, 1e-42, 1.0, -1.0, np.inf, -np.inf, np.nan):
        assert _summary32(r=r) == rc.RADIUS, r
    assert _summary32(x=np.nan, m=np.nan, r=np.nan) == 15


def test_expected_summary_fp64_has_two_bits():
    s = lambda x=1.0, m=1.0, r=0.0: rc.expected_summary(np.array([[x, 1.0]]), np.array([m]), np.array([r]), rc.F64)
    assert s() == 0 and s(x=0.0) == 0 and s(x=1e-300) == 0 and s(m=np.inf) == 0 and s(m=np.nan) == 0
    assert s(x=2.0 ** 249) == rc.UNBOUNDED and s(x=np.nextafter(2.0 ** 249, 0)) == 0 and s(x=-2.0 ** 249) == rc.UNBOUNDED
    assert s(x=2.0 ** 38) == 0 and s(x=np.inf) == rc.UNBOUNDED and s(x=np.nan) == rc.UNBOUNDED
    assert s(r=-0.0) == rc.RADIUS and s(r=5e-324) == rc.RADIUS and s(r=np.nan) == rc.RADIUS and s(r=0.0) == 0


def test_expected_tile_rmax():
    R = np.zeros(300, f32)
    R[0], R[127] = -3.0, 2.0                               # |r|; the tile's last body
    R[128], R[130] = np.nan, 1e-42                         # NaN ignored, a denormal kept
    R[256], R[299] = np.inf, np.nan                        # inf kept
    got = rc.expected_tile_rmax(R, 6)
    want = np.array([3.0, 1e-42, np.inf, 0, 0, 0], f32)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    only_nan = np.full(128, np.nan, f32)
    assert np.array_equal(rc.expected_tile_rmax(only_nan, 3).view(np.uint32), np.zeros(3, np.uint32))
    assert np.array_equal(rc.expected_tile_rmax(np.array([-0.0], f32), 2).view(np.uint32), np.zeros(2, np.uint32))
    assert rc.expected_tile_rmax(np.zeros(0, f32), 2).tolist() == [0, 0]
    assert rc.expected_tile_rmax(np.array([1e300]), 1)[0] == np.inf      # fp64 radii: rounded to float


def test_accessor_is_declared_bound_and_refuses_null(nb):
    name = "nbody_debug_screen_state"
    assert name in nb.SYMBOLS and getattr(nb.lib, name).argtypes == nb.SYMBOLS[name][1]
    with open(os.path.join(ROOT, "include", "nbody.h")) as f:
        assert "int nbody_debug_screen_state(nbody_ctx* ctx, int* summary, float* tile_rmax, int cap, int* n_tiles);" in f.read()
    s, k = ctypes.c_int(-7), ctypes.c_int(-7)
    buf = np.zeros(4, f32)
    assert nb.lib.nbody_debug_screen_state(None, ctypes.byref(s), buf.ctypes.data, 4, ctypes.byref(k)) == -1
    assert b"nbody_debug_screen_state" in nb.lib.nbody_last_error_string()
    assert nb.lib.nbody_debug_screen_state(None, None, None, 0, None) == -1
    assert (s.value, k.value) == (-7, -7) and not buf.any()
    assert nb.lib.nbody_abi_version() == 2


CASES = rc.mid_run_cases_f32() + rc.mid_run_cases_f64()


@pytest.fixture(scope="module")
def trajectories():
    return {c["name"]: rc.oracle_trajectory(c, want_events=True) for c in CASES}


def _transitions(c):
    seq = [c["summary0"]] + c["summaries"]
    return set(zip(seq[:-1], seq[1:]))


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_case_shows_the_summaries_it_declares(case, trajectories):
    b = case["bodies"]
    assert 2048 <= case["n"] <= 8192 and 6 <= case["steps"] <= 10
    assert rc.expected_summary(b.Positions, b.Masses, b.Radii, case["precision"]) == case["summary0"], \
        "%s: summary at upload" % case["name"]
    got = rc.summaries_of(case, trajectories[case["name"]])
    assert got == case["summaries"], "%s: the oracle's trajectory shows %r, the case declares %r" % (
        case["name"], got, case["summaries"])


def test_every_transition_occurs():
    f32_cases = rc.mid_run_cases_f32()
    seen = set().union(*[_transitions(c) for c in f32_cases])
    for t in ((0, rc.SMALL), (rc.SMALL, 0), (0, rc.UNBOUNDED), (rc.UNBOUNDED, 0), (0, rc.MASS), (rc.RADIUS, 0)):
        assert t in seen, "no fp32 case goes %d -> %d" % t
    seen64 = set().union(*[_transitions(c) for c in rc.mid_run_cases_f64()])
    for t in ((0, rc.UNBOUNDED), (rc.UNBOUNDED, 0), (rc.RADIUS, 0)):
        assert t in seen64, "no fp64 case goes %d -> %d" % t


def test_small_coordinates_land_where_the_case_says(trajectories):
    c = rc.case_small_enters_and_leaves()
    i, j = c["small_bodies"]
    tr = trajectories[c["name"]]
    P2 = ol.carve(tr[1][1], tr[1][0])[0]
    assert P2[i, 0] == f32(2.0 ** -20) and P2[j, 1] == 0.0 and not np.signbit(P2[j, 1])
    P3 = ol.carve(tr[2][1], tr[2][0])[0]
    assert abs(P3[i, 0]) > 0.5 and P3[j, 1] == -1.0


def test_pair_sits_below_the_chain_domain_while_bit_2_is_set(trajectories):
    c = rc.case_small_pair_below_the_chain_domain()
    i, j = c["pair"]
    k = c["pair_step"]
    tr = trajectories[c["name"]]
    assert c["summaries"][k - 1] == rc.SMALL and c["summaries"][k] == rc.SMALL
    P, V, M, _ = ol.carve(tr[k - 1][1], tr[k - 1][0])
    dx, dy = f32(P[j, 0] - P[i, 0]), f32(P[j, 1] - P[i, 1])
    d2 = f32(f32(dx * dx) + f32(dy * dy))
    assert 0 < d2 < f32(2.0 ** -80), d2                     # outside [2^-80, 2^80], the proved domain of the fast chain
    assert abs(float(P[j, 0]) - float(P[i, 0])) == 2.0 ** -41 and 0 < P[i, 0] < 2.0 ** -17 and 0 < P[j, 0] < 2.0 ** -17
    # the pair's own term shows in the state: the next step changes both velocities (everything else is below half an ulp)
    V4 = ol.carve(tr[k][1], tr[k][0])[1]
    assert V4[i, 0] != V[i, 0] and V4[j, 0] != V[j, 0]
    # and every pair is inside the domain at upload and after step 1, when bit 2 is clear
    for blk, n in ((c["bodies"].block, c["n"]), (tr[0][1], tr[0][0])):
        Pk = ol.carve(blk, n)[0]
        assert abs(float(Pk[j, 0]) - float(Pk[i, 0])) >= 2.0 ** -40


@pytest.mark.parametrize("precision", [rc.F32, rc.F64])
@pytest.mark.parametrize("where", ["tile0", "middle", "last-tile"])
def test_body_leaves_the_bound_and_returns(where, precision, trajectories):
    c = rc.case_body_leaves_the_bound(where, precision)
    i = c["body"]
    bound = 2.0 ** (249 if precision == rc.F64 else 38)
    assert c["n"] % 128 != 0 and {"tile0": i < 128, "middle": 1024 < i < 2048, "last-tile": i >= c["n"] // 128 * 128}[where]
    xs = [float(ol.carve(blk, n)[0][i, 0]) for n, blk, _, _ in trajectories[c["name"]]]
    assert all(n == c["n"] for n, _, _, _ in trajectories[c["name"]])
    assert [abs(x) >= bound for x in xs] == [True, False, True, False, True, False], xs


def test_masses_merge(trajectories):
    c = rc.case_masses_merge_past_the_bound()
    M0 = c["bodies"].Masses
    assert M0.max() == f32(1.5 * 2.0 ** 89) < f32(2.0 ** 90)
    n1, blk, ab, de = trajectories[c["name"]][0]
    (e0, e1), (u0, u1) = c["equal"], c["unequal"]
    assert sorted(map(tuple, ab.tolist())) == sorted([(e0, e1), (e1, e0), (u1, u0)]) and de.tolist() == [u0] and n1 == c["n"] - 1
    M1 = np.sort(ol.carve(blk, n1)[2])[-3:]
    assert M1.tolist() == [2.0 ** 90, 2.0 ** 90, 2.5 * 2.0 ** 89]
    assert not np.isnan(trajectories[c["name"]][3][1]).any()   # four steps of finite state (then the field is torn apart)


@pytest.mark.parametrize("precision", [rc.F32, rc.F64])
@pytest.mark.parametrize("growth", [0.0, 0.1])
def test_last_radius_disappears(growth, precision, trajectories):
    c = rc.case_last_radius_disappears(growth, precision)
    light, host = c["light"], c["host"]
    R0 = c["bodies"].Radii
    assert np.count_nonzero(R0) == 1 and R0[light] == 500.0 and c["bodies"].Masses.argmin() == light
    assert light // 128 != host // 128
    tr = trajectories[c["name"]]
    for k in (0, 1):
        assert tr[k][0] == c["n"] and len(tr[k][2]) == 0
    n3, blk3, ab3, de3 = tr[2]
    assert ab3.tolist() == [[host, light]] and de3.tolist() == [light] and n3 == c["n"] - 1
    rm2 = rc.expected_tile_rmax(ol.carve(tr[1][1], tr[1][0])[3], 18)
    rm3 = rc.expected_tile_rmax(ol.carve(blk3, n3)[3], 18)
    assert np.nonzero(rm2)[0].tolist() == [light // 128]
    if growth == 0:
        assert not rm3.any()                               # and summary 2 -> 0: asserted by the sequence
    else:
        new_host = host - (light < host)
        assert np.nonzero(rm3)[0].tolist() == [new_host // 128] and rm3[new_host // 128] == 50.0   # the maximum changed tile
    # the radius-0 pair collides after the switch
    i, j = c["pair"]
    i, j = i - (light < i), j - (light < j)
    n5, _, ab5, de5 = tr[4]
    assert len(ab5) == 1 and sorted(ab5[0].tolist()) == [i, j] and len(de5) == 1 and n5 == c["n"] - 2
    assert len(tr[3][2]) == 0 and all(len(t[2]) == 0 for t in tr[5:])


@pytest.mark.parametrize("n", [3000, 4096])
def test_radius_bounds_state_moves_a_tile_maximum(n):
    """The state of test_collision_screen_radius_bounds: deletions move bodies from tile to tile, so some tile's largest
    |radius| changes between two steps (what unpack_slots has to rebuild, not keep)."""
    cfg, bodies, field = rc.radius_bounds_bodies(n)
    blk = bodies.block.copy()
    cur = n
    prev = rc.expected_tile_rmax(bodies.Radii, n // 128 + 2)
    assert np.isinf(prev).any() and rc.expected_summary(bodies.Positions, bodies.Masses, bodies.Radii, rc.F32) == rc.RADIUS | rc.MASS
    changed = 0
    for s in range(5):
        cur, *_ = ol.port_step(blk, cur, f32(0.2), field, field, f32(0.1), want_events=False)
        now = rc.expected_tile_rmax(ol.carve(blk, cur)[3], n // 128 + 2)
        changed += int((now.view(np.uint32) != prev.view(np.uint32)).sum())
        prev = now
    assert changed > 0 and cur < n


def test_reuse_states_are_what_the_context_test_needs():
    (_, s1, k1), (_, s2, k2), (_, s3, k3) = rc.reuse_states()
    assert (s1.numBodies, s2.numBodies, s3.numBodies) == (8000, 1500, 8192) and s3.numBodies == rc.REUSE_CAPACITY
    assert rc.expected_summary(s1.Positions, s1.Masses, s1.Radii, rc.F32) == rc.UNBOUNDED | rc.RADIUS
    assert np.isnan(s1.Radii).sum() == 1 and rc.expected_tile_rmax(s1.Radii, 64)[:63].min() > 0
    assert rc.expected_summary(s2.Positions, s2.Masses, s2.Radii, rc.F32) == 0 and not s2.Radii.any()
    blk, cur = s1.block.copy(), 8000
    for _ in range(k1):
        cur, *_ = ol.port_step(blk, cur, f32(0.2), rc.REUSE_FIELD, rc.REUSE_FIELD, f32(0.1), want_events=False)
    assert s2.numBodies + 128 < cur < 8000 - 512           # the live bound of the exchange has shrunk, S2 ends tiles earlier ...
    assert s3.numBodies > cur and s2.numBodies < 8000      # ... a re-upload is larger than it; another one smaller than S1
    assert rc.exchange_stride(cur, 2) < rc.exchange_stride(8192, 2)
    blk, cur = s2.block.copy(), 1500
    for _ in range(k2):
        cur, *_ = ol.port_step(blk, cur, f32(0.2), rc.REUSE_FIELD, rc.REUSE_FIELD, f32(0.1), want_events=False)
        assert cur == 1500 and rc.expected_summary(*[ol.carve(blk, cur)[k] for k in (0, 2, 3)], rc.F32) == 0


# ---------------------------------------------------------------------------------------------------------
# planted states (one value at one index of a calm state): what the GPU and host tests rest on
# ---------------------------------------------------------------------------------------------------------
# One planted value can set: nothing (a value just inside a bound); bit 0 (a coordinate at the bound or infinite); bit 2 (a
# coordinate below the floor); bits 0 and 2 together (a NaN coordinate is neither below the bound nor at or above the
# floor); bit 3 (a mass); bit 1 (a radius).  No single value sets bit 1 or 3 with another bit: each rests on one field.
# An fp64 context has bits 0 and 1 only.
REACHABLE = {rc.F32: {0, rc.UNBOUNDED, rc.SMALL, rc.UNBOUNDED | rc.SMALL, rc.MASS, rc.RADIUS},
             rc.F64: {0, rc.UNBOUNDED, rc.RADIUS}}


@pytest.mark.parametrize("precision", [rc.F32, rc.F64])
def test_planted_states_reach_every_summary_one_value_can(precision):
    states = rc.planted_states(precision)
    calm_tiles = np.zeros(rc.PLANT_N // 128 + 2, np.uint32)
    seen = {}
    for s in states:
        b = s["bodies"]
        assert b.numBodies == rc.PLANT_N == 257 and b.precision == precision
        got = rc.expected_summary(b.Positions, b.Masses, b.Radii, precision)
        assert got == s["summary"], "%s: the numpy statement gives %d, the list declares %d" % (s["name"], got, s["summary"])
        seen.setdefault(got, set()).add(s["index"])
        tiles = rc.expected_tile_rmax(b.Radii, len(calm_tiles)).view(np.uint32)
        changed = np.nonzero(tiles != calm_tiles)[0].tolist()
        assert len(changed) == s["tiles_changed"], (s["name"], changed)
        assert changed in ([], [s["index"] // 128]), (s["name"], changed)
        if s["field"] != "r":
            assert s["tiles_changed"] == 0
    assert set(seen) == REACHABLE[precision], sorted(seen)
    for value, where in seen.items():                        # every value at every index: both wave ends, both tile sides
        assert where == set(rc.PLANT_INDICES), (value, sorted(where))
    # each radius of the issue's list either moves one bound or none - and both kinds occur
    assert {s["tiles_changed"] for s in states if s["field"] == "r"} == {0, 1}
    assert {s["field"] for s in states} == {"x", "y", "m", "r"}


def test_wave_straddles_a_tile_as_the_case_says(nb):
    c = rc.case_wave_straddles_a_tile()
    i, j = rc.STRADDLE_PAIR
    lo0, cnt0 = nb.partition(c["n"], 0, 2)
    assert (lo0, cnt0) == (0, 128) and c["n"] == 300 and i < 128 and j < 128
    (n1, blk1, ab1, de1), (n2, _, ab2, de2) = rc.oracle_trajectory(c, want_events=True)
    assert n1 == 299 and de1.tolist() == [j] and ab1.tolist() == [[i, j]]           # the merge happens, inside rank 0's range
    assert n2 == 299 and len(ab2) == 0                                              # and nothing else does
    offset = cnt0 - 1                                        # survivors of rank 0 = where rank 1's slot is unpacked
    assert offset == 127 and offset % 64 != 0 and offset // 128 != (offset + 63) // 128    # that wave covers two tiles
    R1 = ol.carve(blk1, n1)[3]
    assert R1[offset] == f32(0.25) and R1[offset + 1] == f32(0.5) and offset // 128 == 0 and (offset + 1) // 128 == 1
    want = rc.expected_tile_rmax(R1, 5)
    assert want.tolist() == [0.25, 0.5, 0, 0, 0]             # tile 0's bound comes from the straddling wave alone
    assert rc.summaries_of(c) == c["summaries"] and \
        rc.expected_summary(c["bodies"].Positions, c["bodies"].Masses, c["bodies"].Radii, rc.F32) == c["summary0"]
