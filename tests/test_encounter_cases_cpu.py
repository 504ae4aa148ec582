"""CPU tests of the encounter query's definition (tests/encounter_cases.py), of its host half nbody_encounter_finish (plain C,
no GPU) and of what the query claims about the stepper, on the oracle."""
import numpy as np
import pytest

import encounter_cases as ec
import oracle_lib as ol

INF = float("inf")


# ---------------------------------------------------------------------------------------------------------------------
# 1. the standard states prove something about every class
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [0, 1])
@pytest.mark.parametrize("n", ec.STANDARD_N)
def test_standard_state_has_every_class(n, precision):
    P, V, R = ec.standard_state(n, ec.DTYPE_OF[precision])
    enc, info = ec.model_encounters(P, V, R, ec.H)
    now, end_only, missed = ec.classes(enc)
    assert now >= 3 and end_only >= 3 and missed >= 3, (n, now, end_only, missed)
    assert info["pairs"] < n and info["pairs"] == len(enc)
    assert (info["now"], info["missed"]) == (now, missed) and info["end"] >= end_only
    t = enc["t"][enc["t"] != 0.0]
    assert len(np.unique(t)) == len(t)                            # the order of the list never rests on (i, j) but at t = 0
    assert (np.diff(enc["t"]) >= 0).all() and (enc["i"] < enc["j"]).all()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the model against the scalar loop
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", [0.0, 0.5, INF])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 127, 128, 129])
def test_model_equals_the_scalar_loop(n, h):
    for precision in (0, 1):
        P, V, R = ec.standard_state(n, ec.DTYPE_OF[precision])
        got = ec.model_encounters(P, V, R, h)
        ec.assert_same(got, ec.loop_encounters(P, V, R, h), "n %d h %g" % (n, h))
        enc, info = got
        if h == 0.0:                                              # swept == now, and end == now for finite velocities
            assert info["pairs"] == info["now"] == info["end"] and info["missed"] == 0 and (enc["t"] == 0.0).all()
        if h == INF:
            assert info["end"] == 0 and info["pairs"] == info["now"] + info["missed"]
            assert np.isfinite(enc["t"]).all()                    # every pair on a collision course has its time


def test_first_contacts(nb):
    P, V, R = ec.standard_state(300, np.float32)
    enc, _ = ec.model_encounters(P, V, R, ec.H)
    want, got = ec.first_contacts(enc, 300), nb.first_contacts(enc, 300)
    for k in ("t", "partner", "count"):
        assert np.array_equal(got[k], want[k]), k
    assert got["count"].sum() == 2 * len(enc) and (got["partner"] >= 0).sum() == (got["count"] > 0).sum() > 100
    empty = nb.first_contacts(enc[:0], 5)
    assert np.isinf(empty["t"]).all() and (empty["partner"] == -1).all() and (empty["count"] == 0).all()


# ---------------------------------------------------------------------------------------------------------------------
# 3. hand cases
# ---------------------------------------------------------------------------------------------------------------------
def pair(x0, x1, v0, v1, r=1.0, y1=0.0):
    return np.array([[x0, 0.0], [x1, y1]]), np.array([[v0, 0.0], [v1, 0.0]]), np.array([r, r])


@pytest.mark.parametrize("h,want", [(5.0, None), (9.0, (9.0, ec.END)), (10.0, (9.0, ec.END)), (20.0, (9.0, 0)), (INF, (9.0, 0))])
def test_head_on_pair(h, want):
    """x = -+10, r = 1, v = +-1: dx = 20, dvx = -2, c = 396, b = -40, a = 4, disc = 16: contact at 396 / (4 + 40) = 9; the
    centres meet at 10 and part again; at 11 the bodies separate."""
    for model in (ec.model_encounters, ec.loop_encounters):
        enc, info = model(*pair(-10.0, 10.0, 1.0, -1.0), h)
        if want is None:
            assert len(enc) == 0 and info["pairs"] == 0
        else:
            assert len(enc) == 1 and (enc["t"][0], enc["i"][0], enc["j"][0], enc["flags"][0]) == (want[0], 0, 1, want[1])
            assert (info["now"], info["end"], info["missed"]) == (0, int(want[1] == ec.END), int(want[1] == 0))


def test_receding_grazing_and_resting_pairs():
    for h in (0.0, 1.0, 100.0, INF):
        enc, _ = ec.model_encounters(*pair(-10.0, 10.0, -1.0, 1.0), h)               # receding: b > 0
        assert len(enc) == 0
    # grazing: the centres pass at distance exactly s = 2, disc = (b*b) - (a*c) = 0: swept, at the time of closest approach
    P, V, R = pair(-10.0, 10.0, 1.0, -1.0, y1=2.0)
    enc, info = ec.model_encounters(P, V, R, 20.0)
    assert len(enc) == 1 and enc["t"][0] == 10.0 and enc["flags"][0] == 0 and info["missed"] == 1
    enc, info = ec.model_encounters(P, V, R, 10.0)                                   # closest approach AT h: end holds, e2 = 4 <= 4
    assert len(enc) == 1 and enc["t"][0] == 10.0 and enc["flags"][0] == ec.END
    P[1, 1] = 2.0 + 1e-9                                                             # a billionth further out: disc < 0
    assert len(ec.model_encounters(P, V, R, 20.0)[0]) == 0
    # at rest and overlapping: NOW and END whatever h is (a = b = 0; dvx * inf = NaN takes END away at h = +inf)
    for h, flags in ((0.0, ec.NOW | ec.END), (3.0, ec.NOW | ec.END), (INF, ec.NOW)):
        enc, info = ec.model_encounters(*pair(0.0, 1.5, 0.0, 0.0), h)
        assert len(enc) == 1 and enc["t"][0] == 0.0 and enc["flags"][0] == flags and info["now"] == 1
    assert len(ec.model_encounters(*pair(0.0, 2.5, 0.0, 0.0), INF)[0]) == 0         # at rest and apart: never


def test_nan_and_huge_inputs():
    P, V, R = ec.standard_state(129, np.float64)
    base, _ = ec.model_encounters(P, V, R, ec.H)
    k = int(base["i"][base["flags"] == 0][0])                     # a body of a missed pair

    def without(enc, body):
        return enc[(enc["i"] != body) & (enc["j"] != body)]

    for what, arrays in (("coordinate", (0, (k, 1))), ("radius", (2, (k,)))):
        S = [P.copy(), V.copy(), R.copy()]
        S[arrays[0]][arrays[1]] = np.nan
        for model in (ec.model_encounters, ec.loop_encounters):
            enc, info = model(*S, ec.H)
            assert np.array_equal(enc, without(base, k)), what    # exactly that body's pairs are gone
    Vn = V.copy()
    Vn[k, 0] = np.nan                                             # a NaN velocity: end and mid fail, `now` does not read it
    enc, _ = ec.model_encounters(P, Vn, R, ec.H)
    ec.assert_same((enc, ec._info(129, enc["flags"], ec.H)), ec.loop_encounters(P, Vn, R, ec.H))
    kept = base[((base["i"] == k) | (base["j"] == k)) & ((base["flags"] & ec.NOW) != 0)]
    assert len(enc) == len(without(base, k)) + len(kept)
    assert np.array_equal(without(enc, k), without(base, k))
    # 1e200: d2 = +inf, c = +inf, disc = NaN: not swept unless the end positions are close again
    Ph, Vh = P.copy(), V.copy()
    Ph[5], Vh[7] = [1e200, 3.0], [1e200, -1e200]
    for h in (0.0, ec.H, INF):
        ec.assert_same(ec.model_encounters(Ph, Vh, R, h), ec.loop_encounters(Ph, Vh, R, h), "1e200, h %g" % h)
    enc, _ = ec.model_encounters(Ph, Vh, R, ec.H)
    assert not ((enc["i"] == 5) | (enc["j"] == 5)).any() and np.array_equal(without(without(enc, 5), 7), without(without(base, 5), 7))
    Pe, Ve, Re = pair(0.0, 1e200, 0.0, -1e200)                    # ... as here: ex = 1e200 + (-1e200 * 1) = 0: END, with t = h
    enc, info = ec.model_encounters(Pe, Ve, Re, 1.0)
    assert len(enc) == 1 and enc["flags"][0] == ec.END and enc["t"][0] == 1.0
    ec.assert_same((enc, info), ec.loop_encounters(Pe, Ve, Re, 1.0))


# ---------------------------------------------------------------------------------------------------------------------
# 4. nbody_encounter_finish: the host half, through ctypes
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", [0.0, 0.5, INF])
def test_finish_matches_the_model(nb, h):
    assert nb.ENCOUNTER_RAW_DTYPE == ec.RAW_DTYPE and nb.ENCOUNTER_RECORD_DTYPE == ec.RECORD_DTYPE
    assert (ec.RAW_DTYPE.itemsize, ec.RECORD_DTYPE.itemsize, ec.INFO_DTYPE.itemsize) == (40, 24, 48)
    for n, precision in ((300, 0), (1000, 1)):
        P, V, R = ec.standard_state(n, ec.DTYPE_OF[precision])
        enc, info, raw = ec.model_encounters(P, V, R, h, want_raw=True)
        assert len(raw) == info["pairs"] > 0
        rng = np.random.default_rng(3)
        for order in (np.arange(len(raw)), np.arange(len(raw))[::-1], rng.permutation(len(raw))):   # the device appends in any order
            shuffled = raw[order].copy()
            swap = rng.integers(0, 2, len(raw)).astype(bool)      # and either orientation of the pair
            shuffled["i"][swap], shuffled["j"][swap] = raw["j"][order][swap], raw["i"][order][swap]
            shuffled["flags"] |= np.uint32(0xF0)                  # bits that are not flags are not read
            got = nb.encounter_finish(shuffled, h)
            ec.assert_same((got, info), (enc, info), "n %d h %g" % (n, h))


def test_finish_breaks_ties_by_index_and_checks_arguments(nb):
    raw = np.zeros(6, dtype=ec.RAW_DTYPE)
    raw["i"], raw["j"] = [7, 2, 2, 9, 0, 4], [8, 5, 3, 1, 6, 4 + 1]
    raw["flags"] = [ec.NOW, 0, ec.NOW, ec.END, 0, ec.NOW | ec.END]
    raw["c"], raw["b"], raw["disc"] = 396.0, -40.0, 16.0
    got = nb.encounter_finish(raw, 20.0)
    assert got["t"].tolist() == [0.0, 0.0, 0.0, 9.0, 9.0, 9.0]
    assert list(zip(got["i"].tolist(), got["j"].tolist())) == [(2, 3), (4, 5), (7, 8), (0, 6), (1, 9), (2, 5)]
    assert got["flags"].tolist() == [ec.NOW, ec.NOW | ec.END, ec.NOW, 0, ec.END, 0]
    assert nb.encounter_finish(raw, 4.0)["t"].tolist() == [0.0, 0.0, 0.0, 4.0, 4.0, 4.0]          # min(9, h)
    raw["b"] = 1.0                                                # not approaching: t = h
    assert nb.encounter_finish(raw, INF)["t"].tolist() == [0.0, 0.0, 0.0, INF, INF, INF]
    assert len(nb.encounter_finish(raw[:0], 1.0)) == 0
    out = np.zeros(6, dtype=ec.RECORD_DTYPE)
    fn = nb.lib.nbody_encounter_finish
    assert fn(None, 0, 1.0, None) == 0
    for args in ((raw.ctypes.data, -1, 1.0, out.ctypes.data), (None, 6, 1.0, out.ctypes.data), (raw.ctypes.data, 6, 1.0, None),
                 (raw.ctypes.data, 6, -1.0, out.ctypes.data), (raw.ctypes.data, 6, float("nan"), out.ctypes.data)):
        assert fn(*args) == -1
    assert not out.view(np.uint8).any()


def test_finish_under_sanitizers(tmp_path):
    """nbody_encounters.c with a stand-alone driver under AddressSanitizer + UBSan: exact-size heap buffers, every count from
    0 to 4097, every kind of horizon.  Host code only."""
    import os
    import shutil
    import subprocess
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "ppa-nbody-collisions_amd", "csrc")
    exe = str(tmp_path / "encounters_driver")
    cmd = ["gcc", "-std=gnu11", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-Wall", "-Wextra", "-ffp-contract=off", "-I" + os.path.join(root, "include"), "-I" + csrc,
           os.path.join(root, "tests", "host_asan", "encounters_driver.c"), os.path.join(csrc, "nbody_encounters.c"),
           os.path.join(csrc, "nbody_error.c"), "-o", exe, "-lm"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip("sanitizer runtime not available: " + r.stderr[-200:])
    assert r.returncode == 0, r.stderr[-2000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-3000:]
    assert p.returncode == 0 and "encounters ok" in p.stdout, (p.returncode, p.stdout, p.stderr[-2000:])


# ---------------------------------------------------------------------------------------------------------------------
# 5. the tie to the stepper, on the oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("semantics", [ol.LITERAL, ol.CLEAN])
def test_flags_mean_what_the_stepper_does(semantics):
    """Six bodies of mass 2 and 1 in turns - of two bodies that overlap the heavier absorbs and the lighter is deleted; equal
    masses would absorb each other and both stay - (G m / d^2 dt ~ 1e-11: no velocity changes in fp32) in a field of +-1e6 (no wall), so one fp32 step
    moves every body by fl(x + fl(dt v)).  Three pairs 1000 apart, every threshold cleared by far more than 1e-3 of s = 2:
      bodies 0, 1: 1.5 apart, at rest relative to each other      NOW: d2 = 2.25 <= 4                  merges in step 1
      bodies 2, 3: 4 apart, closing at 12: 1.6 apart at dt         END only: d2 = 16, e2 = 2.56         merges in step 2
      bodies 4, 5: 3 apart, closing at 30: 3 apart again at dt     missed: d2 = e2 = 9, contact at 1/30 survives both steps"""
    dt = np.float32(0.2)
    P = np.array([[1000.0, 0.0], [1001.5, 0.0], [2000.0, 0.0], [2004.0, 0.0], [3000.0, 0.0], [3003.0, 0.0]])
    V = np.array([[10.0, 5.0], [10.0, 5.0], [6.0, 10.0], [-6.0, 10.0], [15.0, -10.0], [-15.0, -10.0]])
    M, R = np.array([2.0, 1.0, 2.0, 1.0, 2.0, 1.0]), np.ones(6)
    enc, info = ec.model_encounters(P, V, R, float(dt))
    assert (info["pairs"], info["now"], info["end"], info["missed"]) == (3, 1, 2, 1)     # the resting pair overlaps at both ends
    by_pair = {(int(e["i"]), int(e["j"])): (float(e["t"]), int(e["flags"])) for e in enc}
    assert by_pair[(0, 1)] == (0.0, ec.NOW | ec.END)
    assert by_pair[(2, 3)][1] == ec.END and abs(by_pair[(2, 3)][0] - 2.0 / 12.0) < 1e-6
    assert by_pair[(4, 5)][1] == 0 and abs(by_pair[(4, 5)][0] - 1.0 / 30.0) < 1e-6
    blk = ol.make_block(P, V, M, R)
    n1, _, absorbed1, _, _ = ol.port_step(blk, 6, dt, 1000000, 1000000, np.float32(0.0), semantics)
    assert n1 == 5 and absorbed1.tolist() == [[0, 1]]   # NOW: at once, and nothing else
    P1, V1, _, R1 = (np.asarray(a, dtype=np.float64) for a in ol.carve(blk, n1))
    enc1, info1 = ec.model_encounters(P1, V1, R1, float(dt))
    now1 = enc1[(enc1["flags"] & ec.NOW) != 0]
    assert len(now1) == 1 and P1[now1["i"][0], 0] > 2000.0 and P1[now1["j"][0], 0] < 2010.0   # the END pair overlaps now
    n2, _, absorbed2, _, _ = ol.port_step(blk, n1, dt, 1000000, 1000000, np.float32(0.0), semantics)
    assert n2 == 4 and len(absorbed2) == 1                        # END: at the next step; the missed pair: no event in either
    assert sorted(absorbed2[0].tolist()) == sorted([int(now1["i"][0]), int(now1["j"][0])])
    P2, V2, _, _ = ol.carve(blk, n2)
    far = P2[:, 0] > 2900.0                                       # bodies 4 and 5 passed through each other, untouched
    assert far.sum() == 2 and sorted(V2[far, 0].tolist()) == [-15.0, 15.0]
    assert sorted(P2[far, 0].tolist()) == [float(np.float32(3003.0) + 2 * np.float32(-3.0)), float(np.float32(3000.0) + 2 * np.float32(3.0))]
