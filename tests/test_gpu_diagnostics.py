"""Diagnostics of the resident state (nbody_get_diagnostics / nbody_group_diagnostics) on the MI355X.

The oracle evaluates every term in np.longdouble (x86-64 80-bit: eps 2^-63) and is called "exact" here.  Tolerances are
summation error bounds with u = 2^-53, not fitted to runs:
  * phi_i: every term has one sign and is within 4 u of its exact value, so any order of the n-1 adds and the product with
    G stay within (n + 4) u |phi_i|;
  * a total of n products: (n + 8) u sum |products|; the potential sums n products m_i phi_i whose factors phi_i carry
    their own (n + 4) u: (2 n + 8) u sum |m_i phi_i|.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
G = float(np.float32(6.67408e-11))
LD = np.longdouble


def setup_module(module):
    assert np.finfo(np.longdouble).eps < 1e-18, "the oracle needs an 80-bit long double (x86-64)"


def state_arrays(b):
    return (np.asarray(b.Positions, dtype=np.float64), np.asarray(b.Velocities, dtype=np.float64),
            np.asarray(b.Masses, dtype=np.float64))


def exact_phi(P, M, rows):
    """phi_i for the given rows, in long double; pairs at distance 0 (and j == i) left out; also the coincident count."""
    x, y, m = P[:, 0].astype(LD), P[:, 1].astype(LD), M.astype(LD)
    phi = np.zeros(len(rows), dtype=LD)
    coincident = 0
    for a in range(0, len(rows), 16):
        r = np.asarray(rows[a:a + 16])
        dx = x[None, :] - x[r, None]
        dy = y[None, :] - y[r, None]
        zero = (dx == 0) & (dy == 0)
        coincident += int(zero.sum()) - len(r)
        d = np.sqrt(dx * dx + dy * dy)
        d[zero] = 1
        t = m[None, :] / d
        t[zero] = 0
        phi[a:a + 16] = -LD(G) * t.sum(axis=1)
    return phi, coincident


def check_phi(got, want, n, what=""):
    err = np.abs(got.astype(LD) - want)
    bound = (n + 4) * LD(U) * np.abs(want)
    bad = np.nonzero(err > bound)[0]
    assert len(bad) == 0, (what, bad[:8], got[bad[:8]], want[bad[:8]])


def check_totals(d, P, V, M, phi_for_potential, what=""):
    n = len(M)
    x, y, vx, vy, m = (a.astype(LD) for a in (P[:, 0], P[:, 1], V[:, 0], V[:, 1], M))
    k = (n + 8) * LD(U)

    def close(got, want, scale, name, bound=None):
        b = k * scale if bound is None else bound
        assert abs(LD(got) - want) <= b, (what, name, got, float(want), float(b))

    assert d["n_bodies"] == n
    mass = m.sum()
    close(d["mass"], mass, np.abs(m).sum(), "mass")
    close(d["momentum"][0], (m * vx).sum(), np.abs(m * vx).sum(), "px")
    close(d["momentum"][1], (m * vy).sum(), np.abs(m * vy).sum(), "py")
    for c, (q, name) in enumerate(((x, "cx"), (y, "cy"))):
        want = (m * q).sum() / mass
        b = (k * np.abs(m * q).sum() + abs(want) * k * np.abs(m).sum()) / abs(mass) + LD(U) * abs(want)
        close(d["center_of_mass"][c], want, None, name, bound=b)
    close(d["angular_momentum"], (m * (x * vy - y * vx)).sum(), (np.abs(m) * (np.abs(x * vy) + np.abs(y * vx))).sum(), "L")
    close(d["kinetic"], LD(0.5) * (m * (vx * vx + vy * vy)).sum(), LD(0.5) * (np.abs(m) * (vx * vx + vy * vy)).sum(), "K")
    pw = m * phi_for_potential.astype(LD)
    close(d["potential"], LD(0.5) * pw.sum(), None, "potential",
          bound=(2 * n + 8) * LD(U) * LD(0.5) * np.abs(pw).sum())


def diag_bits(d):
    vals = [d["step"], d["n_bodies"], d["coincident_pairs"]]
    for k in ("mass", "momentum", "center_of_mass", "angular_momentum", "kinetic", "potential"):
        v = d[k] if isinstance(d[k], tuple) else (d[k],)
        vals += [int(np.float64(e).view(np.uint64)) for e in v]
    if "phi" in d:
        vals.append(d["phi"].view(np.uint64).tobytes())
    return tuple(vals)


def bodies_with_velocities(nb, n, precision, seed=7, field=None):
    kw = {} if field is None else {"fieldWidth": field, "fieldHeight": field}
    cfg = nb.stock_config(particleCount=n, **kw)
    b = nb.init_bodies(cfg, precision)
    rng = np.random.default_rng(seed)
    b.Velocities[:] = rng.uniform(-3, 3, size=(n, 2)).astype(b.dtype)
    return cfg, b


# ---------------------------------------------------------------------------------------------------------------------
# 1. closed forms
# ---------------------------------------------------------------------------------------------------------------------
def test_two_bodies_closed_form(nb):
    b = nb.BodiesData.from_arrays([[0.0, 0.0], [3.0, 4.0]], [[0, 0], [0, 0]], [2.0, 5.0], [0, 0], nb.F64)
    st = nb.Stepper(capacity=2, precision=nb.F64, timestep=0.2, growthRate=0.1, fieldWidth=100, fieldHeight=100)
    st.upload(b)
    d = st.diagnostics(potential=True)
    want = -LD(G) * 2 * 5 / 5
    assert abs(LD(d["potential"]) - want) <= 5 * LD(U) * abs(want)
    assert abs(LD(d["phi"][0]) - (-LD(G) * 5 / 5)) <= 5 * LD(U) * LD(G)
    assert abs(LD(d["phi"][1]) - (-LD(G) * 2 / 5)) <= 5 * LD(U) * LD(G) * 2 / 5
    assert d["coincident_pairs"] == 0 and d["n_bodies"] == 2 and d["step"] == 0
    st.close()


@pytest.mark.parametrize("precision", [0, 1])
def test_two_body_cases_across_exponent_ranges(nb, precision):
    """200 random two-body states (one context, re-uploaded): phi within 5 u of -G m_j / r exactly (4 u for the term, 1 for
    the product with G).  This checks the per-term accuracy of the refined v_rsq_f64 chain."""
    rng = np.random.default_rng(11 + precision)
    span = 60 if precision == nb.F32 else 240           # coordinates and masses 2^[-span/2, span/2]
    st = nb.Stepper(capacity=2, precision=precision, timestep=0.2, growthRate=0.1, fieldWidth=100, fieldHeight=100)
    dt = np.float64 if precision == nb.F64 else np.float32
    for case in range(200):
        P = (rng.choice([-1, 1], size=(2, 2)) * np.exp2(rng.uniform(-span / 2, span / 2, size=(2, 2)))).astype(dt)
        M = np.exp2(rng.uniform(-span / 2, span / 2, size=2)).astype(dt)
        st.upload(nb.BodiesData.from_arrays(P, np.zeros((2, 2)), M, [0, 0], precision))
        d = st.diagnostics(potential=True)
        P64, M64 = P.astype(np.float64), M.astype(np.float64)
        r = np.sqrt((LD(P64[1, 0]) - LD(P64[0, 0])) ** 2 + (LD(P64[1, 1]) - LD(P64[0, 1])) ** 2)
        want = np.array([-LD(G) * LD(M64[1]) / r, -LD(G) * LD(M64[0]) / r])
        err = np.abs(d["phi"].astype(LD) - want)
        assert np.all(err <= 5 * LD(U) * np.abs(want)), (case, P, M, d["phi"], want, err / (LD(U) * np.abs(want)))
    st.close()


def test_regular_polygon_and_square(nb):
    # a square with exact coordinates: phi = -G m (2 / (R sqrt 2) + 1 / (2 R)) for every vertex
    R, m = 3.0, 7.0
    P = [[R, 0], [0, R], [-R, 0], [0, -R]]
    st = nb.Stepper(capacity=64, precision=nb.F64, timestep=0.2, growthRate=0.1, fieldWidth=100, fieldHeight=100)
    st.upload(nb.BodiesData.from_arrays(P, np.zeros((4, 2)), [m] * 4, [0] * 4, nb.F64))
    d = st.diagnostics(potential=True)
    want = -LD(G) * LD(m) * (2 / (LD(R) * np.sqrt(LD(2))) + 1 / (2 * LD(R)))
    assert np.all(np.abs(d["phi"].astype(LD) - want) <= 8 * LD(U) * abs(want)), d["phi"]
    assert abs(LD(d["potential"]) - 2 * LD(m) * want) <= 16 * LD(U) * abs(2 * m * want)
    assert d["center_of_mass"] == (0.0, 0.0) and d["mass"] == 4 * m
    # k equal masses on a circle: sum_{j=1}^{k-1} 1 / (2 R sin(pi j / k)); the vertices are rounded to fp64, which moves
    # each distance by a few u
    k = 24
    ang = 2 * np.pi * np.arange(k) / k
    P = np.stack([R * np.cos(ang), R * np.sin(ang)], axis=1)
    st.upload(nb.BodiesData.from_arrays(P, np.zeros((k, 2)), [m] * k, [0] * k, nb.F64))
    d = st.diagnostics(potential=True)
    j = np.arange(1, k, dtype=LD)
    want = -LD(G) * LD(m) * (1 / (2 * LD(R) * np.sin(np.pi * j / k))).sum()
    assert np.all(np.abs(d["phi"].astype(LD) - want) <= (k + 16) * LD(U) * abs(want)), d["phi"] - float(want)
    st.close()


def test_single_body(nb):
    st = nb.Stepper(capacity=4, precision=nb.F32, timestep=0.2, growthRate=0.1, fieldWidth=100, fieldHeight=100)
    st.upload(nb.BodiesData.from_arrays([[1.5, -2.0]], [[0.5, 0.25]], [3.0], [1.0], nb.F32))
    d = st.diagnostics(potential=True)
    assert d["phi"][0] == 0 and d["potential"] == 0 and d["coincident_pairs"] == 0
    assert d["mass"] == 3.0 and d["momentum"] == (1.5, 0.75) and d["center_of_mass"] == (1.5, -2.0)
    assert d["angular_momentum"] == 3.0 * (1.5 * 0.25 - (-2.0) * 0.5)
    assert d["kinetic"] == 0.5 * 3.0 * (0.25 + 0.0625)
    st.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. against the exact oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [0, 1])
def test_against_exact_oracle(nb, precision):
    for n in (2, 100, 127, 128, 129, 1000, 4096):
        cfg, b = bodies_with_velocities(nb, n, precision, seed=n)
        st = nb.Stepper(cfg, precision=precision)
        st.upload(b)
        d = st.diagnostics(potential=True)
        P, V, M = state_arrays(b)
        want, coincident = exact_phi(P, M, np.arange(n))
        check_phi(d["phi"], want, n, "n=%d" % n)
        assert d["coincident_pairs"] == coincident
        check_totals(d, P, V, M, want, "n=%d" % n)
        st.close()


@pytest.mark.parametrize("precision", [0, 1])
def test_stepped_state_with_collisions(nb, precision):
    """The stock initial condition in a 5000-wide field after 5 steps (bodies absorbed, velocities from the forces):
    against the downloaded state."""
    cfg = nb.stock_config(particleCount=3000, fieldWidth=5000, fieldHeight=5000)
    st = nb.Stepper(cfg, precision=precision)
    st.upload(nb.init_bodies(cfg, precision))
    st.step(5)
    d = st.diagnostics(potential=True)
    b = st.download()
    assert b.numBodies < 3000 and d["step"] == 5
    P, V, M = state_arrays(b)
    want, coincident = exact_phi(P, M, np.arange(b.numBodies))
    check_phi(d["phi"], want, b.numBodies)
    assert d["coincident_pairs"] == coincident
    check_totals(d, P, V, M, want)
    st.close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. coincident bodies
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [0, 1])
def test_coincident_bodies(nb, precision):
    """The duplicated positions of test_coincident_bodies_at_zero_radii: the ordered-pair count is exact, phi and the
    potential are finite and match the oracle with those pairs left out."""
    n = 4096
    cfg = nb.stock_config(particleCount=n, minRadius=0.0, maxRadius=0.0)
    b = nb.init_bodies(cfg, precision)
    P = b.Positions
    P[70] = P[5]
    P[200] = P[130]
    P[1000] = P[300]
    P[4090] = P[3]
    P[2000] = P[2001] = P[2002]
    P[2500] = P[2600]
    P[129] = P[128]
    st = nb.Stepper(cfg, precision=precision)
    st.upload(b)
    d = st.diagnostics(potential=True)
    Pd, V, M = state_arrays(b)
    want, coincident = exact_phi(Pd, M, np.arange(n))
    assert coincident == 2 * 6 + 6 and d["coincident_pairs"] == coincident
    assert np.all(np.isfinite(d["phi"])) and np.isfinite(d["potential"])
    check_phi(d["phi"], want, n)
    check_totals(d, Pd, V, M, want)
    st.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. headline size, sampled
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision,n", [(0, 262144), (1, 131072)])
def test_headline_size_sampled(nb, precision, n):
    cfg, b = bodies_with_velocities(nb, n, precision, seed=3)
    st = nb.Stepper(cfg, precision=precision)
    st.upload(b)
    d = st.diagnostics(potential=True)
    P, V, M = state_arrays(b)
    rows = np.sort(np.random.default_rng(5).choice(n, size=256, replace=False))
    want, _ = exact_phi(P, M, rows)
    check_phi(d["phi"][rows], want, n)
    # totals: the O(N) ones exactly; the potential against 1/2 sum m_i phi_i of the device's phi (checked on the sample)
    check_totals(d, P, V, M, d["phi"])
    assert np.all(np.isfinite(d["phi"]))
    st.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. partition independence, determinism
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [65536, 100003])
def test_partition_independence(nb, n):
    """world 1, 2, 3, 8 on one GPU (peer copies), the single-rank RCCL path (force_comm) and a plain context: the same
    bits, call after call."""
    cfg, b = bodies_with_velocities(nb, n, nb.F32, seed=n, field=20000)
    plain = nb.Stepper(cfg)
    plain.upload(b)
    plain.step(2)
    ref = diag_bits(plain.diagnostics(potential=True))
    assert ref == diag_bits(plain.diagnostics(potential=True))
    plain.close()
    for world in (1, 2, 3, 8):
        grp = nb.StepperGroup(world, cfg=cfg)
        grp.upload(b)
        grp.step(2)
        assert diag_bits(grp.diagnostics(potential=True)) == ref, world
        assert diag_bits(grp.diagnostics(potential=True)) == ref, world
        grp.close()
    rc = nb.Stepper(cfg, comm_id=nb.comm_unique_id(), force_comm=True)
    rc.upload(b)
    rc.step(2)
    assert diag_bits(rc.diagnostics(potential=True)) == ref
    assert diag_bits(rc.diagnostics()) == ref[:-1]
    rc.close()


# ---------------------------------------------------------------------------------------------------------------------
# 6. no effect on stepping
# ---------------------------------------------------------------------------------------------------------------------
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


@pytest.mark.parametrize("precision,world", [(0, 0), (1, 0), (0, 3)])
def test_no_effect_on_stepping(nb, precision, world):
    cfg = nb.stock_config(particleCount=4000, fieldWidth=5000, fieldHeight=5000)
    b = nb.init_bodies(cfg, precision)

    def make():
        return nb.StepperGroup(world, cfg=cfg, precision=precision) if world else nb.Stepper(cfg, precision=precision)

    a = make()
    a.upload(b)
    a.step(10)
    want = a.download()
    a.close()
    c = make()
    c.upload(b)
    c.step(5)
    c.diagnostics(potential=True)
    c.step(5)
    d = c.diagnostics()
    got = c.download()
    c.close()
    assert d["step"] == 10 and d["n_bodies"] == got.numBodies
    assert got.numBodies == want.numBodies and np.array_equal(_bits(got.block), _bits(want.block))


# ---------------------------------------------------------------------------------------------------------------------
# 7. errors
# ---------------------------------------------------------------------------------------------------------------------
def test_errors(nb):
    cfg = nb.stock_config(particleCount=1000)
    st = nb.Stepper(cfg)
    with pytest.raises(nb.NbodyError) as e:
        st.diagnostics()
    assert e.value.status == -9 and "before nbody_upload" in str(e.value)
    st.close()
    grp = nb.StepperGroup(2, cfg=cfg)
    grp.upload(nb.init_bodies(cfg))
    d = nb.Diag()
    assert nb.lib.nbody_get_diagnostics(grp.ranks[1]._ctx, ctypes.byref(d), None) == -9
    assert b"nbody_group_diagnostics" in nb.lib.nbody_last_error_string()
    # ranks that were not stepped together
    nb.lib.nbody_group_step(grp._arr, 2, 1)
    grp.ranks[1].upload(nb.init_bodies(cfg))
    with pytest.raises(nb.NbodyError) as e:
        grp.diagnostics()
    assert e.value.status == -9
    grp.close()


# ---------------------------------------------------------------------------------------------------------------------
# 8. CLI
# ---------------------------------------------------------------------------------------------------------------------
def test_cli_diagnostics_lines(nb, tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(root, "ppa-nbody-collisions_amd", "nbody")
    cfg = nb.stock_config(particleCount=1024, totalIterations=20)
    nb.write_config(str(tmp_path / "nbodyConfig.txt"), cfg)
    r = subprocess.run([exe, "--diagnostics", "5"], cwd=str(tmp_path), capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.decode().splitlines() if ln.startswith("diag ")]
    parsed = [dict(kv.split("=") for kv in ln.split()[1:]) for ln in lines]
    assert [int(p["step"]) for p in parsed] == [0, 5, 10, 15, 20]
    st = nb.Stepper(cfg)
    st.upload(nb.init_bodies(cfg))
    done = 0
    for p in parsed:
        st.step(int(p["step"]) - done)
        done = int(p["step"])
        d = st.diagnostics()
        assert int(p["n"]) == d["n_bodies"] and int(p["coincident"]) == d["coincident_pairs"]
        got = [float(p[k]) for k in ("mass", "px", "py", "cx", "cy", "L", "kinetic", "potential")]
        want = [d["mass"], d["momentum"][0], d["momentum"][1], d["center_of_mass"][0], d["center_of_mass"][1],
                d["angular_momentum"], d["kinetic"], d["potential"]]
        assert np.array_equal(np.array(got).view(np.uint64), np.array(want).view(np.uint64)), (p, d)
    st.close()


# ---------------------------------------------------------------------------------------------------------------------
# 9. the bits, pinned
# ---------------------------------------------------------------------------------------------------------------------
# The three potential kernels (diag_potential, batch_diag_potential, track_potential) share one walk over j and host and
# device share one finish, so the cross-checks between them compare a function with itself.  tests/golden/diag_pins.npz
# holds states and what the library gave for them when the fixture was recorded (tests/golden/make_diag_pins.py): the bits
# may not move.  n = 1: a lone body; 129: a j tile of one body; 256: exactly one full workgroup of rows; 300: an odd tile
# count, a partial last tile and a partial second workgroup, with bodies 5 and 200 at one position (general rows, the
# coincident count).
PINS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "diag_pins.npz")
PIN_SIZES = (1, 129, 256, 300)
PIN_BATCH_SIZES = (0, 1, 129, 256, 300)
PIN_BATCH_CAPACITY = 384
PIN_TRACK_IDS = (0, 5, 127, 128, 200, 255, 256, 299)
PIN_TRACK_KEYS = ("step", "n_bodies", "index", "x", "y", "vx", "vy", "m", "r", "phi")


def pin_tag(nb, precision):
    return "f64" if precision == nb.F64 else "f32"


def pin_bits(a):
    """Any array as its bit pattern: what the fixture stores and what the test compares."""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]).copy()


def pin_bodies(nb, pins, precision, n):
    """The recorded input state: the [P | V | M | R] block as stored, never derived again."""
    if n == 0:
        return nb.BodiesData(0, precision)
    dt = np.float64 if precision == nb.F64 else np.float32
    return nb.BodiesData.from_block(pins["in_%s_n%d" % (pin_tag(nb, precision), n)].view(dt), n, precision)


def pin_record(d):
    return np.array(diag_bits({k: v for k, v in d.items() if k != "phi"}), dtype=np.uint64)


def pin_stepper(nb, pins, precision, n):
    """-> {key: bits} of diagnostics(potential=True) straight after the upload."""
    tag = "ctx_%s_n%d" % (pin_tag(nb, precision), n)
    with nb.Stepper(nb.stock_config(particleCount=n), precision=precision) as st:
        st.upload(pin_bodies(nb, pins, precision, n))
        d = st.diagnostics(potential=True)
    return {tag + "_rec": pin_record(d), tag + "_phi": pin_bits(d["phi"])}


def pin_batch(nb, pins):
    """One fp32 batch of PIN_BATCH_SIZES: the records with and without phi (two instantiations), phi, and a track row."""
    out = {}
    cfg = nb.stock_config(particleCount=PIN_BATCH_CAPACITY)
    with nb.StepperBatch(len(PIN_BATCH_SIZES), PIN_BATCH_CAPACITY, cfg=cfg, track_ids=True) as b:
        b.upload([pin_bodies(nb, pins, nb.F32, n) for n in PIN_BATCH_SIZES])
        ds = b.diagnostics(potential=True)
        out["batch_rec"] = np.stack([pin_record(d) for d in ds])
        out["batch_rec_without_phi"] = np.stack([pin_record(d) for d in b.diagnostics()])
        for n, d in zip(PIN_BATCH_SIZES, ds):
            out["batch_phi_n%d" % n] = pin_bits(d["phi"])
        b.reserve_tracks(1, ids=list(PIN_TRACK_IDS), potential=True)
        b.record_tracks()
        t = b.tracks()
    for k in PIN_TRACK_KEYS:
        out["batch_track_" + k] = pin_bits(t[k])
    return out


def pin_tracks(nb, pins, precision):
    """One track record with the potential on the n = 300 state."""
    n = PIN_SIZES[-1]
    with nb.Stepper(nb.stock_config(particleCount=n), precision=precision, track_ids=True) as st:
        st.reserve_tracks(1, ids=list(PIN_TRACK_IDS), potential=True)
        st.upload(pin_bodies(nb, pins, precision, n))
        st.record_tracks()
        t = st.tracks()
    return {"track_%s_%s" % (pin_tag(nb, precision), k): pin_bits(t[k]) for k in PIN_TRACK_KEYS}


def check_pins(pins, got):
    assert got, "nothing was computed"
    for key, bits in got.items():
        want = pins[key]
        assert want.dtype == bits.dtype and want.shape == bits.shape, (key, want.dtype, bits.dtype, want.shape, bits.shape)
        assert np.array_equal(want, bits), (key, np.nonzero(want != bits)[0][:8])


@pytest.fixture(scope="module")
def pins():
    with np.load(PINS) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("n", PIN_SIZES)
@pytest.mark.parametrize("precision", [0, 1])
def test_pinned_bits_stepper(nb, pins, precision, n):
    check_pins(pins, pin_stepper(nb, pins, precision, n))


def test_pinned_bits_batch(nb, pins):
    got = pin_batch(nb, pins)
    check_pins(pins, got)
    # the record of a system does not depend on whether phi is kept, and an empty system reads NaN for its centre
    assert np.array_equal(got["batch_rec"], got["batch_rec_without_phi"])
    assert got["batch_rec"][0, 1] == 0 and got["batch_rec"][4, 2] == 2          # n_bodies of system 0; the pair (5, 200) twice


@pytest.mark.parametrize("precision", [0, 1])
def test_pinned_bits_tracks(nb, pins, precision):
    got = pin_tracks(nb, pins, precision)
    check_pins(pins, got)
    # the track's phi is the diagnostics' phi of the same rows (identity = index straight after the upload)
    phi = pins["ctx_%s_n%d_phi" % (pin_tag(nb, precision), PIN_SIZES[-1])]
    assert np.array_equal(got["track_%s_phi" % pin_tag(nb, precision)][0], phi[list(PIN_TRACK_IDS)])
