"""The model and the cases of the tracer particles (nbody_tracers_*, nbody_batch_tracers_*).

advance() restates the update of include/nbody.h in numpy: every operation on np.float64 arrays, each rounded on its own
(numpy never fuses a multiply with an add), in the order the header writes them.  The field itself is an input: the GPU
tests take it from the library's own nbody_get_field on the twin's state (whose accuracy test_gpu_field.py bounds), the CPU
tests from point_field() below.
"""
import numpy as np

G = float(np.float32(6.67408e-11))
# The dense fields test_gpu_batch.py uses (FIELD_OF there: 77 -> 1000, 130 -> 1500, 300 -> 2000, 1024 -> 5000), and for the
# sizes it has no entry for the field of the next larger size that has one: stock radii collide in every step.
DENSE_FIELD = {0: 1000, 1: 1000, 127: 1500, 129: 1500, 130: 1500, 300: 2000, 1024: 5000}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def advance(tr, acc, dt, walls, field):
    """One advance of the tracers `tr` ({"pos": (..., 2), "vel": (..., 2)}) from the accelerations `acc` (..., 2) of the
    field at their positions: dt the time step already widened to double, walls the NBODY_TRACER_WALLS flag, field =
    (fieldWidth, fieldHeight).  -> {"pos", "vel"}."""
    pos = np.array(tr["pos"], dtype=np.float64)
    vel = np.array(tr["vel"], dtype=np.float64)
    acc = np.asarray(acc, dtype=np.float64)
    dt = np.float64(dt)
    with np.errstate(all="ignore"):
        dv = dt * acc
        if walls:
            hi = np.array([field[0], field[1]], dtype=np.float64)
            lo = np.array([-field[0], -field[1]], dtype=np.float64)
            t = pos + (acc * dt)
            vel = np.where((t > hi) | (t < lo), vel * np.float64(-1.0), vel)
        vel = vel + dv
        pos = pos + (dt * vel)
    return {"pos": pos, "vel": vel}


def point_field(P, M, pts):
    """A plain fp64 field of the sources (P (n, 2), M (n,)) at pts (m, 2), sources at distance 0 left out: good enough for
    the properties of the model (its roundings are not the library's)."""
    P, M, pts = (np.asarray(a, dtype=np.float64) for a in (P, M, pts))
    acc = np.zeros(pts.shape, dtype=np.float64)
    with np.errstate(all="ignore"):
        for j in range(len(M)):
            d = P[j] - pts
            r2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
            w = np.where(r2 == 0, 0.0, G * M[j] / (np.where(r2 == 0, 1.0, r2) * np.sqrt(np.where(r2 == 0, 1.0, r2))))
            acc = acc + w[:, None] * d
    return acc


def dt_of(nb, cfg, precision):
    """StepParams<T>::dt widened to double."""
    return float(np.float32(cfg.timestep)) if precision == nb.F32 else float(cfg.timestep)


def dense_case(nb, n, precision=0, seed=1024):
    """(cfg, bodies): the stock initial condition of n bodies in the dense field of its size."""
    f = DENSE_FIELD[n]
    cfg = nb.stock_config(particleCount=max(n, 1), fieldWidth=f, fieldHeight=f)
    if n == 0:
        return cfg, nb.BodiesData(0, precision)
    return cfg, nb.init_bodies(cfg, precision, seed=seed)


def tracer_set(cfg, m, seed):
    """m tracers: uniform over the field (centre and corners of it are body territory), velocities of a few units; when there
    is room the last ones sit far outside the field and just outside a wall."""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-1, 1, size=(m, 2)) * [cfg.fieldWidth, cfg.fieldHeight]
    vel = rng.uniform(-5, 5, size=(m, 2))
    if m >= 3:
        pos[-1] = [-7.5 * cfg.fieldWidth, 11.25 * cfg.fieldHeight]
        pos[-2] = [cfg.fieldWidth + 0.5, 0.25 * cfg.fieldHeight]
    return pos, vel
