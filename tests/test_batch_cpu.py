"""Host side of the batched stepper (nbody_batch_*, StepperBatch) and the seeded initial condition: everything that
needs no GPU.  Argument errors must be found before any device call, so they are checked here."""
import ctypes
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INVALID, NO_DEVICE = -1, -5


def _restated_init(nb, cfg, precision, seed):
    """src/nbody.cu:401-416 with the seed as a parameter: x, y, m, r per body in that order from one generator, fp32
    rounding each finished draw where csrc/nbody_bodies.c does, fp64 keeping the double draws; v = 0."""
    g = nb.Rng()
    nb.lib.nbody_rng_seed(ctypes.byref(g), seed)
    n = cfg.particleCount
    real = np.float64 if precision == nb.F64 else np.float32
    P, M, R = np.zeros((n, 2), real), np.zeros(n, real), np.zeros(n, real)
    draw = lambda a, b: nb.lib.nbody_rng_fval_range(ctypes.byref(g), float(a), float(b))   # noqa: E731
    for i in range(n):
        x = draw(0, cfg.fieldWidth << 1) - cfg.fieldWidth
        y = draw(0, cfg.fieldHeight << 1) - cfg.fieldHeight
        m = draw(cfg.minRandBodyMass, cfg.maxRandBodyMass)
        r = draw(cfg.minRadius, cfg.maxRadius)
        P[i] = [real(x), real(y)]
        M[i] = real(m)
        R[i] = real(r)
    return np.concatenate([P.ravel(), np.zeros(2 * n, real), M, R])


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def test_seed_1024_is_the_reference_initial_condition(nb):
    z = np.load(os.path.join(GOLD, "init_stock.npz"))
    cfg = nb.stock_config(particleCount=64)
    for precision in (nb.F32, nb.F64):
        a = nb.BodiesData(64, precision)
        b = nb.BodiesData(64, precision)
        assert nb.lib.nbody_init_bodies(ctypes.byref(cfg), a.ptr, precision) == 0
        assert nb.lib.nbody_init_bodies_seeded(ctypes.byref(cfg), b.ptr, precision, 1024) == 0
        assert np.array_equal(_bits(a.block), _bits(b.block))
    seeded = nb.init_bodies(cfg, seed=1024)
    assert np.array_equal(seeded.block.view(np.uint32), z["stock_n64"])
    assert np.array_equal(nb.init_bodies(cfg).block.view(np.uint32), z["stock_n64"])          # the default seed
    small = nb.stock_config(particleCount=48, fieldWidth=5000, fieldHeight=7000, minRandBodyMass=1.0,
                            maxRandBodyMass=1e6, minRadius=0.0, maxRadius=0.0)
    assert np.array_equal(nb.init_bodies(small, seed=1024).block.view(np.uint32), z["small_n48"])


@pytest.mark.parametrize("precision", [0, 1], ids=["fp32", "fp64"])
@pytest.mark.parametrize("seed", [1, 0xfeedfacecafebeef])
def test_other_seeds_equal_the_restated_draw_order(nb, seed, precision):
    cfg = nb.stock_config(particleCount=97, fieldWidth=5000, fieldHeight=7000)
    got = nb.init_bodies(cfg, precision, seed=seed)
    want = _restated_init(nb, cfg, precision, seed)
    assert got.block.dtype == want.dtype
    assert np.array_equal(_bits(got.block), _bits(want))
    assert not np.array_equal(_bits(got.block), _bits(nb.init_bodies(cfg, precision).block))  # and it is another draw


def test_seeded_init_rejects_bad_arguments(nb):
    cfg = nb.stock_config(particleCount=4)
    assert nb.lib.nbody_init_bodies_seeded(None, None, 0, 7) == INVALID
    assert nb.lib.nbody_init_bodies_seeded(ctypes.byref(cfg), None, 0, 7) == INVALID
    assert nb.lib.nbody_last_error_string()


def _desc(nb, **kw):
    d = nb._BatchDesc()
    d.precision, d.semantics, d.systems, d.capacity, d.device = nb.F32, nb.LITERAL, 4, 256, 0
    d.flags, d.event_capacity, d.kernel_variant = 0, 0, 0
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _params(nb, n):
    arr = (nb._BatchParams * max(n, 1))()
    for p in arr:
        p.timestep, p.growthRate, p.fieldWidth, p.fieldHeight = 0.2, 0.1, 100000, 100000
    return arr


BAD_DESCRIPTORS = {
    "systems-0": dict(systems=0),
    "systems-negative": dict(systems=-3),
    "systems-above-grid-y": dict(systems=65536, capacity=1),
    "capacity-0": dict(capacity=0),
    "capacity-negative": dict(capacity=-1),
    "too-many-bodies": dict(systems=65535, capacity=1 << 20),
    "fp64": dict(precision=1),
    "precision-unknown": dict(precision=7),
    "semantics-unknown": dict(semantics=2),
    "flag-group-exchange": dict(flags=2),
    "flag-force-comm": dict(flags=4),
    "flag-events-and-exchange": dict(flags=3),
    "flag-unknown": dict(flags=1 << 9),
    "event-capacity-negative": dict(flags=1, event_capacity=-1),
    "variant-3": dict(kernel_variant=3),
    "variant-11": dict(kernel_variant=11),
}


@pytest.mark.parametrize("case", sorted(BAD_DESCRIPTORS))
def test_bad_descriptor_is_invalid_before_any_device_call(nb, case):
    """NBODY_ERR_INVALID, not NBODY_ERR_NO_DEVICE: the descriptor is judged before the device is looked for."""
    d = _desc(nb, **BAD_DESCRIPTORS[case])
    out = ctypes.c_void_p(0x1)
    rc = nb.lib.nbody_batch_create(ctypes.byref(out), ctypes.byref(d), _params(nb, 4))
    assert rc == INVALID, (case, rc, nb.lib.nbody_last_error_string())
    assert nb.lib.nbody_last_error_string(), case
    assert not out.value, "no handle is handed out on failure"


def test_fp64_batch_says_what_to_do_instead(nb):
    out = ctypes.c_void_p()
    assert nb.lib.nbody_batch_create(ctypes.byref(out), ctypes.byref(_desc(nb, precision=1)), _params(nb, 4)) == INVALID
    assert b"fp64" in nb.lib.nbody_last_error_string()


def test_null_arguments_are_invalid(nb):
    L = nb.lib
    out = ctypes.c_void_p()
    d = _desc(nb)
    assert L.nbody_batch_create(ctypes.byref(out), ctypes.byref(d), None) == INVALID          # NULL params
    assert b"params" in L.nbody_last_error_string()
    assert L.nbody_batch_create(None, ctypes.byref(d), _params(nb, 4)) == INVALID
    assert L.nbody_batch_create(ctypes.byref(out), None, _params(nb, 4)) == INVALID
    n, total = ctypes.c_int(0), ctypes.c_int64(0)
    buf = np.zeros(16, np.float32)
    counts = (ctypes.c_int * 1)(0)
    ptrs = (ctypes.c_void_p * 1)(buf.ctypes.data)
    st = nb.Stats()
    for rc in (L.nbody_batch_upload(None, ptrs, counts), L.nbody_batch_step(None, 1), L.nbody_batch_sync(None),
               L.nbody_batch_counts(None, counts), L.nbody_batch_download(None, 0, buf.ctypes.data, ctypes.byref(n)),
               L.nbody_batch_get_events(None, 0, None, 0, ctypes.byref(total)),
               L.nbody_batch_get_stats(None, 0, ctypes.byref(st))):
        assert rc == INVALID
        assert L.nbody_last_error_string()
    assert L.nbody_batch_kernel_name(None) == b""
    assert L.nbody_batch_destroy(None) == 0


def test_stepper_batch_checks_its_parameter_list(nb):
    with pytest.raises(ValueError):
        nb.StepperBatch(3, 128, params=[(0.2, 0.1, 1000, 1000)] * 2)
    with pytest.raises(nb.NbodyError) as ei:                  # neither params nor cfg: NULL params
        nb.StepperBatch(3, 128)
    assert ei.value.status == INVALID
    with pytest.raises(nb.NbodyError) as ei:
        nb.StepperBatch(0, 128, params=[])
    assert ei.value.status == INVALID
    with pytest.raises(nb.NbodyError) as ei:
        nb.StepperBatch(2, 128, cfg=nb.stock_config(), precision=nb.F64)
    assert ei.value.status == INVALID


def test_valid_descriptor_fails_loudly_without_gpu(nb):
    if os.path.exists("/dev/kfd"):
        pytest.skip("a GPU is present")
    for systems in (1, 4096):                                  # the largest batch the issue names is a valid descriptor
        with pytest.raises(nb.NbodyError) as ei:
            nb.StepperBatch(systems, 1024, cfg=nb.stock_config(particleCount=1024), record_events=True)
        assert ei.value.status == NO_DEVICE
