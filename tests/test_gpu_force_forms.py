"""GPU test of WHICH force kernel a context runs (run with -m gpu on an MI355X).

nbody_force_kernel_name() is what bench.py reports as the kernel it measured, so it has to name the form that
launch_forces takes - for every kernel_variant the library knows, for the automatic choice on both sides of each of its
size thresholds, and with the event log on and off.  The expected strings below were written down from the name function
as it stood BEFORE the choice got one home (one switch for the launch, a second one for the name); they are not derived
from the library's table.  The name is a host decision: it needs a created context and an upload, no step - one step is
taken at n = 1024 only, where every variant must give variant 1's state bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

V1, V3, V3W = "forces_v1<float>", "forces_v3_f32", "forces_v3w_f32"
R2X8 = "forces_ring_f32 (2 rings x 8 waves per workgroup)"
R4X4 = "forces_ring_f32 (4 rings x 4 waves per workgroup)"
R1X8 = "forces_ring_f32 (1 ring x 8 waves per workgroup)"
R2X8T16 = "forces_ring_f32 (2 rings x 8 waves, 16-position turns)"
QUEUE = "forces_ring_f32 (4 rings x 4 waves per workgroup, persistent)"
SOLO = "forces_ring_f32 (16 solo waves per workgroup)"
SOLO_QUEUE = "forces_ring_f32 (16 solo waves per workgroup, persistent)"

# the variants whose name does not depend on the size
FIXED = {1: V1, 11: V3, 12: V3, 14: V3, 18: V3, 31: V3W, 32: V3W, 50: R2X8, 55: R2X8, 56: R2X8, 58: R2X8, 52: R4X4,
         59: R4X4, 61: QUEUE, 62: QUEUE, 53: R2X8T16, 54: R1X8, 70: SOLO, 71: SOLO_QUEUE, 72: SOLO_QUEUE}
BY_SIZE = (0, 60, 63)        # automatic, and the two that fall through to it where the persistent form does not apply
FP64 = {0: "forces_v3w_f64", 1: "forces_v1<double>", 52: "forces_v3w_f64", 71: "forces_v3w_f64"}


def name_by_size(variant, n, log, cus):
    """The name function of the parent commit for variants 0, 60 and 63 on one rank, restated: own_upper is n rounded up to
    whole blocks; the persistent 4 x 4 form applies from two rounds of rings on (a ring is 64 bodies, a CU serves 4)."""
    own = (n + 127) // 128 * 128
    rings = 2 * max(own // 128, 1)
    slots = 4 * min(cus, (rings + 3) // 4)
    queue = rings >= 2 * slots
    if variant in (60, 63) and queue:
        return QUEUE
    if not log and rings == 16 * cus:
        return SOLO_QUEUE
    if own >= 49152:
        return QUEUE if queue else R4X4
    if own >= 24576:
        return R2X8
    return R1X8


# the same, as plain values for the device this library is built for (256 CUs): (variant, n, log) -> name
PINNED_256 = {
    (0, 1024, False): R1X8, (0, 24448, False): R1X8, (0, 24449, False): R2X8, (0, 24576, True): R2X8,
    (0, 49024, False): R2X8, (0, 49025, False): R4X4, (0, 49152, True): R4X4, (0, 65536, False): R4X4,
    (0, 131072, False): QUEUE, (0, 131072, True): QUEUE, (0, 262144, False): SOLO_QUEUE, (0, 262144, True): QUEUE,
    (60, 1024, False): R1X8, (60, 24576, False): R2X8, (60, 65536, True): R4X4, (60, 131072, False): QUEUE,
    (60, 262144, False): QUEUE, (63, 49152, False): R4X4, (63, 131072, True): QUEUE, (63, 262144, False): QUEUE,
}


def _sizes(cus):
    solo = 16 * cus * 64
    return sorted({1024, 24448, 24449, 24576, 49024, 49025, 49152, 65536, solo // 2, solo})


@pytest.fixture(scope="module")
def big(nb):
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = max(_sizes(cus))
    cfg = nb.stock_config(particleCount=n, minRadius=0.0, maxRadius=0.0)
    return cus, cfg, nb.init_bodies(cfg)


def _first(nb, bodies, n):
    b = nb.BodiesData(n, bodies.precision)
    for dst, src in ((b.Positions, bodies.Positions), (b.Velocities, bodies.Velocities), (b.Masses, bodies.Masses),
                     (b.Radii, bodies.Radii)):
        dst[:] = src[:n]
    return b


def test_pinned_names_are_the_restated_rule():
    for (variant, n, log), name in PINNED_256.items():
        assert name_by_size(variant, n, log, 256) == name, (variant, n, log)
    assert {n for _, n, _ in PINNED_256} <= set(_sizes(256)) and _sizes(256)[-1] == 262144


@pytest.mark.parametrize("log", [False, True], ids=["no-log", "event-log"])
def test_name_is_the_parents_for_every_variant_and_size(nb, big, log):
    cus, cfg, bodies = big
    sizes = _sizes(cus)
    cut = {n: _first(nb, bodies, n) for n in sizes}
    for variant in sorted(FIXED) + list(BY_SIZE) + [7, 99]:                 # 7, 99: no such variant - automatic, as 0
        with nb.Stepper(cfg, kernel_variant=variant, record_events=log) as st:
            for n in (sizes if variant not in FIXED else (1024, 49152)):
                st.upload(cut[n])
                want = FIXED[variant] if variant in FIXED else name_by_size(variant if variant in BY_SIZE else 0, n, log, cus)
                assert st.force_kernel_name() == want, (variant, n, log, cus, st.force_kernel_name())
                if cus == 256 and (variant, n, log) in PINNED_256:
                    assert st.force_kernel_name() == PINNED_256[variant, n, log], (variant, n, log)


def test_name_fp64(nb):
    b = nb.init_bodies(nb.stock_config(particleCount=1024, minRadius=0.0, maxRadius=0.0), nb.F64)
    for variant, want in FP64.items():
        for log in (False, True):
            with nb.Stepper(nb.stock_config(particleCount=1024), precision=nb.F64, kernel_variant=variant, record_events=log) as st:
                st.upload(b)
                assert st.force_kernel_name() == want, (variant, log)


@pytest.mark.parametrize("log", [False, True], ids=["no-log", "event-log"])
def test_every_variant_steps_like_variant_1(nb, log):
    """One step at n = 1024 in a dense field with stock radii (collisions, deletions): every variant number and the
    automatic choice leave variant 1's state."""
    cfg = nb.stock_config(particleCount=1024, fieldWidth=5000, fieldHeight=5000)
    bodies = nb.init_bodies(cfg)

    def step(variant):
        with nb.Stepper(cfg, kernel_variant=variant, record_events=log) as st:
            st.upload(bodies)
            st.step(1)
            d = st.download()
            return d.numBodies, d.block.view(np.uint32).copy()
    n1, ref = step(1)
    assert n1 < 1024
    for variant in [0] + sorted(set(FIXED) - {1}) + [60, 63]:
        n, got = step(variant)
        assert n == n1 and np.array_equal(got, ref), "variant %d (event log %s) != variant 1" % (variant, log)
