"""The fp32 ring kernel's turn bookkeeping at the smallest sizes where it can go wrong: the index arithmetic of the turn
loop is 32-bit unsigned on the scalar unit (first body of the next tile, its wrap at N, the length of a tile, "is the
window an aligned tile that ends at or before N"), the window's first entry is a byte offset kept in a register, and the
look at the other rings of a workgroup is one per-lane read.  BIT-EXACT against the CPU oracle: state
words, survivor count and the pair counter, three steps on one context.

    N = 100         fewer bodies than a tile
    N = 129, 130    clean: a truncated last tile of one / two entries; literal: the ONE tile is the truncated one, of
                    N mod 129 = 0 / 1 entries (no pair at all: the one entry is the body itself), bodies from 128 on frozen
    N = 257         clean: a last tile of one entry; literal: two tiles, the last one of 257 mod 129 = 128 entries, body 256
                    frozen
    N = 512         the last tile ends exactly at N: st + 128 == N takes the aligned window
    N = 640         two and a half workgroups of four rings: ring slots without own bodies next to the look at the other rings
    N = 1000        literal: truncated last tile of 1000 mod 129 entries, bodies 896 ... 999 frozen; clean: a last tile of 104
    N = 2053        unaligned windows after the wrap (st + 128 > N: the entries wrap inside a window)

Every shape in literal and clean semantics, at radii 0 in a wide field (no screen per pair) and at stock radii in a
5000-wide field (collisions, absorptions, deletions), under the one-shot 4 x 4, 2 x 8 and 1 x 8 geometries (kernel_variant
52, 50, 54) and the persistent form with every walk cut into segments of 1 / 3 tiles (61, 62).  One oracle reference per
case, computed once and shared; no exclusions."""
import numpy as np
import pytest

import oracle_lib as ol

pytestmark = pytest.mark.gpu

DT, GROWTH = np.float32(0.2), np.float32(0.1)
STEPS = 3
SIZES = [100, 129, 130, 257, 512, 640, 1000, 2053]
VARIANTS = [52, 61, 62, 50, 54]
SEMANTICS = {"literal": ol.LITERAL, "clean": ol.CLEAN}
RADII = {"r0": dict(field=100000, kw={"minRadius": 0.0, "maxRadius": 0.0}), "stock": dict(field=5000, kw={})}


def _bodies(nb, n, radii):
    field = RADII[radii]["field"]
    cfg = nb.stock_config(particleCount=n, fieldWidth=field, fieldHeight=field, **RADII[radii]["kw"])
    return cfg, nb.init_bodies(cfg), field


_REFERENCE = {}


def _reference(nb, n, semantics, radii):
    """-> per step (survivors, state words, pairs so far) from the oracle"""
    key = (n, semantics, radii)
    if key not in _REFERENCE:
        _, bodies, field = _bodies(nb, n, radii)
        blk = bodies.contiguousData.copy()
        cur, pairs, out = n, 0, []
        for _ in range(STEPS):
            cur, stats, *_ = ol.port_step(blk, cur, DT, field, field, GROWTH, semantics=SEMANTICS[semantics],
                                          want_events=False)
            pairs += int(stats.pairs)
            out.append((cur, blk[:6 * cur].view(np.uint32).copy(), pairs))
        for o in out:
            o[1].setflags(write=False)
        _REFERENCE[key] = out
    return _REFERENCE[key]


def _check(nb, n, semantics, radii, variant, record_events):
    oracle = _reference(nb, n, semantics, radii)
    cfg, bodies, _ = _bodies(nb, n, radii)
    sem = nb.CLEAN if semantics == "clean" else nb.LITERAL
    with nb.Stepper(cfg, semantics=sem, kernel_variant=variant, record_events=record_events) as st:
        st.upload(bodies)
        for s in range(STEPS):
            st.step(1)
            d = st.download()
            what = "N %d %s %s variant %d step %d" % (n, semantics, radii, variant, s)
            assert d.numBodies == oracle[s][0], (what, d.numBodies, oracle[s][0])
            assert np.array_equal(d.block.view(np.uint32), oracle[s][1]), what + ": state differs from the oracle"
            assert int(st.stats().pairs) == oracle[s][2], (what, int(st.stats().pairs), oracle[s][2])


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("radii", list(RADII))
@pytest.mark.parametrize("semantics", list(SEMANTICS))
@pytest.mark.parametrize("n", SIZES)
def test_turn_edges_three_steps(nb, n, semantics, radii, variant):
    if radii == "stock" and n >= 512:
        assert _reference(nb, n, semantics, radii)[0][0] < n       # the dense field did remove bodies in the first step
    _check(nb, n, semantics, radii, variant, record_events=False)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("semantics", list(SEMANTICS))
@pytest.mark.parametrize("n", SIZES)
def test_turn_edges_event_logging_builds(nb, n, semantics, variant):
    """The builds that record events share the template but keep the 64-bit index arithmetic, the per-window entry and the
    four-address look (they have no register to spare): the same comparison at stock radii, both semantics."""
    _check(nb, n, semantics, "stock", variant, record_events=True)
