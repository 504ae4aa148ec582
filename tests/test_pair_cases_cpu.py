"""The numpy model of the pair-separation counts (tests/pair_cases.py) against a plain scalar loop of the definition, the
consequences the header states (equality at the edges, coincident bodies, NaN and +inf separations, the points form counting
every unordered pair twice), the windowed host model the probe uses, and what of nbody_get_pair_counts /
nbody_batch_get_pair_counts can be checked without a device: the record layout, the wrapper's handling of the edges and the
argument checks that come before any device call."""
import os
import re
import subprocess

import numpy as np
import pytest

import pair_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
LATTICE_EDGES2 = np.array([0.0, 1.0, 2.0, 4.0, 5.0])
# lattice(8): unordered pairs at d2 = 1, 2, 4, 5: 2*8*7, 2*7*7, 2*8*6, 4*7*6
LATTICE_AT = {1.0: 112, 2.0: 98, 4.0: 96, 5.0: 168}


def edge_sets(n, field):
    top = (0.3 * field) ** 2
    return [np.linspace(0.0, top, 9), np.array([0.0, np.inf]), np.array([4.0, 9.0]), np.geomspace(1e-3, 4 * field * field, 41)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", [0, 1, 2, 50])
def test_model_equals_the_plain_loop(n, dtype):
    P, _ = pc.random_state(n, dtype, seed=n + 1, field=20.0)
    pts = np.random.default_rng(n).uniform(-2, 22, size=(7, 2))
    for e2 in edge_sets(n, 20.0):
        got, want = pc.model_pair_counts(P, e2), pc.loop_pair_counts(P, e2)
        pc.assert_same(got, want, "own form, n %d, %d bins" % (n, len(e2) - 1))
        pc.check_sum(got, n * (n - 1) // 2)
        for m in (0, 1, 7):
            got, want = pc.model_pair_counts(P, e2, pts[:m]), pc.loop_pair_counts(P, e2, pts[:m])
            pc.assert_same(got, want, "points form, n %d, m %d, %d bins" % (n, m, len(e2) - 1))
            pc.check_sum(got, m * n)
    whole = pc.model_pair_counts(P, [0.0, np.inf])
    assert (whole["counts"][0], whole["below"], whole["rest"]) == (n * (n - 1) // 2, 0, 0)


def test_lattice_equality_at_the_edges():
    P, _ = pc.lattice(8)
    for d2, k in LATTICE_AT.items():                             # the closed forms, from the model one value at a time
        assert pc.model_pair_counts(P, [d2, np.nextafter(d2, np.inf)])["counts"][0] == k
    got = pc.model_pair_counts(P, LATTICE_EDGES2)
    pc.assert_same(got, pc.loop_pair_counts(P, LATTICE_EDGES2))
    assert got["counts"].tolist() == [0, 112, 98, 96] and got["below"] == 0     # e2[k] <= d2: the lower edge belongs to the bin
    assert got["rest"] == 2016 - 306                              # d2 == 5 is not below the top edge
    # one ulp down (the first edge stays: a negative edge is refused): every integer d2 stays where it was
    down = np.concatenate([[0.0], np.nextafter(LATTICE_EDGES2[1:], -np.inf)])
    assert pc.model_pair_counts(P, down)["counts"].tolist() == [0, 112, 98, 96]
    # one ulp up: d2 == 1 now lies below edge 1, and so on: every count moves one bin down, d2 == 5 comes in from rest
    up = np.concatenate([[0.0], np.nextafter(LATTICE_EDGES2[1:], np.inf)])
    got = pc.model_pair_counts(P, up)
    pc.assert_same(got, pc.loop_pair_counts(P, up))
    assert got["counts"].tolist() == [112, 98, 96, 168] and got["rest"] == 2016 - 474


def test_awkward_values():
    P, _ = pc.random_state(40, np.float64, seed=3, field=10.0)
    e2 = np.array([0.0, 1.0, 50.0, np.inf])
    clean = pc.model_pair_counts(P, e2)
    assert clean["rest"] == 0
    Pn = P.copy()
    Pn[5, 0] = np.nan                                            # its 39 pairs are in rest, top edge +inf or not
    got = pc.model_pair_counts(Pn, e2)
    pc.assert_same(got, pc.loop_pair_counts(Pn, e2))
    assert got["rest"] == 39 and got["below"] == 0
    Pi = P.copy()
    Pi[5] = [1e200, 0.0]                                         # d2 = +inf fails d2 < +inf
    got = pc.model_pair_counts(Pi, e2)
    pc.assert_same(got, pc.loop_pair_counts(Pi, e2))
    assert got["rest"] == 39
    C = np.array([[3.0, 4.0], [10.0, 10.0], [3.0, 4.0]])         # two bodies at one place: d2 = +0
    assert pc.model_pair_counts(C, [0.0, 1.0])["counts"].tolist() == [1]
    got = pc.model_pair_counts(C, [1e-300, 1.0])
    assert (got["counts"].tolist(), got["below"], got["rest"]) == ([0], 1, 2)


def test_points_on_the_bodies_count_every_pair_twice():
    P, _ = pc.random_state(60, np.float32, seed=9, field=15.0)
    e2 = np.linspace(0.0, 40.0, 6)
    own, pts = pc.model_pair_counts(P, e2), pc.model_pair_counts(P, e2, P)
    want = 2 * own["counts"].astype(np.int64)
    want[0] += 60                                                # every body against itself at d2 = 0
    assert pts["counts"].tolist() == want.tolist() and pts["pairs"] == 3600
    assert pts["rest"] == 2 * own["rest"]


def test_window_equals_model():
    P, _ = pc.random_state(2000, np.float32, seed=21, field=300.0)
    for e2 in (np.geomspace(0.01, 20.0 ** 2, 33), np.array([0.0, 5.0 ** 2]), np.array([16.0, 25.0, 400.0 ** 2])):
        got, want = pc.window_pair_counts(P, e2), pc.model_pair_counts(P, e2)
        pc.assert_same(got, want, "window, top %g" % e2[-1])
        assert int(want["counts"].sum()) > 0
    C = np.array([[1.0, 1.0], [1.0, 2.0], [1.0, 1.0], [4.0, 1.0]])     # equal x, a coincident pair
    pc.assert_same(pc.window_pair_counts(C, [0.0, 1.0, 9.0]), pc.model_pair_counts(C, [0.0, 1.0, 9.0]))


def test_record_layout(nb, tmp_path):
    hdr = open(os.path.join(ROOT, "include", "nbody.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"typedef struct nbody_pair_info \{ int64_t n_bodies, rows, pairs, below, rest; \} nbody_pair_info;", code)
    for name in ("nbody_get_pair_counts", "nbody_batch_get_pair_counts"):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), "%s is not declared in include/nbody.h" % name
        assert name in nb.SYMBOLS and getattr(nb.lib, name).argtypes == nb.SYMBOLS[name][1]
    names = ("n_bodies", "rows", "pairs", "below", "rest")
    assert nb.PAIR_INFO_DTYPE.itemsize == 40 and nb.PAIR_INFO_DTYPE == pc.INFO_DTYPE
    assert [nb.PAIR_INFO_DTYPE.fields[k][1] for k in names] == [0, 8, 16, 24, 32]
    src = tmp_path / "sz.c"                                       # sizeof and offsets as the C compiler sees them
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "nbody.h"\nint main(void) { printf("%zu", sizeof(nbody_pair_info));\n'
                   + "".join('printf(" %%zu", offsetof(nbody_pair_info, %s));\n' % k for k in names) + "return 0; }\n")
    exe = tmp_path / "sz"
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert subprocess.check_output([str(exe)]).split() == [b"40", b"0", b"8", b"16", b"24", b"32"]
    assert nb.lib.nbody_abi_version() == 2


def test_wrapper_squares_once_and_refuses_negative_lengths(nb):
    edges = np.array([0.0, 0.1, 1.0 / 3.0, np.pi, 1e155, 1e200, np.inf])
    e2 = nb.pair_edges2(edges)
    with np.errstate(over="ignore"):
        want = edges * edges
    assert e2.dtype == np.float64 and np.array_equal(e2.view(np.uint64), want.view(np.uint64))
    wide = np.float32([0.1, 0.7]).astype(np.float64)            # fp32 lengths are widened first, then squared in float64
    assert np.array_equal(nb.pair_edges2(np.float32([0.1, 0.7])).view(np.uint64), (wide * wide).view(np.uint64))
    same = nb.pair_edges2(edges, squared=True)
    assert np.array_equal(same.view(np.uint64), edges.view(np.uint64)) and same is not edges
    with pytest.raises(ValueError):
        nb.pair_edges2([0.0, -1.0, 2.0])
    with pytest.raises(ValueError):
        nb.pair_edges2([-0.5, 1.0])
    nb.pair_edges2([-4.0, 1.0], squared=True)                    # squared edges are the library's to refuse
    for bad in ([1.0], [[0.0, 1.0]], []):
        with pytest.raises(ValueError):
            nb.pair_edges2(bad)


def test_bad_arguments_are_invalid_before_any_device_call(nb):
    """NULL handles, and with a handle that is never dereferenced: every check on edges, bins and m comes first."""
    counts = np.full(4, 7, dtype=np.uint64)
    info = np.full(1, 7, dtype=pc.INFO_DTYPE)
    e2 = np.array([0.0, 1.0, 4.0])
    one, many = nb.lib.nbody_get_pair_counts, nb.lib.nbody_batch_get_pair_counts
    for call, name in ((one, b"nbody_get_pair_counts"), (many, b"nbody_batch_get_pair_counts")):
        assert call(None, None, 0, e2.ctypes.data, 2, counts.ctypes.data, info.ctypes.data) == INVALID
        assert name + b": NULL" in nb.lib.nbody_last_error_string()
    assert (counts == 7).all() and info.tobytes() == np.full(1, 7, dtype=pc.INFO_DTYPE).tobytes()
