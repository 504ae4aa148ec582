"""The numpy model of group finding (tests/group_cases.py) against a plain scalar loop of the definition, the consequences the
header states (labels are lowest indices, symmetry, the overlap predicate at (link, radius_scale) = (0, 1), NaN coordinates),
and what of nbody_get_groups / nbody_batch_get_groups can be checked without a device: the exports, the record layout and
the argument handling."""
import ctypes
import os
import re

import numpy as np
import pytest

import group_cases as gc
import neighbor_cases as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1
NEW_SYMBOLS = ("nbody_get_groups", "nbody_batch_get_groups")
# random_state(300, ., seed=11, field=100): (link, radius_scale) -> (n_groups, largest), the same for both precisions
COUNTS_300 = {(4.0, 1.0): (67, 25), (6.0, 1.0): (5, 292), (0.0, 1.0): (272, None)}


def check_labels(label):
    n = len(label)
    assert label.dtype == np.int32 and label.shape == (n,)
    assert np.array_equal(label[label], label) and (label <= np.arange(n)).all() and (label >= 0).all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n", [1, 2, 3, 129, 300])
def test_model_equals_the_plain_loop(n, dtype):
    P, R = gc.random_state(n, dtype, seed=n, field=40.0)
    for link, scale in ((0.0, 1.0), (1.0, 1.0), (2.5, 0.0), (0.0, 0.0), (np.inf, 1.0), (0.5, 2.0)):
        got, want = gc.model_groups(P, R, link, scale), gc.loop_groups(P, R, link, scale)
        gc.assert_same(got, want, "n %d link %g scale %g" % (n, link, scale))
        check_labels(got["label"])
        assert got["n_groups"] == len(np.unique(got["label"])) and 1 <= got["largest"] <= n
    assert gc.model_groups(P, R, np.inf)["n_groups"] == 1
    assert gc.model_groups(P, R, 0.0, 0.0)["n_groups"] == n       # no two bodies coincide


def test_no_bodies():
    got = gc.model_groups(np.zeros((0, 2)), np.zeros(0), 1.0)
    assert got["label"].shape == (0,) and (got["n_groups"], got["largest"]) == (0, 0)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_the_states_of_the_gpu_tests(dtype):
    P, R = gc.random_state(300, dtype, seed=11, field=100)
    for (link, scale), (n_groups, largest) in COUNTS_300.items():
        got = gc.model_groups(P, R, link, scale)
        check_labels(got["label"])
        assert got["n_groups"] == n_groups and largest in (None, got["largest"]), (link, scale, got["n_groups"], got["largest"])
    big = gc.model_groups(P, R, 6.0)
    members = np.flatnonzero(big["label"] == np.bincount(big["label"]).argmax())
    assert len(set(members // 128)) == 3                          # the percolating group spans all three tiles
    P, R = gc.random_state(1000, dtype, seed=11, field=100)
    assert gc.model_groups(P, R, 2.0, 0.0)["n_groups"] == 519


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_adjacency_is_symmetric_and_is_the_overlap_predicate(dtype):
    P, R = gc.random_state(300, dtype, seed=12, field=30.0)
    for link, scale in ((0.0, 1.0), (0.7, 1.0), (1.5, 0.0), (0.3, 2.5)):
        A = gc.adjacency(P, R, link, scale)
        assert np.array_equal(A, A.T) and not A.diagonal().any() and A.any()
    own = nc.model_neighbors(P, R)
    A = gc.adjacency(P, R, 0.0, 1.0)
    assert np.array_equal(A.sum(axis=1), own["overlaps"])         # 1*x and x + 0 are exact: the same s*s
    singles = gc.model_groups(P, R, 0.0)["label"]
    alone = np.bincount(singles, minlength=300)[singles] == 1
    assert np.array_equal(alone, own["overlaps"] == 0)


def test_chain_and_lattice():
    P, R = gc.shuffled_chain(300)
    assert sorted(P[:, 0].tolist()) == list(range(300)) and P[0, 0] != 0
    one = gc.model_groups(P, R, 0.5)                              # s = 1: d2 = 1 <= 1
    assert (one["label"] == 0).all() and (one["n_groups"], one["largest"]) == (1, 300)
    assert gc.model_groups(P, R, 0.25)["n_groups"] == 300
    gc.assert_same(one, gc.loop_groups(P, R, 0.5))
    P, R = gc.lattice(8, 0.25)
    assert gc.model_groups(P, R, 0.5)["n_groups"] == 1            # equality counts: d2 == s*s == 1
    assert gc.model_groups(P, R, 0.49)["n_groups"] == 64
    assert gc.model_groups(P, R, 0.0, 2.0)["n_groups"] == 1       # the radii alone, doubled


def test_awkward_values():
    P, R = gc.random_state(130, np.float64, seed=2, field=30.0, radius=1.0)
    clean = gc.model_groups(P, R, 0.5)
    assert 1 < clean["n_groups"] < 130
    Pn = P.copy()
    Pn[7, 0] = np.nan                                             # a NaN coordinate: every d2 with body 7 is NaN
    got = gc.model_groups(Pn, R, 0.5)
    gc.assert_same(got, gc.loop_groups(Pn, R, 0.5))
    assert got["label"][7] == 7 and (got["label"] == 7).sum() == 1
    assert (gc.model_groups(Pn, R, np.inf)["label"] == np.where(np.arange(130) == 7, 7, 0)).all()
    Rn = R.copy()
    Rn[5] = np.nan                                                # a NaN radius: s*s is NaN, body 5 links nothing ...
    got = gc.model_groups(P, Rn, 0.5)
    assert got["label"][5] == 5 and (got["label"] == 5).sum() == 1
    gc.assert_same(gc.model_groups(P, Rn, 0.5, 0.0), gc.model_groups(P, R, 0.5, 0.0))   # ... and 0 * NaN is NaN too
    C = np.array([[3.0, 4.0], [10.0, 10.0], [3.0, 4.0]])
    got = gc.model_groups(C, np.zeros(3), 0.0)                    # coincident, radii 0, link 0: 0 <= 0
    assert got["label"].tolist() == [0, 1, 0]
    assert (gc.model_groups(P, R, np.inf)["label"] == 0).all()


def test_zero_times_nan_radius_is_nan():
    """radius_scale = 0 does not hide a NaN radius: 0 * NaN is NaN, the pair is not linked."""
    P = np.array([[0.0, 0.0], [1.0, 0.0], [2.0, 0.0]])
    R = np.array([0.1, np.nan, 0.1])
    assert gc.model_groups(P, R, 1.0, 0.0)["label"].tolist() == [0, 1, 2]
    assert gc.loop_groups(P, R, 1.0, 0.0)["label"].tolist() == [0, 1, 2]
    assert gc.model_groups(P, R, 2.0, 0.0)["label"].tolist() == [0, 1, 0]


def test_library_exports_the_symbols_and_the_record(nb, tmp_path):
    hdr = open(os.path.join(ROOT, "include", "nbody.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    raw = ctypes.CDLL(nb.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), "%s is not declared in include/nbody.h" % name
        assert hasattr(raw, name), "the library does not export %s" % name
        assert name in nb.SYMBOLS and getattr(nb.lib, name).argtypes == nb.SYMBOLS[name][1]
    assert re.search(r"typedef struct nbody_groups_info \{ int32_t n_bodies, n_groups, largest, sweeps; \} nbody_groups_info;", code)
    assert nb.GROUPS_INFO_DTYPE.itemsize == 16 and nb.GROUPS_INFO_DTYPE == gc.INFO_DTYPE
    assert [nb.GROUPS_INFO_DTYPE.fields[k][1] for k in ("n_bodies", "n_groups", "largest", "sweeps")] == [0, 4, 8, 12]
    # sizeof as the C compiler sees it
    src = tmp_path / "sz.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "nbody.h"\n'
                   'int main(void) { printf("%zu %zu\\n", sizeof(nbody_groups_info), offsetof(nbody_groups_info, sweeps)); return 0; }\n')
    import subprocess
    exe = tmp_path / "sz"
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    assert subprocess.check_output([str(exe)]).split() == [b"16", b"12"]


def test_abi_version_stays_2(nb):
    assert nb.lib.nbody_abi_version() == 2


def test_null_handles_and_bad_parameters_are_invalid(nb):
    label = np.full(4, 7, dtype=np.int32)
    info = np.full(1, 7, dtype=gc.INFO_DTYPE)
    one, many = nb.lib.nbody_get_groups, nb.lib.nbody_batch_get_groups
    assert one(None, 1.0, 1.0, label.ctypes.data, 4, info.ctypes.data) == INVALID
    assert b"nbody_get_groups: NULL" in nb.lib.nbody_last_error_string()
    assert many(None, 1.0, 1.0, label.ctypes.data, info.ctypes.data) == INVALID
    assert b"nbody_batch_get_groups: NULL" in nb.lib.nbody_last_error_string()
    # the parameters are looked at first, so the message names them even without a handle
    for link, scale, word in ((np.nan, 1.0, b"link"), (-1.0, 1.0, b"link"), (-np.inf, 1.0, b"link"), (1.0, np.nan, b"radius_scale"),
                              (1.0, -0.5, b"radius_scale"), (1.0, np.inf, b"radius_scale"), (np.inf, -np.inf, b"radius_scale")):
        for call in (lambda: one(None, link, scale, label.ctypes.data, 4, info.ctypes.data),
                     lambda: many(None, link, scale, label.ctypes.data, info.ctypes.data)):
            assert call() == INVALID
            assert word + b" = " in nb.lib.nbody_last_error_string(), (link, scale, nb.lib.nbody_last_error_string())
    assert one(None, np.inf, 0.0, label.ctypes.data, 4, info.ctypes.data) == INVALID     # both legal: the handle is what is wrong
    assert b"NULL" in nb.lib.nbody_last_error_string()
    assert (label == 7).all() and info["sweeps"][0] == 7


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_window_groups_equals_the_model(dtype):
    """The checker the probe uses at sizes the n x n model cannot reach."""
    for n, field in ((1, 10.0), (2, 1.0), (300, 100.0), (1000, 100.0)):
        P, R = gc.random_state(n, dtype, seed=11, field=field)
        for link, scale in ((0.0, 1.0), (4.0, 1.0), (6.0, 1.0), (2.0, 0.0), (0.0, 0.0), (0.5, 2.0)):
            got, want = gc.window_groups(P, R, link, scale), gc.model_groups(P, R, link, scale)
            gc.assert_same(got, want, "n %d link %g scale %g" % (n, link, scale))
            assert n < 2 or got["links"] == gc.adjacency(P, R, link, scale).sum() // 2
    P, R = gc.shuffled_chain(300)
    assert (gc.window_groups(P, R, 0.5)["label"] == 0).all() and gc.window_groups(P, R, 0.25)["n_groups"] == 300
    P, R = gc.lattice(8, 0.25)
    assert gc.window_groups(P, R, 0.5)["n_groups"] == 1 and gc.window_groups(P, R, 0.49)["n_groups"] == 64
