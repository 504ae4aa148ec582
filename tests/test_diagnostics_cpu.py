"""Diagnostics entry points without a device: the symbols are exported and bound, NULL arguments are refused, and the
ctypes mirror of struct nbody_diag has the layout the C compiler gives include/nbody.h."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DIAG_FIELDS = ("step", "n_bodies", "coincident_pairs", "mass", "momentum", "center_of_mass", "angular_momentum",
               "kinetic", "potential")


def test_diagnostics_symbols_are_exported_and_bound(nb):
    for name in ("nbody_get_diagnostics", "nbody_group_diagnostics"):
        assert name in nb.SYMBOLS
        fn = getattr(nb.lib, name)
        assert fn.restype is ctypes.c_int
        assert fn.argtypes == nb.SYMBOLS[name][1]
    with open(os.path.join(ROOT, "include", "nbody.h")) as f:
        h = f.read()
    assert "typedef struct nbody_diag {" in h
    assert "int nbody_get_diagnostics(nbody_ctx* ctx, nbody_diag* out, double* phi);" in h
    assert "int nbody_group_diagnostics(nbody_ctx** ctxs, int world, nbody_diag* out, double* phi);" in h


def test_diagnostics_null_arguments_are_invalid(nb):
    d = nb.Diag()
    assert nb.lib.nbody_get_diagnostics(None, ctypes.byref(d), None) == -1
    assert b"NULL" in nb.lib.nbody_last_error_string()
    assert nb.lib.nbody_get_diagnostics(None, None, None) == -1
    assert nb.lib.nbody_group_diagnostics(None, 1, ctypes.byref(d), None) == -1
    arr = (ctypes.c_void_p * 1)(None)
    assert nb.lib.nbody_group_diagnostics(arr, 1, None, None) == -1
    assert nb.lib.nbody_group_diagnostics(arr, 0, ctypes.byref(d), None) == -1


def test_diag_struct_layout(nb):
    """Three int64_t, then eight doubles (mass, momentum[2], center_of_mass[2], angular_momentum, kinetic, potential)."""
    assert [f[0] for f in nb.Diag._fields_] == list(DIAG_FIELDS)
    want = {"step": 0, "n_bodies": 8, "coincident_pairs": 16, "mass": 24, "momentum": 32, "center_of_mass": 48,
            "angular_momentum": 64, "kinetic": 72, "potential": 80}
    assert {k: getattr(nb.Diag, k).offset for k in DIAG_FIELDS} == want
    assert ctypes.sizeof(nb.Diag) == 88


def test_diag_struct_layout_matches_the_c_compiler(nb, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "nbody.h"\n'
                   'int main(void) {\n  printf("%zu", sizeof(nbody_diag));\n' +
                   "".join('  printf(" %%zu", offsetof(nbody_diag, %s));\n' % k for k in DIAG_FIELDS) +
                   "  return 0;\n}\n")
    exe = tmp_path / "layout"
    cc = os.environ.get("CC", "cc")
    try:
        subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    except (OSError, subprocess.CalledProcessError) as e:   # the library build needs a C compiler: so does this test
        pytest.fail("cannot compile the layout probe: %s" % e)
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got[0] == ctypes.sizeof(nb.Diag)
    assert got[1:] == [getattr(nb.Diag, k).offset for k in DIAG_FIELDS]
