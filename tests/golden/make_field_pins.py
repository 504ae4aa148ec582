#!/usr/bin/env python3
"""Generates tests/golden/field_pins.npz: probe points and the bits the field evaluation gives at them and at the bodies'
own positions for the states of diag_pins.npz (tests/test_gpu_field.py, "the bits, pinned").  Data only: inputs and
recorded outputs.

    python tests/golden/make_field_pins.py --root DIR

DIR is a built checkout of the commit whose bits are to be kept (make -C ppa-nbody-collisions_amd/csrc), e.g. a git
worktree under build/; the library is loaded from there, what is computed from the inputs is the test's own code (the
pin_field_* functions of test_gpu_field.py).  Needs the GPU.  The fixture is recorded once: a later change of the kernels
must reproduce it, not regenerate it.

Inputs: the states of diag_pins.npz (read, not copied), and per precision 257 points, point 100 on body 5 of the n = 300
state.  Outputs: acc, phi and coincident of Stepper.field() and Stepper.field(points) per state, and of one fp32
StepperBatch of n = 0, 1, 129, 256, 300 at capacity 300.
"""
import argparse
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--root", required=True, help="built checkout whose library computes the pinned outputs")
    ap.add_argument("--out", default=os.path.join(HERE, "field_pins.npz"))
    a = ap.parse_args()
    try:
        import torch  # noqa: F401  (one ROCm runtime per process: tests/conftest.py)
    except ImportError:
        pass
    sys.path.insert(0, os.path.abspath(a.root))
    import ppa_nbody_collisions_amd as nb
    assert os.path.dirname(os.path.abspath(nb.__file__)).startswith(os.path.abspath(a.root)), nb.__file__
    sys.path.insert(0, os.path.dirname(HERE))
    import test_gpu_diagnostics as dg
    import test_gpu_field as t

    with np.load(dg.PINS) as z:
        states = {k: z[k] for k in z.files if k.startswith("in_")}
    pins = {}
    for precision in (nb.F32, nb.F64):
        pins.update(t.pin_field_points(nb, states, precision))
    for precision in (nb.F32, nb.F64):
        for n in dg.PIN_SIZES:
            pins.update(t.pin_field_stepper(nb, states, pins, precision, n))
    pins.update(t.pin_field_batch(nb, states, pins))
    np.savez_compressed(a.out, **pins)
    print("%s: %d arrays, %d bytes" % (a.out, len(pins), os.path.getsize(a.out)))
    for k in sorted(pins):
        if k.endswith("_coincident"):
            print(k, pins[k].tolist())


if __name__ == "__main__":
    main()
