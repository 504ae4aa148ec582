#!/usr/bin/env python3
"""End-to-end time of nbody_get_diagnostics (host clock around the synchronising call, phi returned): the stock initial
condition with random velocities, N = 262144 from an fp32 context and N = 1048576 from an fp64 context.  Kernel times come
from a separate `rocprofv3 --kernel-trace --stats` run of this script (kernels diag_potential / diag_moments).
    python3 diag_probe.py [reps]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)
import torch  # noqa: F401,E402  (one ROCm runtime per process: tests/conftest.py)
import numpy as np  # noqa: E402
import ppa_nbody_collisions_amd as nb  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
for precision, n in ((nb.F32, 262144), (nb.F64, 1048576)):
    cfg = nb.stock_config(particleCount=n)
    b = nb.init_bodies(cfg, precision)
    b.Velocities[:] = np.random.default_rng(1).uniform(-3, 3, size=(n, 2)).astype(b.dtype)
    st = nb.Stepper(cfg, precision=precision)
    st.upload(b)
    d = st.diagnostics(potential=True)                    # warm-up: code objects, lazy buffers
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        d = st.diagnostics(potential=True)
        ms.append((time.perf_counter() - t0) * 1e3)
    st.close()
    print(json.dumps({"precision": "fp64" if precision == nb.F64 else "fp32", "n": n, "reps": reps,
                      "ms_per_call_median": float(np.median(ms)), "ms_per_call_min": min(ms),
                      "pairs_per_s_end_to_end": float(n) * (n - 1) / (np.median(ms) * 1e-3),
                      "potential": d["potential"], "kinetic": d["kinetic"],
                      "coincident_pairs": d["coincident_pairs"]}), flush=True)
