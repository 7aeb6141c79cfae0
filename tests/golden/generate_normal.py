#!/usr/bin/env python3
"""normal.npz: turtle_stepper_normal_n as include/turtle_amd.h defines it, evaluated over the real
reference (run in the build container; see generate.py for the conventions).

The reference computes every part it has a function for -- turtle_ecef_to_geodetic, the
elevations and gradients of maps and stacks, turtle_projection_project -- and the geoid's
share and the tangent arithmetic (steps 5 and 6 of the definition) are evaluated in IEEE
doubles in the stated operand order: tests/normal_cases.py, restate().  Per case <c> of
normal_cases.CASES: <c>_position, <c>_layer, the expected <c>_data_index and <c>_normal (rows
without data hold SENTINEL), and for diagnosis <c>_latitude, <c>_longitude, <c>_glat, <c>_glon,
<c>_hs."""
import os
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import ref_ffi as R  # noqa: E402
import normal_cases as NC  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
SENTINEL = -7.0


def main():
    out = {}
    tmp = tempfile.mkdtemp(prefix="turtle_normal_")
    try:
        for case in NC.CASES:
            geo = NC.reference_geometry(case, os.path.join(tmp, case))
            position, layer = NC.positions(case)
            r = NC.restate(geo, position, layer, SENTINEL)
            NC.destroy(geo)
            out[case + "_position"], out[case + "_layer"] = position, layer
            for name, value in r.items():
                out[f"{case}_{name}"] = value
            print(case, position.shape[0], "points; data_index -1, 0, 1:",
                  [int((r["data_index"] == k).sum()) for k in (-1, 0, 1)])
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    path = os.path.join(OUT, "normal.npz")
    np.savez_compressed(path, **out)
    print("normal.npz", os.path.getsize(path), "bytes; errors:", R.errors())


if __name__ == "__main__":
    main()
