#!/usr/bin/env python3
"""horizon.npz: turtle_stepper_horizon_n as include/turtle_amd.h defines it, evaluated over the real
reference (run in the build container; see generate.py for the conventions).

The reference computes every part it has a function for -- turtle_ecef_to_geodetic,
turtle_ecef_from_horizontal, turtle_stepper_position -- and the frame, the dot product and the
maximum are evaluated in IEEE doubles in the stated operand order: tests/horizon_cases.py,
restate().  Per case <c> of horizon_cases.CASES: the inputs <c>_position, <c>_azimuth,
<c>_distance, <c>_layer; the expected <c>_elevation, <c>_sample, <c>_range (lines without a
sample hold SENTINEL); and the whole profile <c>_sine, <c>_data_index [n][n_az][n_d] (NaN / -1
where a sample was skipped)."""
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
import horizon_cases as HC  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def main():
    out = {}
    tmp = tempfile.mkdtemp(prefix="turtle_horizon_")
    try:
        for case in HC.CASES:
            geo = NC.reference_geometry(case, os.path.join(tmp, case))
            stepper = HC.reference_stepper(geo)
            position, azimuth, distance = HC.observers(case, stepper), HC.azimuths(), HC.distances()
            r = HC.restate(stepper, position, azimuth, distance, HC.LAYER[case])
            stepper.destroy()
            NC.destroy(geo)
            out[case + "_position"], out[case + "_azimuth"], out[case + "_distance"] = position, azimuth, distance
            out[case + "_layer"] = np.int32(HC.LAYER[case])
            for name, value in r.items():
                out[f"{case}_{name}"] = value
            print(case, "samples:", r["sample"].tolist(), "skipped:", int(np.isnan(r["sine"]).sum()),
                  "smallest gap: %.3e" % HC.gaps(r["sine"]).min())
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    path = os.path.join(OUT, "horizon.npz")
    np.savez_compressed(path, **out)
    print("horizon.npz", os.path.getsize(path), "bytes; errors:", R.errors())


if __name__ == "__main__":
    main()
