#!/usr/bin/env python3
"""viewshed.npz: turtle_stepper_viewshed_n as include/turtle_amd.h defines it, evaluated over the
real reference (run in the build container; see generate.py for the conventions).

The inputs are those of horizon.npz (tests/horizon_cases.py) and are not stored again.  Per case
<c> of viewshed_cases.CASES and target height <h> of viewshed_cases.TARGET_HEIGHTS (h0, h10):
<c>_<h>_visible int8, <c>_<h>_sine, <c>_<h>_horizon [4][5][130] and <c>_<h>_n_visible int32 [4][5];
<c>_<h>_target_height holds the height.  tests/viewshed_cases.py, restate(), is the definition."""
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
import viewshed_cases as VC  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def main():
    out = {}
    tmp = tempfile.mkdtemp(prefix="turtle_viewshed_")
    try:
        for case in VC.CASES:
            geo = NC.reference_geometry(case, os.path.join(tmp, case))
            stepper = HC.reference_stepper(geo)
            position, azimuth, distance = HC.observers(case, stepper), HC.azimuths(), HC.distances()
            for height in VC.TARGET_HEIGHTS:
                r = VC.restate(stepper, position, azimuth, distance, VC.LAYER[case], height)
                key = f"{case}_{VC.tag(height)}"
                out[key + "_target_height"] = np.float64(height)
                for name, value in r.items():
                    out[f"{key}_{name}"] = value
                v = r["visible"]
                print(key, "with data:", int((v >= 0).sum()), "visible:", int((v == 1).sum()), "skipped:",
                      int((v < 0).sum()), "smallest margin: %.3e" % VC.margins(r["sine"], r["horizon"], v).min())
            stepper.destroy()
            NC.destroy(geo)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    path = os.path.join(OUT, "viewshed.npz")
    np.savez_compressed(path, **out)
    print("viewshed.npz", os.path.getsize(path), "bytes; errors:", R.errors())


if __name__ == "__main__":
    main()
