#!/usr/bin/env python3
"""clearance.npz: turtle_stepper_clearance_n as include/turtle_amd.h defines it, evaluated over the
real reference (run in the build container; see generate.py for the conventions).

Per case <c> of clearance_cases.CASES: <c>_observer [4][3], <c>_target [6][3], <c>_fraction [130],
<c>_layer; the expected <c>_clearance, <c>_sample, <c>_n_data [4][6] (lines without a sample keep
clearance_cases.SENTINEL); and the whole profile <c>_profile (NaN where a sample was skipped) and
<c>_data_index [4][6][130].  tests/clearance_cases.py, restate(), is the definition.

The generator prints and asserts what the GPU tests lean on: the lowest-to-second gap of every line
is above 1e-5 m, and no sample's data index changes when its latitude and longitude move by 4 ulp."""
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
import clearance_cases as CC  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
STORED = CC.OUTPUTS + ("profile", "data_index")


def main():
    out = {}
    tmp = tempfile.mkdtemp(prefix="turtle_clearance_")
    try:
        for case in CC.CASES:
            geo = NC.reference_geometry(case, os.path.join(tmp, case))
            stepper = HC.reference_stepper(geo)
            observer, target, fraction = HC.observers(case, stepper), CC.targets(case, stepper), CC.fractions()
            r = CC.restate(stepper, observer, target, fraction, CC.LAYER[case])
            moved = CC.data_is_robust(stepper, r["latitude"], r["longitude"], r["data_index"], CC.LAYER[case])
            stepper.destroy()
            NC.destroy(geo)
            out[case + "_observer"], out[case + "_target"], out[case + "_fraction"] = observer, target, fraction
            out[case + "_layer"] = np.int32(CC.LAYER[case])
            for name in STORED:
                out[f"{case}_{name}"] = r[name]
            gap = CC.gaps(r["profile"]).min()
            print(case, "minima: %s" % np.array2string(r["clearance"], precision=1, max_line_width=200))
            print(case, "samples:", r["sample"].tolist(), "n_data:", r["n_data"].tolist())
            print(case, "smallest lowest-to-second gap: %.3e m; data indices that move within %d ulp: %d"
                  % (gap, CC.NUDGE, moved))
            assert gap > 1e-5, (case, gap)
            assert moved == 0, (case, moved)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    path = os.path.join(OUT, "clearance.npz")
    np.savez_compressed(path, **out)
    print("clearance.npz", os.path.getsize(path), "bytes; errors:", R.errors())


if __name__ == "__main__":
    main()
