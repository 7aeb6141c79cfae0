#!/usr/bin/env python3
"""advance.npz: the lines of sight of traverse.npz advanced by a column-depth budget and a distance
limit, computed by the REAL reference.  Build container only:

    make -C oracle ref && python tests/golden/generate_advance.py

The geometries and rays are those of generate_traverse.py (the 1201^2 tiles of
tests/traverse_cases.py, the "ground" and "c2" recipes of 1000 rays each, their ceilings).  Each ray
gets a budget and a distance limit from tests/advance_cases.py's recipe, a pure function of
traverse.npz and crossings.npz (densities 2650 / 1.205 kg/m^3 for rock / air, 2650 / 1000 / 1.205
with the layer between them), and the reference (turtle_stepper_range_set(0)) runs, ray by ray with
a fresh stepper history, the loop that include/turtle_amd.h states for turtle_stepper_advance_n
(advance_cases.reference_loop).  Stored per case and recipe: budget, distance_max, density, and the
loop's position, index, depth, distance, n_steps and status.  The rays themselves are
traverse.npz's."""
from __future__ import annotations

import os
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import ref_ffi as R  # noqa: E402

import advance_cases as AC  # noqa: E402
import generate_traverse as GT  # noqa: E402
import traverse_cases as TC  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def main():
    if not R.available():
        sys.exit("oracle/_ref/libturtle_ref.so missing: run `make -C oracle ref`")
    rays = np.load(os.path.join(OUT, "traverse.npz"))
    given = AC.golden_budgets(rays, np.load(os.path.join(OUT, "crossings.npz")))
    out = {}
    for case in TC.CASES:
        tmp = tempfile.mkdtemp(prefix="turtle_advance_")
        try:
            m = R.RefMap.load(TC.write_tile(tmp, case))
            st = AC.reference_stepper(case, m)
            for recipe in ("ground", "c2"):
                key = f"{case}_{recipe}_"
                pos, d = GT.rays(st, recipe, len(TC.layers(case)) - 1)
                # the same rays as traverse.npz's, bit for bit
                assert np.array_equal(pos, rays[key + "position"]) and np.array_equal(d, rays[key + "direction"])
                b = given[case, recipe]
                t = AC.reference_loop(st, pos, d, b["density"], b["budget"], b["distance_max"],
                                      float(rays[key + "ceiling"]), GT.MAX_STEPS)
                assert np.array_equal(t["status"], b["status"]), np.flatnonzero(t["status"] != b["status"])
                out.update({key + name: b[name] for name in ("budget", "distance_max", "density")})
                out.update({key + name: t[name] for name in AC.OUTPUTS})
                print(f"{case:5s} {recipe:6s}: status {np.bincount(t['status'], minlength=5)}, SPENT in rock "
                      f"{int(((t['status'] == AC.SPENT) & (t['index'][:, 0] == 0)).sum())}, least margin "
                      f"{b['margin'].min():.2e} T, stop vs numpy {np.abs(t['distance'] - b['stop']).max():.2e} m")
            st.destroy()
            m.destroy()
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    np.savez_compressed(os.path.join(OUT, "advance.npz"), **out)
    print("wrote", os.path.join(OUT, "advance.npz"))


if __name__ == "__main__":
    main()
