#!/usr/bin/env python3
"""advance_exp.npz: the lines of sight of traverse.npz advanced by a column-depth budget and a
distance limit through air whose density falls with altitude, computed by the REAL reference.  Build
container only:

    make -C oracle ref && python tests/golden/generate_advance_exp.py

The geometries and rays are those of generate_traverse.py (the 1201^2 tiles of
tests/traverse_cases.py, the "ground" and "c2" recipes of 1000 rays each, their ceilings).  Rock is
uniform at 2650 kg/m^3 (scale height HUGE_VAL), the middle layer of "two" uniform at 1000, air is
1.205 kg/m^3 at altitude 0 with a scale height of 8400 m.  The reference
(turtle_stepper_range_set(0)) runs, ray by ray with a fresh stepper history, the loop that
include/turtle_amd.h states for turtle_stepper_advance_exp_n (advance_exp_cases.reference_loop):
first uncut, recording (d, X) after every step, which gives each ray its full depth D, its path T
and the profile that tests/advance_exp_cases.py's recipe draws a budget and a limit from; then with
them.  Stored per case and recipe: budget, distance_max, density, scale_height, D, T, and the loop's
position, index, depth, distance, n_steps and status.  The rays themselves are traverse.npz's."""
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

import advance_exp_cases as AE  # noqa: E402
import generate_traverse as GT  # noqa: E402
import traverse_cases as TC  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def main():
    if not R.available():
        sys.exit("oracle/_ref/libturtle_ref.so missing: run `make -C oracle ref`")
    rays = np.load(os.path.join(OUT, "traverse.npz"))
    crossings = np.load(os.path.join(OUT, "crossings.npz"))
    rng = np.random.default_rng(AE.SEED)
    out = {}
    spent_in_air = far_in_air = 0
    for case in TC.CASES:          # (with the recipes below: AE.BATCHES' order, one generator)
        tmp = tempfile.mkdtemp(prefix="turtle_advance_exp_")
        try:
            m = R.RefMap.load(TC.write_tile(tmp, case))
            st = AE.reference_stepper(case, m)
            for recipe in ("ground", "c2"):
                key = f"{case}_{recipe}_"
                pos, d = GT.rays(st, recipe, len(TC.layers(case)) - 1)
                # the same rays as traverse.npz's, bit for bit
                assert np.array_equal(pos, rays[key + "position"]) and np.array_equal(d, rays[key + "direction"])
                n = pos.shape[0]
                ceiling = float(rays[key + "ceiling"])
                media = rays[key + "length"].shape[0]
                density, scale = AE.DENSITY[media], AE.SCALE_HEIGHT[media]
                profiles = []
                full = AE.reference_loop(st, pos, d, density, scale, np.full(n, AE.INF), None, ceiling,
                                         GT.MAX_STEPS, record=profiles)
                # uncut, the loop is traverse's
                assert np.array_equal(full["index"], rays[key + "index"])
                assert np.array_equal(full["n_steps"], rays[key + "n_steps"])
                b = AE.budgets(rng, profiles, rays[key + "index"], crossings[key + "offset"],
                               crossings[key + "distance"], density, scale)
                assert np.array_equal(b["T"], full["distance"]) and np.array_equal(b["D"], full["depth"])
                t = AE.reference_loop(st, pos, d, density, scale, b["budget"], b["distance_max"], ceiling,
                                      GT.MAX_STEPS)
                assert np.array_equal(t["status"], b["status"]), np.flatnonzero(t["status"] != b["status"])
                moving = b["T"] > 0
                assert (b["margin"][moving] >= AE.MARGIN).all()
                air = t["index"][:, 0] == media - 1
                s_air = int(((t["status"] == AE.SPENT) & air).sum())
                f_air = int(((t["status"] == AE.DISTANCE) & air).sum())
                spent_in_air += s_air
                far_in_air += f_air
                out.update({key + name: b[name] for name in ("budget", "distance_max", "T", "D")})
                out[key + "density"], out[key + "scale_height"] = density, scale
                out.update({key + name: t[name] for name in AE.OUTPUTS})
                print(f"{case:5s} {recipe:6s}: status {np.bincount(t['status'], minlength=5)}, in air: SPENT "
                      f"{s_air}, DISTANCE {f_air}; least margin {b['margin'].min():.2e} T, stop vs recipe "
                      f"{np.abs(t['distance'] - b['stop']).max():.2e} m, steps {int(full['n_steps'].sum())}")
            st.destroy()
            m.destroy()
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    print(f"in the exponential medium: {spent_in_air} SPENT, {far_in_air} cut by DISTANCE")
    assert spent_in_air >= 200 and far_in_air >= 100
    np.savez_compressed(os.path.join(OUT, "advance_exp.npz"), **out)
    print("wrote", os.path.join(OUT, "advance_exp.npz"))


if __name__ == "__main__":
    main()
