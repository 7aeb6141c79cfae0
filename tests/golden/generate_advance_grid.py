#!/usr/bin/env python3
"""advance_grid.npz: the lines of sight of traverse.npz advanced by a column-depth budget and a
distance limit through rock whose density is a box of voxels, computed by the REAL reference.  Build
container only:

    make -C oracle ref && python tests/golden/generate_advance_grid.py

The geometries and rays are those of generate_traverse.py (the 1201^2 tiles of
tests/traverse_cases.py, the "ground" and "c2" recipes of 1000 rays each, their ceilings).  The box
is tests/advance_grid_cases.py's: east-north-up at the middle of the tile, its frame from the
reference's own transforms, its voxels from the formula there (the file does not hold them); outside
it the media have advance.npz's densities.  The reference (turtle_stepper_range_set(0)) runs, ray by
ray with a fresh stepper history, the loop that include/turtle_amd.h states for
turtle_stepper_advance_grid_n (advance_grid_cases.reference_loop): first uncut, recording (d, X)
after every step, which gives each ray its full depth D, its path T and the profile that the recipe
draws a budget and a limit from; then with them.  Stored per case and recipe: budget, distance_max,
density, D, T, and the loop's position, index, depth, distance, n_steps and status; once: the box's
origin, axis, size, n, medium and block.  The rays themselves are traverse.npz's.  What the fixture
is meant to hold is asserted here, on the reference's own run."""
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

import advance_grid_cases as AG  # noqa: E402
import generate_traverse as GT  # noqa: E402
import traverse_cases as TC  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def reference_frame():
    """the box's origin and axes by the reference's own transforms"""
    lat, lon = np.full(3, AG.LATITUDE), np.full(3, AG.LONGITUDE)
    axis = R.ecef_from_horizontal(lat, lon, np.array([90.0, 0.0, 0.0]), np.array([0.0, 0.0, 90.0]))   # east, north, up
    origin = R.ecef_from_geodetic(lat[:1], lon[:1], np.array([AG.HEIGHT])).reshape(3)
    return origin + AG.OFFSET[0] * axis[0] + AG.OFFSET[1] * axis[1] + AG.OFFSET[2] * axis[2], axis


def main():
    if not R.available():
        sys.exit("oracle/_ref/libturtle_ref.so missing: run `make -C oracle ref`")
    rays = np.load(os.path.join(OUT, "traverse.npz"))
    crossings = np.load(os.path.join(OUT, "crossings.npz"))
    rng = np.random.default_rng(AG.SEED)
    origin, axis = reference_frame()
    box = AG.golden_box(origin, axis)
    out = dict(origin=origin, axis=axis, size=np.array(AG.SIZE), n=np.array(AG.N, dtype=np.int32),
               medium=np.int32(AG.MEDIUM), block=np.array(AG.BLOCK, dtype=np.int32),
               block_density=np.float64(AG.BLOCK_DENSITY))
    rock_steps = voxel_steps = face_rays = spent_inside = far_inside = 0
    for case in TC.CASES:          # (with the recipes below: AG.BATCHES' order, one generator)
        tmp = tempfile.mkdtemp(prefix="turtle_advance_grid_")
        try:
            m = R.RefMap.load(TC.write_tile(tmp, case))
            st = AG.reference_stepper(case, m)
            for recipe in ("ground", "c2"):
                key = f"{case}_{recipe}_"
                pos, d = GT.rays(st, recipe, len(TC.layers(case)) - 1)
                # the same rays as traverse.npz's, bit for bit
                assert np.array_equal(pos, rays[key + "position"]) and np.array_equal(d, rays[key + "direction"])
                n = pos.shape[0]
                ceiling = float(rays[key + "ceiling"])
                media = rays[key + "length"].shape[0]
                density = AG.DENSITY[media]
                profiles = []
                tally = np.zeros((n, 3), dtype=np.int64)
                full = AG.reference_loop(st, pos, d, density, box, np.full(n, AG.INF), None, ceiling, GT.MAX_STEPS,
                                         record=profiles, tally=tally)
                # uncut, the loop is traverse's
                assert np.array_equal(full["index"], rays[key + "index"])
                assert np.array_equal(full["n_steps"], rays[key + "n_steps"])
                b = AG.budgets(rng, profiles, pos, d, rays[key + "index"], crossings[key + "offset"],
                               crossings[key + "distance"], density, box)
                assert np.array_equal(b["T"], full["distance"]) and np.array_equal(b["D"], full["depth"])
                t = AG.reference_loop(st, pos, d, density, box, b["budget"], b["distance_max"], ceiling, GT.MAX_STEPS)
                assert np.array_equal(t["status"], b["status"]), np.flatnonzero(t["status"] != b["status"])
                moving = b["T"] > 0
                assert (b["margin"][moving] >= AG.MARGIN).all()
                counts = np.bincount(t["status"], minlength=5)
                assert counts[AG.SPENT] > 0 and counts[AG.DISTANCE] > 0 and counts[AG.MAX_STEPS] == 0
                rock = t["index"][:, 0] == AG.MEDIUM
                within = np.array([AG.inside(box, p) for p in t["position"]])
                s_in = int(((t["status"] == AG.SPENT) & rock & within).sum())
                f_in = int(((t["status"] == AG.DISTANCE) & rock & within).sum())
                spent_inside += s_in
                far_inside += f_in
                rock_steps += int(tally[:, 0].sum())
                voxel_steps += int(tally[:, 1].sum())
                face_rays += int((tally[:, 2] > 0).sum())
                out.update({key + name: b[name] for name in ("budget", "distance_max", "T", "D")})
                out[key + "density"] = density
                out.update({key + name: t[name] for name in AG.OUTPUTS})
                print(f"{case:5s} {recipe:6s}: status {counts}, in the box: SPENT {s_in}, DISTANCE {f_in}; rock steps "
                      f"{int(tally[:, 0].sum())}, met a voxel {int(tally[:, 1].sum())}, rays through a face "
                      f"{int((tally[:, 2] > 0).sum())}; least margin {b['margin'].min():.2e} T, stop vs recipe "
                      f"{np.abs(t['distance'] - b['stop']).max():.2e} m", flush=True)
            st.destroy()
            m.destroy()
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    print(f"steps begun in the rock: {rock_steps}, of which {voxel_steps} met a voxel; {face_rays} rays met a face "
          f"in mid-step; in the box: {spent_inside} SPENT, {far_inside} cut by DISTANCE")
    assert voxel_steps >= 0.3 * rock_steps and face_rays >= 100 and spent_inside >= 200 and far_inside >= 50
    np.savez_compressed(os.path.join(OUT, "advance_grid.npz"), **out)
    print("wrote", os.path.join(OUT, "advance_grid.npz"))


if __name__ == "__main__":
    main()
