#!/usr/bin/env python3
"""traverse.npz: lines of sight through every medium, computed by the REAL reference.  Build
container only:

    make -C oracle ref && python tests/golden/generate_traverse.py

For each geometry of tests/traverse_cases.py ("hgt": the 1201^2 sin.cos tile, one map layer;
"two": the same tile in two layers, offsets -0.5 / 0, three media; "rough": synth.rough_nodes),
the reference (turtle_stepper_range_set(0)) runs, ray by ray with a fresh stepper history, the loop
of its examples/example-stepper.c:128-140 with the stop the library adds (the ray has left the
data):

    turtle_stepper_step(s, pos, NULL, NULL, NULL, &alt, NULL, NULL, idx);
    while (idx[0] >= 0 && alt < altitude_max && steps < max_steps) {
            m = idx[0]; turtle_stepper_step(s, pos, dir, NULL, NULL, &alt, NULL, &ds, idx);
            length[m][r] += ds; steps++; if (idx[0] != m) crossings++;
    }

on two recipes of 1000 rays: "ground", from 0.5 m above the top layer's ground, azimuth
U[0, 360), elevation U[0, 30] degrees, no ceiling (in "two", whose flat layers
never end, 2000 m); "c2", BASELINE's C2 recipe (500 m above it,
elevation -10 .. -1 degrees) with altitude_max = 2000 m, its last 16 rays starting 2500 m above
the ground (above the ceiling) and the 16 before them outside the tile.  Stored per case and
recipe: the origins and directions (the reference's own position and ecef_from_horizontal), the
ceiling, and the loop's index, length [media][n], step and crossing counts."""
from __future__ import annotations

import ctypes as C
import os
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_ffi as R  # noqa: E402
from turtle_amd import synth  # noqa: E402

import traverse_cases as TC  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
RAYS = 1000
SPECIAL = 16
MAX_STEPS = 1000000
D = C.c_double


def ref_stepper(case, m):
    st = R.RefStepper()
    st.range_set(0.0)
    if case == "two":
        for off in (-0.5, 0.0):
            st.add_layer()
            st.add_flat(off)
            st.add_map(m, off)
    else:
        st.add_map(m, 0.0)
    return st


def rays(st, recipe, top):
    box_lat, box_lon = (TC.LAT0, TC.LAT0 + 1), (TC.LON0, TC.LON0 + 1)
    if recipe == "ground":
        lat, lon, az, el = synth.uniform_rays(RAYS, box_lat, box_lon, seed=0x7A5E, el_range=(0.0, 30.0))
        height = np.full(RAYS, 0.5)
    else:
        lat, lon, az, el = synth.uniform_rays(RAYS, box_lat, box_lon, seed=0x5EED2026)
        height = np.full(RAYS, 500.0)
        height[-SPECIAL:] = 2500.0
    pos = np.empty((RAYS, 3))
    for r in range(RAYS):
        rc, p, di = st.position(lat[r], lon[r], height[r], top)
        assert rc == 0 and di >= 0, (r, rc, di, R.errors())
        pos[r] = p
    if recipe == "c2":  # outside the tile (its south-west rim and beyond)
        k = np.arange(SPECIAL)
        out = slice(RAYS - 2 * SPECIAL, RAYS - SPECIAL)
        pos[out] = R.ecef_from_geodetic(TC.LAT0 - 0.01 - 0.01 * k, TC.LON0 + 0.5 + 0.01 * k,
                                        np.full(SPECIAL, 1000.0))
    d = R.ecef_from_horizontal(lat, lon, az, el)
    return np.ascontiguousarray(pos), np.ascontiguousarray(d)


def loop(st, pos, d, altitude_max, media):
    L = R.lib()
    step = L.turtle_stepper_step
    n = pos.shape[0]
    index = np.empty((n, 2), dtype=np.int32)
    length = np.zeros((media, n))
    n_steps = np.empty(n, dtype=np.int32)
    n_cross = np.empty(n, dtype=np.int32)
    p, q = (D * 3)(), (D * 3)()
    alt, ds = D(), D()
    idx = (C.c_int * 2)()
    for r in range(n):
        st.reset()
        p[:] = pos[r]
        q[:] = d[r]
        assert step(st.h, p, None, None, None, C.byref(alt), None, None, idx) == 0
        k = crossings = 0
        while idx[0] >= 0 and alt.value < altitude_max and k < MAX_STEPS:
            m = idx[0]
            assert step(st.h, p, q, None, None, C.byref(alt), None, C.byref(ds), idx) == 0
            length[m, r] += ds.value
            k += 1
            if idx[0] != m:
                crossings += 1
        index[r] = idx[:]
        n_steps[r] = k
        n_cross[r] = crossings
    return index, length, n_steps, n_cross


def main():
    if not R.available():
        sys.exit("oracle/_ref/libturtle_ref.so missing: run `make -C oracle ref`")
    out = {}
    for case in TC.CASES:
        tmp = tempfile.mkdtemp(prefix="turtle_traverse_")
        try:
            m = R.RefMap.load(TC.write_tile(tmp, case))
            st = ref_stepper(case, m)
            media = len(TC.layers(case)) + 1
            # (flat layers have no end: in "two" a ray that climbs stops at a ceiling or nowhere)
            for recipe, ceiling in (("ground", 2000.0 if case == "two" else np.inf), ("c2", 2000.0)):
                pos, d = rays(st, recipe, len(TC.layers(case)) - 1)
                index, length, n_steps, n_cross = loop(st, pos, d, ceiling, media)
                key = f"{case}_{recipe}_"
                out.update({key + "position": pos, key + "direction": d, key + "ceiling": np.float64(ceiling),
                            key + "index": index, key + "length": length, key + "n_steps": n_steps,
                            key + "n_crossings": n_cross})
                print(f"{case:5s} {recipe:6s}: {int(n_steps.sum())} steps, crossings max {n_cross.max()} "
                      f"mean {n_cross.mean():.2f}, final media {np.bincount(index[:, 0] + 1)}")
            st.destroy()
            m.destroy()
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    out["rough_nodes_sha"] = np.array(__import__("hashlib").sha256(TC.nodes("rough").tobytes()).hexdigest())
    np.savez_compressed(os.path.join(OUT, "traverse.npz"), **out)
    print("wrote", os.path.join(OUT, "traverse.npz"))


if __name__ == "__main__":
    main()
