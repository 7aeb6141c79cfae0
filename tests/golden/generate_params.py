#!/usr/bin/env python3
"""params.npz: traces at slope and resolution other than the defaults, computed by the REAL
reference.  Build container only:

    make -C oracle ref && python tests/golden/generate_params.py

For the "hgt" and "rough" tiles of tests/traverse_cases.py (1201^2 nodes at 45N 3E, one map layer,
turtle_stepper_range_set(0)) and three recipes of 1000 rays -- "ground" (generate_traverse.py's:
elevation 0 .. 30 degrees from 0.5 m above the ground; from 2 m on the rough tile, see
params_cases.GROUND_HEIGHT), "c2" (generate_traverse.py's: BASELINE's C2 with its last 16 rays
2500 m up and the 16 before them outside the tile) and "graze" (30 m above the middle of the
tile, elevation -3 .. 1 degrees) -- the reference runs the harness
loop (turtle_stepper_step until the medium changes, at most 100 000 steps) at every setting of
tests/params_cases.py (`steep` on the smooth tile only).

Stored once per case and recipe: the origins and directions (the reference's own
turtle_stepper_position and turtle_ecef_from_horizontal).  Stored per setting: the final index,
path length and step count."""
from __future__ import annotations

import hashlib
import os
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_ffi as R  # noqa: E402

import params_cases as PC  # noqa: E402
import traverse_cases as TC  # noqa: E402

import generate_traverse as GT  # noqa: E402  (this directory: the "ground" and "c2" recipes)

OUT = os.path.dirname(os.path.abspath(__file__))
LIMIT = 1 << 20


def rays(st, case, recipe):
    if recipe == "c2":
        assert GT.RAYS == PC.RAYS
        return GT.rays(st, recipe, 0)
    lat, lon, height, az, el = PC.draws(case, recipe)
    pos = np.empty((PC.RAYS, 3))
    for r in range(PC.RAYS):
        rc, pos[r], di = st.position(lat[r], lon[r], height[r], 0)
        assert rc == 0 and di >= 0, (r, rc, di, R.errors())
    return np.ascontiguousarray(pos), np.ascontiguousarray(R.ecef_from_horizontal(lat, lon, az, el))


def main():
    if not (R.available() and R.driver_available()):
        sys.exit("oracle/_ref/libturtle_ref.so missing: run `make -C oracle ref`")
    out = {}
    for case in PC.CASES:
        tmp = tempfile.mkdtemp(prefix="turtle_params_")
        try:
            tile = TC.write_tile(tmp, case)
            m = R.RefMap.load(tile)
            st = GT.ref_stepper(case, m)
            for recipe in PC.RECIPES:
                pos, d = rays(st, case, recipe)
                out[f"{case}_{recipe}_position"], out[f"{case}_{recipe}_direction"] = pos, d
                for name in PC.settings(case):
                    slope, resolution = PC.SETTINGS[name]
                    t = R.trace_map(tile, pos, d, local_range=0.0, slope=slope, resolution=resolution,
                                    max_steps=PC.MAX_STEPS, threads=min(16, os.cpu_count() or 1))
                    k = f"{case}_{recipe}_{name}_"
                    out[k + "index"] = t["index"].astype(np.int8)
                    out[k + "length"], out[k + "n_steps"] = t["length"], t["n_steps"]
                    print(f"{case:5s} {recipe:6s} {name:7s}: {t['total_steps']} steps, max "
                          f"{t['n_steps'].max()}, beyond 32: {(t['n_steps'] > 32).sum()}, beyond 512: "
                          f"{(t['n_steps'] > 512).sum()}, final media {np.bincount(t['index'][:, 0] + 1)}",
                          flush=True)
            st.destroy()
            m.destroy()
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    out["rough_nodes_sha"] = np.array(hashlib.sha256(TC.nodes("rough").tobytes()).hexdigest())
    path = os.path.join(OUT, "params.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print("wrote", path, size, "bytes")
    assert size < LIMIT, "drop a recipe: the fixture must stay below the size limit of a committed file"


if __name__ == "__main__":
    main()
