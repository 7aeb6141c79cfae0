#!/usr/bin/env python3
"""rough.npz: traces and single steps over rough and void ground, and ECEF -> geodetic deep below
the ellipsoid, computed by the REAL reference.  Build container only:

    make -C oracle ref && python tests/golden/generate_rough.py

For each tile of tests/rough_cases.py ("rough": synth.rough_nodes(1201, 1, 800); "void": the same
with HGT voids) the reference (one map layer, turtle_stepper_range_set(0)) runs, ray by ray, the
harness loop -- turtle_stepper_step until the medium changes -- on 10 000 rays of each recipe
("c2": 500 m above the ground, elevation -10 .. -1 degrees; "ground": 0.5 m above it, elevation
-30 .. 30 degrees) and, on the void tile, on 1 000 rays aimed at the edge of each void block
("edge0" .. "edge3").  Stored per tile and recipe: the final index, path length and step count.

Per-step records: the first 2 000 rays of "ground", 32 calls of turtle_stepper_step each (through
every medium, until the ray leaves the data): the step length and index of each call.

Deep points: 2 000 geodetic points 25 .. 40 km below the ellipsoid at every latitude, taken to
ECEF and back by the reference.

The origins, directions, positions, per-step lengths and deep points are 8-byte floats that do not
compress: what the reference computed for them is stored as the sha256 of the arrays (origins,
directions, final positions, per-step lengths and positions, the deep points' ECEF and geodetic
coordinates), so that the file stays small.  tests/test_oracle_golden.py recomputes every
one with the oracle (tests/rough_cases.py's recipes) and checks it against the hash bit for bit,
and the GPU tests (tests/test_gpu_rough.py) take them from there.  The sha256 of each tile's nodes
is stored too, and of the full-size rough tile (3601^2 nodes) that the GPU tests run at full size."""
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

import rough_cases as RC  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
D = C.c_double


def ref_position(st):
    def position(lat, lon, height):
        pos, di = np.empty((lat.size, 3)), np.empty(lat.size, dtype=np.int32)
        for r in range(lat.size):
            rc, pos[r], di[r] = st.position(lat[r], lon[r], height[r], 0)
            assert rc == 0, (r, rc, R.errors())
        return pos, di
    return position


def step_records(st, pos, d):
    """RC.STEPS calls of turtle_stepper_step per ray, a fresh history per ray; ds = NaN and
    index = -2 after the ray has left the data"""
    step = R.lib().turtle_stepper_step
    n = pos.shape[0]
    ds_out = np.full((n, RC.STEPS), np.nan)
    idx_out = np.full((n, RC.STEPS, 2), -2, dtype=np.int32)
    pos_out = np.full((n, RC.STEPS, 3), np.nan)
    p, q = (D * 3)(), (D * 3)()
    ds = D()
    idx = (C.c_int * 2)()
    for r in range(n):
        st.reset()
        p[:] = pos[r]
        q[:] = d[r]
        assert step(st.h, p, None, None, None, None, None, None, idx) == 0
        for k in range(RC.STEPS):
            if idx[0] < 0:
                break
            assert step(st.h, p, q, None, None, None, None, C.byref(ds), idx) == 0
            ds_out[r, k], idx_out[r, k], pos_out[r, k] = ds.value, idx[:], p[:]
    return ds_out, idx_out, pos_out


def main():
    if not R.available():
        sys.exit("oracle/_ref/libturtle_ref.so missing: run `make -C oracle ref`")
    out = {}
    for case in RC.CASES:
        out[f"{case}_nodes_sha"] = np.array(RC.sha(RC.nodes(case)))
        tmp = tempfile.mkdtemp(prefix="turtle_rough_")
        try:
            m = R.RefMap.load(RC.write_tile(tmp, case))
            st = R.RefStepper()
            st.range_set(0.0)
            st.add_map(m, 0.0)
            for recipe in RC.recipes(case):
                pos, d = RC.rays(case, recipe, ref_position(st), R.ecef_from_horizontal)
                st.reset()
                t = st.trace(pos, d, max_steps=1000000)
                assert (t["n_steps"] < 1000000).all()
                k = f"{case}_{recipe}_"
                out.update({k + "origin_sha": np.array(RC.sha(pos)), k + "direction_sha": np.array(RC.sha(d)),
                            k + "position_sha": np.array(RC.sha(t["position"])),
                            k + "index": t["index"].astype(np.int8), k + "length": t["length"],
                            k + "n_steps": t["n_steps"]})
                print(f"{case:5s} {recipe:6s}: {t['n_steps'].sum()} steps, max {t['n_steps'].max()}, "
                      f"final media {np.bincount(t['index'][:, 0] + 1)}", flush=True)
                if recipe == "ground":
                    ds, idx, p = step_records(st, pos[:RC.STEP_RAYS], d[:RC.STEP_RAYS])
                    out.update({f"{case}_steps_ds_sha": np.array(RC.sha(ds)),
                                f"{case}_steps_index": idx.astype(np.int8),
                                f"{case}_steps_position_sha": np.array(RC.sha(p))})
                    print(f"{case:5s} steps: {int(np.isfinite(ds).sum())} records, "
                          f"{int((idx[:, 1:, 0] != idx[:, :-1, 0]).sum())} changes of medium", flush=True)
            st.destroy()
            m.destroy()
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    out["rough3601_nodes_sha"] = np.array(RC.sha(RC.nodes("rough", RC.FULL_N)))
    ecef, geodetic = RC.deep_transforms(R.ecef_from_geodetic, R.ecef_to_geodetic)
    out.update(deep_ecef_sha=np.array(RC.sha(ecef)), deep_geodetic_sha=np.array(RC.sha(geodetic)))
    np.savez_compressed(os.path.join(OUT, "rough.npz"), **out)
    print("wrote", os.path.join(OUT, "rough.npz"), os.path.getsize(os.path.join(OUT, "rough.npz")), "bytes")


if __name__ == "__main__":
    main()
