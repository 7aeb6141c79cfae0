#!/usr/bin/env python3
"""composite.npz: traces, lines of sight and lookups over composite geometries, computed by the
REAL reference.  Build container only:

    make -C oracle ref && python tests/golden/generate_composite.py

For each case of tests/composite_cases.py ("example", "layers", "overlap", "offsets") the reference
runs
  * the harness loop -- turtle_stepper_step until the medium changes -- on the first 500 rays of
    "graze", with its default local range (1, keys "<case>_r1_") and with
    turtle_stepper_range_set(0) ("<case>_r0_", what the GPU library computes): final position,
    index pair, path length and step count;
  * the loop of generate_traverse.py (every medium up to a ceiling of 5000 m, 20 000 steps at
    most, range 0) on the first 500 lines of "sight" ("<case>_sight_"): index pair, length per
    medium, step and crossing counts;
  * at about 900 points 1e-12 .. 1e-4 degree either side of every rim line of the case's data
    ("<case>_rim_"): turtle_stepper_position 100 m above every layer below the lid (position, data
    index) and one turtle_stepper_step without a direction from 2500 m above the ellipsoid
    (latitude, longitude, altitude, elevation pair, index pair).

The inputs (node arrays, rays, points) are pinned by their sha256.  tests/test_oracle_golden.py
recomputes all of it with the CPU restatement and checks it bit for bit;
tests/test_gpu_composite.py compares the kernels with both."""
from __future__ import annotations

import os
import shutil
import sys
import tempfile

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, OUT)

from oracle import ref_ffi as R  # noqa: E402

import composite_cases as CC  # noqa: E402
import generate_traverse as GT  # noqa: E402

RIM_HEIGHT, POSITION_HEIGHT = 2500.0, 100.0


def rim_records(st, case):
    lat, lon, _ = CC.rim_points(case)
    out = {"points_sha": np.array(CC.sha(np.stack([lat, lon])))}
    for layer in range(len(CC.RECIPES[case][1]) - 1):
        pos, di = np.zeros((lat.size, 3)), np.zeros(lat.size, dtype=np.int8)
        for k in range(lat.size):
            rc, pos[k], di[k] = st.position(lat[k], lon[k], POSITION_HEIGHT, layer)
            assert rc == 0, R.errors()
        out[f"position{layer}"], out[f"data{layer}"] = pos, di
    start = R.ecef_from_geodetic(lat, lon, np.full(lat.size, RIM_HEIGHT))
    rows = np.zeros((lat.size, 7))
    for k in range(lat.size):
        o = st.step(start[k], None)
        assert o["rc"] == 0, R.errors()
        rows[k] = (o["latitude"], o["longitude"], o["altitude"], o["elevation"][0], o["elevation"][1],
                   o["index"][0], o["index"][1])
    out["start_sha"], out["step"] = np.array(CC.sha(start)), rows
    return out


def main():
    if not R.available():
        sys.exit("oracle/_ref/libturtle_ref.so missing: run `make -C oracle ref`")
    GT.MAX_STEPS = CC.SIGHT_MAX_STEPS
    out = {}
    for case in CC.CASES:
        out[f"{case}_nodes_sha"] = np.array(CC.nodes_sha(case))
        tmp = tempfile.mkdtemp(prefix="turtle_composite_")
        try:
            pos, d, _ = CC.graze(case, n=CC.GOLDEN_RAYS)
            out[f"{case}_graze_origin_sha"], out[f"{case}_graze_direction_sha"] = np.array(CC.sha(pos)), np.array(CC.sha(d))
            for tag, local_range in (("r1", None), ("r0", 0.0)):
                geo = CC.reference_geometry(case, os.path.join(tmp, tag), local_range)
                t = geo["stepper"].trace(pos, d, max_steps=CC.GRAZE_MAX_STEPS)
                assert (t["n_steps"] < CC.GRAZE_MAX_STEPS).all()
                k = f"{case}_{tag}_"
                out.update({k + "index": t["index"].astype(np.int8), k + "length": t["length"],
                            k + "n_steps": t["n_steps"], k + "position": t["position"]})
                print(f"{case:8s} {tag}: {t['n_steps'].sum()} steps, max {t['n_steps'].max()}, "
                      f"final media {np.bincount(t['index'][:, 0] + 1)}", flush=True)
                if tag == "r0":
                    spos, sd = CC.sight(case, CC.GOLDEN_RAYS)
                    media = len(CC.RECIPES[case][1]) + 1
                    index, length, n_steps, n_cross = GT.loop(geo["stepper"], spos, sd, CC.CEILING, media)
                    k = f"{case}_sight_"
                    out.update({k + "origin_sha": np.array(CC.sha(spos)), k + "direction_sha": np.array(CC.sha(sd)),
                                k + "index": index.astype(np.int8), k + "length": length, k + "n_steps": n_steps,
                                k + "n_crossings": n_cross})
                    print(f"{case:8s} sight: {int(n_steps.sum())} steps, crossings max {n_cross.max()}, "
                          f"{int((n_steps >= CC.SIGHT_MAX_STEPS).sum())} capped", flush=True)
                    geo["stepper"].reset()
                    out.update({f"{case}_rim_{name}": v for name, v in rim_records(geo["stepper"], case).items()})
                CC.destroy(geo)
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    path = os.path.join(OUT, "composite.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
