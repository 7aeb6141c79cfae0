#!/usr/bin/env python3
"""vs_reference.npz: whole batches stepped by the REAL reference, for
tests/test_oracle_vs_reference.py.  Build container only:

    make -C oracle ref && python tests/golden/generate_vs_reference.py

Two recipes, both over synthetic 1201^2 tiles regenerated from turtle_amd/synth.py at test time
(SHA-256 of their nodes stored):

  trace_*   6000 rays through one map (N45E003), each to its first boundary, with the exact
            transform (range 0) and with the reference's local approximation (range 1); the first
            64 again under a cap of 9 steps, and 4 that start outside the map.
  walk_*    6000 scattering walks of 48 steps (a Philox direction a step, tests/philox_ref.py) from
            20 km up over a stack of two tiles that touches longitude 0: through a stack without
            lock / unlock, and through a LOCKED stack on one thread (the client memo quirk).

The fixture holds the ray origins and directions the oracle computed for them (walk directions:
their SHA-256) and the reference's medium index, step count, path length and end position."""
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

from oracle import ffi as O  # noqa: E402
from oracle import ref_ffi as R  # noqa: E402
from turtle_amd import synth  # noqa: E402

import philox_ref as P  # noqa: E402
import terrains as T  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
N_NODES = 1201
WALK_TILES = [(45, 0), (45, 1)]
N_RAYS, WALK_STEPS = 6000, 48


def trace_inputs():
    """the rays of the trace recipe, positioned by the oracle"""
    _, geo = T.hgt_oracle(45, 3, N_NODES)
    lat, lon, az, el = synth.uniform_rays(N_RAYS, (45.0, 46.0), (3.0, 4.0), seed=21)
    pos, _ = geo.position(lat, lon, 500.0)
    return geo, pos, O.ecef_from_horizontal(lat, lon, az, el)


def walk_inputs():
    """the origins and per-step directions of the walk recipe"""
    geo = T.mosaic_oracle(WALK_TILES, N_NODES, 45, 0, 1, 2)
    lat, lon, _, _ = synth.uniform_rays(N_RAYS, (45.0, 46.0), (0.0, 2.0), seed=5)
    pos, _ = geo.position(lat, lon, np.full(N_RAYS, 20000.0))
    dirs = np.stack([P.isotropic(N_RAYS, 7, k) for k in range(WALK_STEPS)])
    return geo, pos, dirs


def main():
    if not R.driver_available():
        sys.exit("oracle/_ref/libturtle_ref_driver.so missing: run `make -C oracle ref`")
    tmp = tempfile.mkdtemp(prefix="turtle_vs_reference_")
    out = {}
    try:
        path = synth.write_hgt(tmp, 45, 3, N_NODES)
        _, pos, d = trace_inputs()
        out.update(trace_position=pos, trace_direction=d,
                   trace_nodes_sha=np.array(T.sha(synth.srtm_like_nodes(45, 3, N_NODES))))
        far = pos[:4] * 3.0
        for rng in (0, 1):
            t = R.trace_map(path, pos, d, local_range=float(rng), threads=4)
            cap = R.trace_map(path, pos[:64], d[:64], local_range=float(rng), max_steps=9)
            out.update({f"trace{rng}_index": t["index"], f"trace{rng}_n_steps": t["n_steps"],
                        f"trace{rng}_length": t["length"], f"trace{rng}_end": t["position"],
                        f"trace{rng}_total_steps": np.array(t["total_steps"]),
                        f"trace{rng}_cap9_n_steps": cap["n_steps"]})
        out["trace_far_index"] = R.trace_map(path, far, d[:4])["index"]

        tiles = os.path.join(tmp, "tiles")
        for la, lo in WALK_TILES:
            synth.write_hgt(tiles, la, lo, N_NODES)
        _, pos, dirs = walk_inputs()
        out.update(walk_position=pos, walk_directions_sha=np.array(T.sha(dirs)),
                   walk_nodes_sha=np.array([T.sha(synth.srtm_like_nodes(la, lo, N_NODES))
                                            for la, lo in WALK_TILES]))
        free = R.stack_run(tiles, pos, dirs, walk_steps=WALK_STEPS, local_range=0.0, locked=False)
        locked = R.stack_run(tiles, pos, dirs, walk_steps=WALK_STEPS, local_range=0.0, threads=1,
                             locked=True)
        for tag, w in (("free", free), ("locked", locked)):
            out.update({f"walk_{tag}_index": w["index"], f"walk_{tag}_n_steps": w["n_steps"],
                        f"walk_{tag}_length": w["length"]})
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    dest = os.path.join(OUT, "vs_reference.npz")
    np.savez_compressed(dest, **out)
    print(f"vs_reference.npz: {os.path.getsize(dest) / 1024:.1f} KiB; trace steps",
          int(out["trace0_total_steps"]), int(out["trace1_total_steps"]),
          "; walks that left the mosaic", int((free["n_steps"] < WALK_STEPS).sum()),
          "; locked walks that differ", int((locked["length"] != free["length"]).sum()))


if __name__ == "__main__":
    main()
