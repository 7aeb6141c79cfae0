#!/usr/bin/env python3
"""irregular.npz: traces and lookups over irregular tile stacks, computed by the REAL reference.
Build container only:

    make -C oracle ref && python tests/golden/generate_irregular.py

For each directory of tests/irregular_cases.py ("mixed", "slots255", "slots254", "slots256"),
written as ESRI .asc tiles, the reference (one stack in one layer) runs the harness loop --
turtle_stepper_step until the medium changes, 20 000 steps at most -- on the first 500 rays of the
case, with its default local range (1, keys "<case>_r1_") and with turtle_stepper_range_set(0)
("<case>_r0_", what the GPU library computes): final position, index pair, path length and step
count.  And turtle_stack_elevation and turtle_stack_gradient at about 2 000 points a case: random
ones, and a lattice hugging the seams, the rim and the missing tile.

The inputs (each tile's nodes, the rays, the points) are pinned by their sha256; the positions at
range 0 are too.  tests/test_oracle_golden.py recomputes all of it with the CPU restatement and
checks it bit for bit; tests/test_gpu_irregular.py takes the gradients from here."""
from __future__ import annotations

import os
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_ffi as R  # noqa: E402

import irregular_cases as IC  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))


def main():
    if not R.available():
        sys.exit("oracle/_ref/libturtle_ref.so missing: run `make -C oracle ref`")
    out = {}
    for case in IC.CASES:
        nodes = IC.tile_nodes(case)
        out[f"{case}_nodes_sha"] = np.array(IC.sha(np.concatenate([nodes[k].ravel() for k in sorted(nodes)])))
        tmp = tempfile.mkdtemp(prefix="turtle_irregular_")
        try:
            stack = R.RefStack(IC.write_asc(tmp, case), 0)
            stack.load()
            pos, d = IC.rays(case, IC.GOLDEN_RAYS)
            out[f"{case}_origin_sha"], out[f"{case}_direction_sha"] = np.array(IC.sha(pos)), np.array(IC.sha(d))
            for tag, local_range in (("r1", None), ("r0", 0.0)):
                st = R.RefStepper()
                if local_range is not None:
                    st.range_set(local_range)
                st.add_stack(stack, 0.0)
                t = st.trace(pos, d, max_steps=IC.MAX_STEPS)
                st.destroy()
                assert (t["n_steps"] < IC.MAX_STEPS).all()
                k = f"{case}_{tag}_"
                out.update({k + "index": t["index"].astype(np.int8), k + "length": t["length"],
                            k + "n_steps": t["n_steps"], k + "position_sha": np.array(IC.sha(t["position"]))})
                if tag == "r1":
                    out[k + "position"] = t["position"]
                print(f"{case:8s} {tag}: {t['n_steps'].sum()} steps, max {t['n_steps'].max()}, "
                      f"final media {np.bincount(t['index'][:, 0] + 1)}", flush=True)
            lat, lon = IC.lookup_points(case)
            z, inside = stack.elevation(lat, lon)
            glat, glon, gin = stack.gradient(lat, lon, fill=0.0)
            assert np.array_equal(inside, gin)
            out.update({f"{case}_points_sha": np.array(IC.sha(np.stack([lat, lon]))), f"{case}_z": z,
                        f"{case}_inside": inside.astype(np.int8), f"{case}_glat": glat, f"{case}_glon": glon})
            print(f"{case:8s} lookups: {lat.size} points, {int(inside.sum())} inside", flush=True)
            stack.destroy()
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    np.savez_compressed(os.path.join(OUT, "irregular.npz"), **out)
    print("wrote", os.path.join(OUT, "irregular.npz"), os.path.getsize(os.path.join(OUT, "irregular.npz")), "bytes")


if __name__ == "__main__":
    main()
