"""Helper of test_gpu_cross_tail.py: traces the named batches through one map and through a
one-tile stack and stores every output array and the device's totals.  Run as a child process,
because the library reads TURTLE_AMD_CROSS_TAIL (and the other knobs) once."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import turtle_amd as TA                      # noqa: E402
from turtle_amd import synth                 # noqa: E402

SHALLOW = dict(el_range=(-3.0, -0.2), height=300.0, max_steps=100000)   # creep_probe.py's recipe: long rays
# name -> rays, recipe
CASES = {
    "probe": (40000, SHALLOW),
    "n1": (1, SHALLOW), "n63": (63, SHALLOW), "n64": (64, SHALLOW), "n65": (65, SHALLOW),
    "n4097": (4097, SHALLOW),
    # straight down at the ground: every ray ends within phase A's closed-form steps
    "steep": (20000, dict(el_range=(-60.0, -60.0), height=300.0, max_steps=100000)),
    # climbing away from ground 20 m below, stopped at 40 steps (past the hand-over at step 32):
    # every ray reaches the lined pass and none of them ever crosses
    "capped": (20000, dict(el_range=(8.0, 10.0), height=20.0, max_steps=40)),
}


def main(out_path, workdir, names):
    n_nodes = 1201
    path = synth.write_hgt(os.path.join(workdir, "map"), 45, 3, n_nodes)
    synth.write_hgt(os.path.join(workdir, "stack"), 45, 3, n_nodes)
    out = {}
    for tag in ("map", "stack"):
        st = TA.Stepper()
        if tag == "map":
            terrain = TA.Map.load(path)
            st.add_map(terrain, 0.0)
        else:
            terrain = TA.Stack(os.path.join(workdir, "stack"), 0)
            st.add_stack(terrain, 0.0)
        for name in names:
            n, recipe = CASES[name]
            lat, lon, az, el = synth.uniform_rays(n, (45.0, 46.0), (3.0, 4.0), seed=123,
                                                  el_range=recipe["el_range"])
            pos, _ = st.position(lat, lon, recipe["height"])
            d = TA.ecef_from_horizontal(lat, lon, az, el)
            t = st.trace(pos.copy(), d, max_steps=recipe["max_steps"])
            for k in ("position", "index", "length", "n_steps"):
                out[f"{name}_{tag}_{k}"] = np.asarray(t[k])
            s = st.trace_stats()
            out[f"{name}_{tag}_stats"] = np.array([s["rays"], s["steps"], s["samples"], s["capped"]],
                                                  dtype=np.uint64)
        st.destroy()
        terrain.destroy()
    np.savez(out_path, **out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2], sys.argv[3].split(","))
