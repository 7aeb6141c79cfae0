"""Helper of test_gpu_first_pass.py: traces mixed batches through one map and through a 2 x 2
regular stack, each a second time from where the first call left the rays
(TURTLE_AMD_TRACE_RESUME), and stores every output array and the device's totals.  Run as a child
process, because the library reads TURTLE_AMD_FIRST_PASS (and the other knobs) once."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import turtle_amd as TA                      # noqa: E402
from turtle_amd import synth                 # noqa: E402

SIZES = (1, 63, 65, 257, 4099)
# beyond the hand-over at step 32: no cap in reach, a cap in the lined pass, the cap just past the
# hand-over; at and below it: the closed-form pass alone (the persistent kernel, whatever the knob)
MAX_STEPS = (100000, 40, 33, 32, 20)
KINDS = ("c2", "steep", "outside", "rim", "shallow")
ARRAYS = ("position", "index", "length", "n_steps")
LAT, LON = (45.0, 46.0), (3.0, 4.0)   # the map; the stack's south-west tile


def kind_of(n):
    """which recipe ray i of a batch of n follows"""
    return np.arange(n) % len(KINDS)


def batch(st, n, seed):
    """n rays, the five kinds in turn: (a) the headline's recipe (-10 .. -1 degrees from 500 m);
    (b) steep ones from 300 m, which cross before step 32; (c) origins outside the data; (d) rays
    that start within a few hundred metres of the south or the west rim and head out; (e) shallow
    ones (-3 .. -0.2 degrees from 300 m), which take thousands of steps."""
    kind = kind_of(n)
    lat, lon, az, el = synth.uniform_rays(n, LAT, LON, seed=seed)
    u = np.random.Generator(np.random.Philox(seed + 1)).random((4, n))
    height = np.full(n, 500.0)
    b = kind == 1
    el[b], height[b] = -90.0 + 30.0 * u[0][b], 300.0
    e = kind == 4
    el[e], height[e] = -3.0 + 2.8 * u[0][e], 300.0
    d_ = kind == 3
    south = d_ & (u[1] < 0.5)
    west = d_ & ~south
    lat[south] = LAT[0] + 0.0005 + 0.0025 * u[2][south]
    az[south] = 150.0 + 60.0 * u[3][south]
    lon[west] = LON[0] + 0.0007 + 0.0033 * u[2][west]
    az[west] = 240.0 + 60.0 * u[3][west]
    c = kind == 2
    lat[c] = LAT[0] - 0.05 - 0.2 * u[2][c]
    # (position_n wants ground below the point: the rays outside get theirs from the ellipsoid)
    lat_in, lon_in = np.where(c, 45.5, lat), np.where(c, 3.5, lon)
    pos, _ = st.position(lat_in, lon_in, height)
    pos = np.array(pos)
    if c.any():
        pos[c] = np.asarray(TA.ecef_from_geodetic(lat[c], lon[c], np.full(int(c.sum()), 1000.0)))
    d = np.asarray(TA.ecef_from_horizontal(lat, lon, az, el))
    return pos, d


def stats_of(st):
    s = st.trace_stats()
    return np.array([s["rays"], s["steps"], s["samples"], s["capped"]], dtype=np.uint64)


def main(out_path, workdir):
    n_nodes = 1201
    path = synth.write_hgt(os.path.join(workdir, "map"), 45, 3, n_nodes)
    for la in (45, 46):
        for lo in (3, 4):
            synth.write_hgt(os.path.join(workdir, "stack"), la, lo, n_nodes)
    out = {}
    for tag in ("map", "stack"):
        st = TA.Stepper()
        if tag == "map":
            terrain = TA.Map.load(path)
            st.add_map(terrain, 0.0)
        else:
            terrain = TA.Stack(os.path.join(workdir, "stack"), 0)
            terrain.load()   # every tile resident: no paging rounds
            st.add_stack(terrain, 0.0)
        for n in SIZES:
            pos, d = batch(st, n, seed=1000 + n)
            for ms in MAX_STEPS:
                key = f"{tag}_n{n}_m{ms}"
                t = st.trace(pos.copy(), d, max_steps=ms)
                for k in ARRAYS:
                    out[f"{key}_{k}"] = np.array(t[k])
                out[f"{key}_stats"] = stats_of(st)
                r = st.trace(out[f"{key}_position"].copy(), d, max_steps=ms,
                             resume_index=out[f"{key}_index"])
                for k in ARRAYS:
                    out[f"{key}_resumed_{k}"] = np.array(r[k])
                out[f"{key}_resumed_stats"] = stats_of(st)
        st.destroy()
        terrain.destroy()
    np.savez(out_path, **out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
