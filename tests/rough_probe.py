"""Helper of test_gpu_rough.test_optional_machinery_gives_the_same_bits: traces n rays over the rough
tile, the void tile and the 2 x 2 stack of tests/rough_cases.py (paged, one tile resident) and
stores the results.  Run as a child process, because the library reads its switches once."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import turtle_amd as TA                      # noqa: E402

import rough_cases as RC                     # noqa: E402


def draws(n, box):
    """half C2's recipe, half the ground recipe"""
    h = n // 2
    a = RC.ray_draws("c2", h, box)
    b = RC.ray_draws("ground", n - h, box)
    return [np.concatenate([u, v]) for u, v in zip(a, b)]


def trace(out, tag, st, box, n):
    lat, lon, h, az, el = draws(n, box)
    pos, di = st.position(lat, lon, h)
    keep = di >= 0          # (not in the stack's missing tile)
    pos = np.ascontiguousarray(pos[keep])
    d = np.ascontiguousarray(TA.ecef_from_horizontal(lat, lon, az, el)[keep])
    t = st.trace(pos.copy(), d, max_steps=1000000)
    for k in ("position", "index", "length", "n_steps"):
        out[f"{tag}_{k}"] = np.asarray(t[k])
    return pos, d


def main(out_path, workdir, n):
    """the tiles at the default arithmetic (FAST); the stack in STRICT and in FAST"""
    out = {}
    for tag in ("rough", "void"):
        st = TA.Stepper()
        terrain = TA.Map.load(RC.write_tile(os.path.join(workdir, tag), tag))
        st.add_map(terrain, 0.0)
        trace(out, tag, st, ((RC.LAT0, RC.LAT0 + 1), (RC.LON0, RC.LON0 + 1)), n)
        st.destroy()
        terrain.destroy()
    path = RC.write_stack(os.path.join(workdir, "stack"))
    for math in ("strict", "fast"):
        TA.set_math(math)
        st = TA.Stepper()
        terrain = TA.Stack(path, 1)
        st.add_stack(terrain, 0.0)
        out["stack_origin"], out["stack_direction"] = trace(out, "stack_" + math, st, RC.STACK_BOX, n)
        out[f"stack_{math}_rounds"] = np.array(st.rounds)
        st.destroy()
        terrain.destroy()
    TA.set_math("fast")
    np.savez(out_path, **out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2], int(sys.argv[3]))
