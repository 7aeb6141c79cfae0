"""Experiment: turtle_stepper_crossings_n (lines of sight with every crossing point) next to
turtle_stepper_traverse_n on C2's tile.

The four workloads of DESIGN 3.7 (scripts/exp_traverse.py), 3601^2 tile of BASELINE's C2:
  valley  one detector 0.5 m above the lowest node near the tile's middle, RAYS directions
          (azimuth U[0, 360), elevation U[0, 30] degrees);
  c2      C2's rays (500 m up, -10 .. -1 degrees);
each with a 2000 m ceiling and with none.  For each: ms a call of traverse_n and of crossings_n
at CAPACITY slots (CUDA events, best of REPS after a warm-up, the two calls alternated), the
crossings a ray, and whether the two calls give the same bits.  Kernel times: run it under
`rocprofv3 --kernel-trace --stats`.

    python scripts/exp_crossings.py [out.json]        (RAYS, CAPACITY, REPS: environment)
"""
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import turtle_amd as TA  # noqa: E402
from turtle_amd import sharding, synth  # noqa: E402

n = int(os.environ.get("RAYS", "1000000"))
capacity = int(os.environ.get("CAPACITY", "32"))
reps = int(os.environ.get("REPS", "5"))
dev = torch.device("cuda", 0)

tmp = tempfile.mkdtemp(prefix="turtle_crossings_")
nodes = synth.srtm_like_nodes(45, 3)
terrain = TA.Map.load(synth.write_hgt(tmp, 45, 3))
st = TA.Stepper()
st.add_map(terrain, 0.0)
stream = torch.cuda.Stream()
torch.cuda.set_stream(stream)
TA.set_stream(stream)


def workload(name):
    if name == "valley":
        c = slice(1500, 2100)
        iy, ix = np.unravel_index(np.argmin(nodes[c, c]), nodes[c, c].shape)
        la, lo = 45 + (1500 + iy) / 3600, 3 + (1500 + ix) / 3600
        rng = np.random.default_rng(7)
        lat, lon = np.full(n, la), np.full(n, lo)
        az, el = rng.uniform(0, 360, n), rng.uniform(0, 30, n)
        height = 0.5
    else:
        lat, lon, az, el = sharding.rank_rays(n, 0, (45., 46.), (3., 4.))
        height = 500.0
    t = [torch.as_tensor(v, device=dev) for v in (lat, lon, az, el)]
    pos, di = st.position(t[0], t[1], height)
    assert bool((di >= 0).all())
    return pos, TA.ecef_from_horizontal(*t)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b)


out = {}
for name in ("valley", "c2"):
    pos0, d = workload(name)
    row = {}
    for ceiling in (2000.0, float("inf")):
        key = "ceiling" if ceiling < 1e30 else "no_ceiling"
        # caller-owned inputs, copied each call (as exp_traverse's clone)
        trav = lambda: st.traverse(pos0.clone(), d, ceiling)                        # noqa: E731
        cros = lambda: st.crossings(pos0.clone(), d, ceiling, capacity=capacity)     # noqa: E731
        trav(), cros()
        torch.cuda.synchronize()
        best_t = best_c = 1e30
        for _ in range(reps):   # alternated, so that both see the same machine
            best_t = min(best_t, event_ms(trav))
            best_c = min(best_c, event_ms(cros))
        t, c = trav(), cros()
        torch.cuda.synchronize()
        same = all(bool(torch.equal(t[k], c[k])) for k in ("position", "index", "length", "n_steps",
                                                            "n_crossings"))
        res = dict(traverse_ms=best_t, crossings_ms=best_c, ratio=best_c / best_t,
                   crossings_mean=float(c["n_crossings"].double().mean()),
                   crossings_max=int(c["n_crossings"].max()),
                   over_capacity=int((c["n_crossings"] > capacity).sum()), same_bits=same)
        row[key] = res
        print(name, key, json.dumps(res), flush=True)
    out[name] = row

path = sys.argv[1] if len(sys.argv) > 1 else None
if path:
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(dict(rays=n, capacity=capacity, math=TA.get_math(), workloads=out), f, indent=1)
