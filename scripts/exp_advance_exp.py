"""Experiment: turtle_stepper_advance_exp_n next to turtle_stepper_advance_n.

RAYS rays over the 3601^2 tile, device-resident, budget = inf and no distance limit (every call takes
the same samples).  Three calls, alternated so that all see the same machine, each timed with device
events REPS times after a warm-up (median, least and most):
  advance    advance_n: one density a medium;
  exp_null   advance_exp_n with scale_height = NULL: the same kernel instance, so what the extra
             argument costs on the host;
  exp_air    advance_exp_n with rock uniform and air at 8400 m: the LAW instance.
Twice: on BASELINE's C2 rays (500 m up, -10 .. -1 degrees, ceiling 2000 m: most steps in rock or
near the ground), and on climbing rays in the style of the tests' "ground" batches (from 0.5 m above
the ground, +1 .. +30 degrees, ceiling 30 km: nearly every event takes the law).  In both
arithmetics.  Kernel times: run it under `rocprofv3 --kernel-trace --stats`.

    python scripts/exp_advance_exp.py [out.txt]        (RAYS, REPS: environment)
"""
import ctypes as C
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import turtle_amd as TA  # noqa: E402
from turtle_amd import sharding, synth  # noqa: E402

n = int(os.environ.get("RAYS", "1000000"))
reps = int(os.environ.get("REPS", "9"))
dev = torch.device("cuda", 0)

tmp = tempfile.mkdtemp(prefix="turtle_advance_exp_")
terrain = TA.Map.load(synth.write_hgt(tmp, 45, 3))
st = TA.Stepper()
st.add_map(terrain, 0.0)
stream = torch.cuda.Stream()
torch.cuda.set_stream(stream)
TA.set_stream(stream)

lat, lon, az, el = (torch.as_tensor(v, device=dev) for v in sharding.rank_rays(n, 0, (45., 46.), (3., 4.)))
density = torch.tensor([2650.0, 1.205], device=dev)
scale = torch.tensor([float("inf"), 8400.0], device=dev)
infinite = torch.full((n,), float("inf"), device=dev, dtype=torch.float64)
climb = torch.as_tensor(np.random.default_rng(0xE8BAD7A).uniform(1.0, 30.0, n), device=dev)
batches = {}
pos0, di = st.position(lat, lon, 500.0)
assert bool((di >= 0).all())
batches["c2"] = (pos0, TA.ecef_from_horizontal(lat, lon, az, el), 2000.0)
pos1, di = st.position(lat, lon, 0.5)
batches["climbing"] = (pos1, TA.ecef_from_horizontal(lat, lon, az, climb), 30000.0)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def exp_null(pos, d, ceiling):
    """the C call with scale_height = NULL (the binding's scale_height=None is advance_n itself), with
    the binding's allocations, so that the three calls differ by what they are"""
    index = torch.empty((n, 2), device=dev, dtype=torch.int32)
    depth, distance = (torch.empty(n, device=dev, dtype=torch.float64) for _ in range(2))
    n_steps, status = (torch.empty(n, device=dev, dtype=torch.int32) for _ in range(2))
    p = [C.c_void_p(t.data_ptr()) for t in (pos, d, density, infinite, index, depth, distance, n_steps, status)]
    rc = TA.lib().turtle_stepper_advance_exp_n(st.h, C.c_long(n), p[0], p[1], p[2], None, p[3], None,
                                               C.c_double(ceiling), 1000000, p[4], p[5], p[6], p[7], p[8],
                                               TA.DEVICE)
    assert rc == 0
    return dict(position=pos, index=index, depth=depth, distance=distance, n_steps=n_steps, status=status)


lines = [f"rays {n}, reps {reps}, device-resident, budget inf, no limit, ms a call: median [least .. most]"]
for name, (pos, d, ceiling) in batches.items():
    for math in ("fast", "strict"):
        TA.set_math(math)
        calls = dict(
            advance=lambda: st.advance(pos.clone(), d, density, infinite, None, ceiling),
            exp_null=lambda: exp_null(pos.clone(), d, ceiling),
            exp_air=lambda: st.advance(pos.clone(), d, density, infinite, None, ceiling, scale_height=scale))
        for fn in calls.values():
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in calls}
        for _ in range(reps):
            for k, fn in calls.items():
                ms[k].append(event_ms(fn))
        a, z, e = (fn() for fn in calls.values())
        torch.cuda.synchronize()
        keys = ("position", "index", "distance", "n_steps", "status")
        same_null = all(bool(torch.equal(a[k], z[k])) for k in keys + ("depth",))
        same_path = all(bool(torch.equal(a[k], e[k])) for k in keys)
        in_air = float((e["index"][:, 0] == 1).double().mean())
        med = {k: statistics.median(v) for k, v in ms.items()}
        for k in calls:
            lines.append(f"{name:8s} {math:6s} {k:8s} {med[k]:8.3f} [{min(ms[k]):8.3f} .. {max(ms[k]):8.3f}]")
        lines.append(f"{name:8s} {math:6s} exp_null / advance {med['exp_null'] / med['advance']:.3f}, exp_air / advance "
                     f"{med['exp_air'] / med['advance']:.3f}; exp_null the bits of advance: {same_null}; exp_air the path "
                     f"of advance: {same_path}; steps {int(a['n_steps'].sum())}; rays ending in air {in_air:.3f}; depth "
                     f"exp / uniform, mean {float((e['depth'].sum() / a['depth'].sum())):.4f}")
print("\n".join(lines), flush=True)

if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
