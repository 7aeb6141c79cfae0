"""Experiment: turtle_stepper_normal_n on C2's tile, next to the composition of batch calls that
gave a normal before it existed.

POINTS points, DEVICE space, CUDA events, best of REPS after a warm-up:
  one_stack   the 3601^2 tile of BASELINE's C2 as a stack of one tile, every point in layer 0 (the
              one-stack kernel): normal_n, alternated with turtle_ecef_to_geodetic_n (STRICT) +
              turtle_stack_elevation_n + turtle_stack_gradient_n + the tangent arithmetic in torch,
              and the largest component by which the two differ;
  layers      a flat at 0, that stack, a flat at 3000 m, the points' layers drawn from 0 .. 2 (the
              generic kernel): normal_n.
Algorithmic bytes a point: 24 + 4 in, 24 + 4 out, and 16 of nodes (a cell's four and up to four
neighbours, 16 bits each) where a grid answers.  Kernel times: run it under
`rocprofv3 --kernel-trace --stats`.

    python scripts/exp_normal.py [out.json]        (POINTS, REPS: environment)
"""
import json
import math
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import turtle_amd as TA  # noqa: E402
from turtle_amd import synth  # noqa: E402

n = int(os.environ.get("POINTS", "1000000"))
reps = int(os.environ.get("REPS", "5"))
dev = torch.device("cuda", 0)
A, E = 6378137.0, 0.081819190842622

tmp = tempfile.mkdtemp(prefix="turtle_normal_")
synth.write_hgt(tmp, 45, 3)
stack = TA.Stack(tmp, 0)
stack.load()
one = TA.Stepper()
one.add_stack(stack, 0.0)
three = TA.Stepper()
for add in (lambda: three.add_flat(0.0), lambda: three.add_stack(stack, 0.0), lambda: three.add_flat(3000.0)):
    three.add_layer()
    add()
stream = torch.cuda.Stream()
torch.cuda.set_stream(stream)
TA.set_stream(stream)

rng = np.random.default_rng(11)
lat = torch.as_tensor(rng.uniform(45.02, 45.98, n), device=dev)
lon = torch.as_tensor(rng.uniform(3.02, 3.98, n), device=dev)
pos = TA.ecef_from_geodetic(lat, lon, torch.as_tensor(rng.uniform(0.0, 3000.0, n), device=dev))
zeros = torch.zeros(n, dtype=torch.int32, device=dev)
layers = torch.as_tensor(rng.integers(0, 3, n).astype(np.int32), device=dev)
out = torch.zeros((n, 3), dtype=torch.float64, device=dev)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def composed():
    """the normal of the one-stack geometry from the calls the library had before normal_n"""
    la, lo, _ = TA.ecef_to_geodetic(pos)
    z, _ = stack.elevation(la, lo)
    glat, glon, _ = stack.gradient(la, lo)
    lam, phi = lo * (math.pi / 180.0), la * (math.pi / 180.0)
    sl, cl, sp, cp = torch.sin(lam), torch.cos(lam), torch.sin(phi), torch.cos(phi)
    g = 1.0 - E * E * sp * sp
    rn = A / torch.sqrt(g)
    rm = rn * (1.0 - E * E) / g
    a = glon / ((rn + z) * cp * (math.pi / 180.0))
    b = glat / ((rm + z) * (math.pi / 180.0))
    w = torch.stack([cl * cp + a * sl + b * cl * sp, sl * cp - a * cl + b * sl * sp, sp - b * cp], 1)
    return w / torch.linalg.norm(w, dim=1, keepdim=True)


TA.set_math("strict")   # (the composition's transform: normal_n's own is strict whatever this says)
call_one = lambda: one.normal(pos, zeros, out=out)          # noqa: E731
call_three = lambda: three.normal(pos, layers, out=out)     # noqa: E731
call_one(), composed(), call_three()
torch.cuda.synchronize()
best = dict(one_stack=1e30, composed=1e30, layers=1e30)
for _ in range(reps):   # alternated, so that all see the same machine
    best["one_stack"] = min(best["one_stack"], event_ms(call_one))
    best["composed"] = min(best["composed"], event_ms(composed))
    best["layers"] = min(best["layers"], event_ms(call_three))
normal, data_index = call_one()
worst = float((normal - composed()).abs().max())
answered = float((data_index >= 0).double().mean())
_, di3 = call_three()
grid3 = float(((layers == 1) & (di3 >= 0)).double().mean())
torch.cuda.synchronize()
res = dict(points=n, one_stack_ms=best["one_stack"], composed_ms=best["composed"], layers_ms=best["layers"],
           one_stack_gbs=n * (56 + 16 * answered) / best["one_stack"] / 1e6,
           layers_gbs=n * (56 + 16 * grid3) / best["layers"] / 1e6,
           composed_over_one_stack=best["composed"] / best["one_stack"], worst_component_difference=worst)
print(json.dumps(res), flush=True)
path = sys.argv[1] if len(sys.argv) > 1 else None
if path:
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
