"""Experiment: turtle_stepper_horizon_n on C2's tile, next to the composition of batch calls that
gave a skyline before it existed.

The 3601^2 tile of BASELINE's C2 as a stack of one tile; OBSERVERS (256) x AZIMUTHS (360) lines of
DISTANCES (1024) samples, 200 m to 100 km in a geometric progression; DEVICE space, events on the
library's stream, a warm-up, the best of REPS alternated runs:
  fused      horizon_n in FAST and in STRICT arithmetic;
  composed   the same answer from the calls the library had before: turtle_ecef_to_geodetic_n
             (STRICT) of the observers, turtle_ecef_from_horizontal_n, the sample points and
             turtle_ecef_to_geodetic_n of them, turtle_stepper_position_n at height 0, the frame,
             the dot product and the maximum in torch -- CHUNK observers at a time, as memory needs.
It reports ns a sample, composed / fused and the largest difference in the sine of the elevation
between the two.  The composition moves on the order of 100 bytes a sample through HBM (24 of
sample point, 24 of geodetic coordinates, 8 of height, 28 of ground point and data index, 8 + 8 of
squared range and sine, read back by the next call each), the fused kernel none: its traffic is the
16-bit nodes under a sample.  Kernel times: run it under `rocprofv3 --kernel-trace --stats`.

    python scripts/exp_horizon.py [out.json]     (OBSERVERS, AZIMUTHS, DISTANCES, CHUNK, REPS: environment)
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

n = int(os.environ.get("OBSERVERS", "256"))
n_az = int(os.environ.get("AZIMUTHS", "360"))
n_d = int(os.environ.get("DISTANCES", "1024"))
chunk = int(os.environ.get("CHUNK", "16"))
reps = int(os.environ.get("REPS", "3"))
dev = torch.device("cuda", 0)

tmp = tempfile.mkdtemp(prefix="turtle_horizon_")
synth.write_hgt(tmp, 45, 3)
stack = TA.Stack(tmp, 0)
stack.load()
st = TA.Stepper()
st.add_stack(stack, 0.0)
stream = torch.cuda.Stream()
torch.cuda.set_stream(stream)
TA.set_stream(stream)

rng = np.random.default_rng(12)
pos, _ = st.position(torch.as_tensor(rng.uniform(45.2, 45.8, n), device=dev),
                     torch.as_tensor(rng.uniform(3.2, 3.8, n), device=dev),
                     torch.as_tensor(rng.uniform(2.0, 300.0, n), device=dev))
azimuth = torch.arange(n_az, dtype=torch.float64, device=dev) * (360.0 / n_az)
distance = torch.as_tensor(200.0 * 500.0 ** (np.arange(n_d) / (n_d - 1.0)), device=dev)
out = dict(elevation=torch.zeros((n, n_az), dtype=torch.float64, device=dev),
           range=torch.zeros((n, n_az), dtype=torch.float64, device=dev))


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def fused(math_):
    TA.set_math(math_)
    return st.horizon(pos, azimuth, distance, 0, out=out)


def composed():
    """the sine of the skyline, and its sample, from the calls the library had before horizon_n"""
    TA.set_math("strict")
    best, best_k = [], []
    for r0 in range(0, n, chunk):
        p = pos[r0:r0 + chunk]
        m = p.shape[0]
        la0, lo0, _ = TA.ecef_to_geodetic(p)
        h = TA.ecef_from_horizontal(la0.repeat_interleave(n_az), lo0.repeat_interleave(n_az), azimuth.repeat(m),
                                    torch.zeros(m * n_az, dtype=torch.float64, device=dev)).reshape(m, n_az, 1, 3)
        q = p.reshape(m, 1, 1, 3) + distance.reshape(1, 1, n_d, 1) * h
        la, lo, _ = TA.ecef_to_geodetic(q.reshape(-1, 3))
        ground, di = st.position(la, lo, 0.0, 0)
        d = ground.reshape(m, n_az, n_d, 3) - p.reshape(m, 1, 1, 3)
        lam, phi = lo0 * (math.pi / 180.0), la0 * (math.pi / 180.0)
        up = torch.stack([torch.cos(lam) * torch.cos(phi), torch.sin(lam) * torch.cos(phi), torch.sin(phi)], 1)
        rr = (d * d).sum(-1)
        sine = (d * up.reshape(m, 1, 1, 3)).sum(-1) / torch.sqrt(rr)
        sine = torch.where((di.reshape(m, n_az, n_d) >= 0) & (rr > 1.1920928955078125e-07), sine, -math.inf)
        value, k = sine.max(-1)
        best.append(value)
        best_k.append(k + 1)
    return torch.cat(best), torch.cat(best_k)


fused("fast"), fused("strict"), composed()
torch.cuda.synchronize()
best = dict(fast=1e30, strict=1e30, composed=1e30)
for _ in range(reps):   # alternated, so that all see the same machine
    best["fast"] = min(best["fast"], event_ms(lambda: fused("fast")))
    best["strict"] = min(best["strict"], event_ms(lambda: fused("strict")))
    best["composed"] = min(best["composed"], event_ms(composed))
got = fused("strict")
sine, k = composed()
TA.set_math("fast")
found = got["sample"] > 0
worst = float((torch.sin(got["elevation"] * (math.pi / 180.0)) - sine)[found].abs().max())
samples = n * n_az * n_d
res = dict(observers=n, azimuths=n_az, distances=n_d, samples=samples, library=os.path.relpath(TA.library_path(), ROOT),
           fast_ms=best["fast"], strict_ms=best["strict"], composed_ms=best["composed"],
           fast_ns_per_sample=best["fast"] * 1e6 / samples, strict_ns_per_sample=best["strict"] * 1e6 / samples,
           composed_ns_per_sample=best["composed"] * 1e6 / samples,
           composed_over_fast=best["composed"] / best["fast"], composed_over_strict=best["composed"] / best["strict"],
           lines_with_a_sample=float(found.double().mean()),
           lines_on_another_sample=int((got["sample"] != k)[found].sum()), worst_sine_difference=worst)
print(json.dumps(res), flush=True)
path = sys.argv[1] if len(sys.argv) > 1 else None
if path:
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
