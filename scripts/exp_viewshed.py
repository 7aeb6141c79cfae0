"""Experiment: turtle_stepper_viewshed_n on C2's tile, next to the composition of batch calls that
gave a viewshed before it existed, and next to turtle_stepper_horizon_n on the same lines.

The workload of scripts/exp_horizon.py: the 3601^2 tile of BASELINE's C2 as a stack of one tile;
OBSERVERS (256) x AZIMUTHS (360) lines of DISTANCES (1024) samples, 200 m to 100 km in a geometric
progression; DEVICE space, events on the library's stream, a warm-up, the best of REPS alternated
runs:
  fused      viewshed_n (target height 0, every output) in FAST and in STRICT arithmetic;
  flags      viewshed_n with `visible` alone (FAST): one byte a sample stored instead of 17;
  horizon    horizon_n on the same inputs, FAST and STRICT: the same samples evaluated, the final
             maximum of a line kept.  fused - horizon is what the scan and the per-sample stores add;
  composed   the same answer from the calls the library had before: turtle_ecef_to_geodetic_n
             (STRICT) of the observers, turtle_ecef_from_horizontal_n, the sample points and
             turtle_ecef_to_geodetic_n of them, turtle_stepper_position_n at height 0, the frame,
             the dot product and cummax in torch -- CHUNK observers at a time, as memory needs.
It reports ns a sample, the ratios, and how the fused STRICT answer compares with the composed one.

    python scripts/exp_viewshed.py [out.json]    (OBSERVERS, AZIMUTHS, DISTANCES, CHUNK, REPS: environment)
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

tmp = tempfile.mkdtemp(prefix="turtle_viewshed_")
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


def fused(math_, want=("sine", "horizon", "n_visible")):
    TA.set_math(math_)
    return st.viewshed(pos, azimuth, distance, 0, want=want)


def skyline(math_):
    TA.set_math(math_)
    return st.horizon(pos, azimuth, distance, 0, out=out)


def composed():
    """visible, sine and horizon from the calls the library had before viewshed_n"""
    TA.set_math("strict")
    flags, sines, horizons = [], [], []
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
        data = (di.reshape(m, n_az, n_d) >= 0) & (rr > 1.1920928955078125e-07)
        filled = torch.where(data, sine, -math.inf)
        inclusive = filled.cummax(-1).values
        horizon = torch.cat([torch.full_like(inclusive[..., :1], -math.inf), inclusive[..., :-1]], -1)
        flags.append(torch.where(data, (filled >= horizon).to(torch.int8), -1))
        sines.append(filled)
        horizons.append(horizon)
    return torch.cat(flags), torch.cat(sines), torch.cat(horizons)


fused("fast"), fused("strict"), fused("fast", ()), skyline("fast"), skyline("strict"), composed()
torch.cuda.synchronize()
arms = dict(fast=lambda: fused("fast"), strict=lambda: fused("strict"), flags_only_fast=lambda: fused("fast", ()),
            horizon_fast=lambda: skyline("fast"), horizon_strict=lambda: skyline("strict"), composed=composed)
best = {name: 1e30 for name in arms}
for _ in range(reps):   # alternated, so that all see the same machine
    for name, arm in arms.items():
        best[name] = min(best[name], event_ms(arm))
got = fused("strict")
flags, sine, horizon = composed()
TA.set_math("fast")
data = flags >= 0
same_data = bool(((got["visible"] >= 0) == data).all())
worst = float((got["sine"] - sine)[data].abs().max())
samples = n * n_az * n_d
res = dict(observers=n, azimuths=n_az, distances=n_d, samples=samples, library=os.path.relpath(TA.library_path(), ROOT))
for name, ms in best.items():
    res[name + "_ms"] = ms
    res[name + "_ns_per_sample"] = ms * 1e6 / samples
res.update(composed_over_fast=best["composed"] / best["fast"], composed_over_strict=best["composed"] / best["strict"],
           fast_over_horizon_fast=best["fast"] / best["horizon_fast"],
           strict_over_horizon_strict=best["strict"] / best["horizon_strict"],
           samples_with_data=float(data.double().mean()), visible_of_those=float((flags == 1).sum() / data.sum()),
           same_samples_with_data=same_data, flags_that_differ=int((got["visible"] != flags).sum()),
           worst_sine_difference=worst)
print(json.dumps(res), flush=True)
path = sys.argv[1] if len(sys.argv) > 1 else None
if path:
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
