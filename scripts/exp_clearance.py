"""Experiment: turtle_stepper_clearance_n on the rough tile, next to the composition of batch calls
that could give the same matrix before it existed, and next to turtle_stepper_horizon_n over the
same number of samples.

The rough tile of the tests (synth.write_rough_hgt, 1201^2 nodes) as a stack of one tile;
OBSERVERS (256) a few metres to 300 m above the ground x TARGETS (256) in the air, some beyond the
tile's rims, x FRACTIONS (1024) interior fractions; DEVICE space, events on the library's stream, a
warm-up, the best of REPS alternated runs:
  fused      clearance_n (every output) in FAST and in STRICT arithmetic;
  horizon    horizon_n over OBSERVERS x TARGETS azimuths x FRACTIONS distances (100 m to 15 km,
             which stay on the tile from every observer), FAST and STRICT: as many samples, about
             the same work each (a transform, the layer's top, a point from geodetic coordinates,
             a dot product), the same reduction;
  composed   the same matrix from the calls the library had before: every sample point built in
             torch, turtle_ecef_to_geodetic_n (STRICT) of them, turtle_stepper_position_n at
             height 0, the verticals, the dot product and min in torch -- CHUNK observers at a
             time, as memory needs.
It reports ns a sample, the ratios, and how the fused STRICT answer compares with the composed one.

    python scripts/exp_clearance.py [out.json]    (OBSERVERS, TARGETS, FRACTIONS, CHUNK, REPS: environment)
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
m = int(os.environ.get("TARGETS", "256"))
n_f = int(os.environ.get("FRACTIONS", "1024"))
chunk = int(os.environ.get("CHUNK", "16"))
reps = int(os.environ.get("REPS", "3"))
dev = torch.device("cuda", 0)

tmp = tempfile.mkdtemp(prefix="turtle_clearance_")
synth.write_rough_hgt(tmp, 45, 3)
stack = TA.Stack(tmp, 0)
stack.load()
st = TA.Stepper()
st.add_stack(stack, 0.0)
stream = torch.cuda.Stream()
torch.cuda.set_stream(stream)
TA.set_stream(stream)

rng = np.random.default_rng(12)
obs, _ = st.position(torch.as_tensor(rng.uniform(45.2, 45.8, n), device=dev),
                     torch.as_tensor(rng.uniform(3.2, 3.8, n), device=dev),
                     torch.as_tensor(rng.uniform(2.0, 300.0, n), device=dev))
tgt = TA.ecef_from_geodetic(torch.as_tensor(rng.uniform(45.1, 46.2, m), device=dev),
                            torch.as_tensor(rng.uniform(3.1, 4.2, m), device=dev),
                            torch.as_tensor(rng.uniform(300.0, 5000.0, m), device=dev))
fraction = torch.as_tensor((2.0 * np.arange(n_f) + 1.0) / (2.0 * n_f), device=dev)
azimuth = torch.arange(m, dtype=torch.float64, device=dev) * (360.0 / m)
distance = torch.as_tensor(100.0 * 150.0 ** (np.arange(n_f) / (n_f - 1.0)), device=dev)
out = torch.zeros((n, m), dtype=torch.float64, device=dev)
sky = dict(elevation=torch.zeros((n, m), dtype=torch.float64, device=dev),
           range=torch.zeros((n, m), dtype=torch.float64, device=dev))


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def fused(math_):
    TA.set_math(math_)
    return st.clearance(obs, tgt, fraction, 0, out=out)


def skyline(math_):
    TA.set_math(math_)
    return st.horizon(obs, azimuth, distance, 0, out=sky)


def composed():
    """clearance, sample and n_data from the calls the library had before clearance_n"""
    TA.set_math("strict")
    lows, samples, counts = [], [], []
    for r0 in range(0, n, chunk):
        p = obs[r0:r0 + chunk]
        c = p.shape[0]
        d = tgt.reshape(1, m, 1, 3) - p.reshape(c, 1, 1, 3)
        q = (p.reshape(c, 1, 1, 3) + fraction.reshape(1, 1, n_f, 1) * d).reshape(-1, 3)
        la, lo, _ = TA.ecef_to_geodetic(q)
        ground, di = st.position(la, lo, 0.0, 0)
        lam, phi = lo * (math.pi / 180.0), la * (math.pi / 180.0)
        cp = torch.cos(phi)
        up = torch.stack([torch.cos(lam) * cp, torch.sin(lam) * cp, torch.sin(phi)], 1)
        data = (di >= 0).reshape(c, m, n_f)
        height = torch.where(data, (up * (q - ground)).sum(-1).reshape(c, m, n_f), math.inf)
        low = height.min(-1)
        lows.append(low.values)
        samples.append(torch.where(torch.isinf(low.values), 0, low.indices + 1))
        counts.append(data.sum(-1))
    return torch.cat(lows), torch.cat(samples), torch.cat(counts)


fused("fast"), fused("strict"), skyline("fast"), skyline("strict"), composed()
torch.cuda.synchronize()
arms = dict(fast=lambda: fused("fast"), strict=lambda: fused("strict"), horizon_fast=lambda: skyline("fast"),
            horizon_strict=lambda: skyline("strict"), composed=composed)
best = {name: 1e30 for name in arms}
for _ in range(reps):   # alternated, so that all see the same machine
    for name, arm in arms.items():
        best[name] = min(best[name], event_ms(arm))
got = {k: v.clone() for k, v in fused("strict").items()}
low, sample, count = composed()
TA.set_math("fast")
lines = sample > 0
res = dict(observers=n, targets=m, fractions=n_f, samples=n * m * n_f, library=os.path.relpath(TA.library_path(), ROOT))
for name, ms in best.items():
    res[name + "_ms"] = ms
    res[name + "_ns_per_sample"] = ms * 1e6 / res["samples"]
res.update(composed_over_fast=best["composed"] / best["fast"], composed_over_strict=best["composed"] / best["strict"],
           fast_over_horizon_fast=best["fast"] / best["horizon_fast"],
           strict_over_horizon_strict=best["strict"] / best["horizon_strict"],
           samples_with_data=float(count.sum() / res["samples"]), lines_open=float((low[lines] >= 0).double().mean()),
           same_n_data=bool((got["n_data"] == count).all()), samples_that_differ=int((got["sample"] != sample).sum()),
           worst_clearance_difference=float((got["clearance"] - low)[lines].abs().max()))
print(json.dumps(res), flush=True)
path = sys.argv[1] if len(sys.argv) > 1 else None
if path:
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(res, f, indent=1)
