"""Experiment: turtle_stepper_traverse_n (lines of sight through every medium) on C2's tile.

Two workloads on the 3601^2 tile of BASELINE's C2:
  valley  one detector 0.5 m above the lowest node near the tile's middle, RAYS directions
          (azimuth U[0, 360), elevation U[0, 30] degrees), ceiling 2000 m;
  c2      C2's rays (500 m up, -10 .. -1 degrees), ceiling 2000 m.
For each: ms a call (CUDA events, best of REPS after a warm-up), ray-steps/s, samples a step
(trace_stats); the same rays with no ceiling through (i) traverse_n and (ii) what a caller
writes today -- step_n to sample the origins, then trace_n with TURTLE_AMD_TRACE_RESUME pass after
pass until every ray has left the data, its lengths added per medium with torch; and the CPU
checker (tests/c/traverse_loop.c) on a CPU_RAYS subset on every core.

    python scripts/exp_traverse.py [out.json]        (RAYS, CPU_RAYS, REPS: environment)
"""
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import turtle_amd as TA  # noqa: E402
from turtle_amd import sharding, synth  # noqa: E402
from oracle import ffi as O  # noqa: E402

import traverse_cases as TC  # noqa: E402

n = int(os.environ.get("RAYS", "1000000"))
cpu_rays = int(os.environ.get("CPU_RAYS", "100000"))
reps = int(os.environ.get("REPS", "5"))
dev = torch.device("cuda", 0)

tmp = tempfile.mkdtemp(prefix="turtle_traverse_")
nodes = synth.srtm_like_nodes(45, 3)
terrain = TA.Map.load(synth.write_hgt(tmp, 45, 3))
st = TA.Stepper()
st.add_map(terrain, 0.0)
stream = torch.cuda.Stream()
torch.cuda.set_stream(stream)
TA.set_stream(stream)
geo = O.OracleGeometry(grids=[O.hgt_grid(45, 3, nodes)], layers=[[(O.MAP, 0, 0.0)]])


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


def timed(fn):
    fn()
    torch.cuda.synchronize()
    best = 1e30
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b))
    return best


def resume_loop(pos0, d):
    """what a caller writes today: sample the origins, then trace_n + RESUME until all have left"""
    pos = pos0.clone()
    s = st.step(pos)
    index = s["index"]
    length = torch.zeros((st.media, pos.shape[0]), dtype=torch.float64, device=dev)
    passes = 0
    while True:
        m = index[:, 0].long()
        live = m >= 0
        if not bool(live.any()):
            break
        t = st.trace(pos, d, max_steps=1000000, resume_index=index)
        length.index_put_((m.clamp(min=0), torch.arange(pos.shape[0], device=dev)),
                          torch.where(live, t["length"], torch.zeros_like(t["length"])), accumulate=True)
        index = t["index"]
        passes += 1
    return length, index, passes


out = {}
for name in ("valley", "c2"):
    pos0, d = workload(name)
    row = {}
    for ceiling in (2000.0, float("inf")):
        key = "ceiling" if ceiling < 1e30 else "no_ceiling"
        res = {}
        ms = timed(lambda: st.traverse(pos0.clone(), d, ceiling))
        t = st.traverse(pos0.clone(), d, ceiling)
        s = st.trace_stats()
        res.update(ms=ms, steps=int(s["steps"]), ray_steps_per_s=s["steps"] / (ms * 1e-3),
                   samples_per_step=s["samples"] / max(s["steps"], 1),
                   crossings_mean=float(t["n_crossings"].double().mean()),
                   crossings_max=int(t["n_crossings"].max()))
        if key == "no_ceiling":
            ms_loop = timed(lambda: resume_loop(pos0, d))
            length, index, passes = resume_loop(pos0, d)
            res.update(resume_loop_ms=ms_loop, resume_loop_passes=passes,
                       resume_loop_same_index=bool((index == t["index"]).all()),
                       resume_loop_max_rel=float(((length - t["length"]).abs().sum(0) /
                                                  t["length"].sum(0).clamp(min=1e-300)).max()))
        # the CPU checker on a subset, every core
        k = min(cpu_rays, n)
        p, dd = pos0[:k].cpu().numpy(), d[:k].cpu().numpy()
        t0 = time.perf_counter()
        ref = TC.check(geo, p, dd, ceiling)
        cpu_s = time.perf_counter() - t0
        steps_cpu = int(ref["n_steps"].sum())
        res.update(cpu_rays=k, cpu_threads=min(64, os.cpu_count() or 1), cpu_s=cpu_s,
                   cpu_ray_steps_per_s=steps_cpu / cpu_s,
                   cpu_same_steps=bool((ref["n_steps"] == t["n_steps"][:k].cpu().numpy()).all()))
        row[key] = res
        print(name, key, json.dumps(res), flush=True)
    out[name] = row

path = sys.argv[1] if len(sys.argv) > 1 else None
if path:
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(dict(rays=n, math=TA.get_math(), workloads=out), f, indent=1)
