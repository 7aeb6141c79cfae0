"""Experiment: what the walk through a density grid costs turtle_stepper_advance_n on C2's tile.

RAYS rays of BASELINE's C2 recipe (500 m up, -10 .. -1 degrees) over the 3601^2 tile with a 2000 m
ceiling, device-resident.  Three calls, alternated so that all see the same machine, each timed with
device events REPS times after a warm-up (median, least and most):
  advance    advance_n: one density a medium (the yardstick: its kernel instance is the parent's);
  uniform    advance_grid_n, every voxel at density[0]: the walk's arithmetic, the same stops;
  grid       advance_grid_n with the box and the voxels of tests/advance_grid_cases.py (the tile is
             the fixture's, at three times its resolution: the box is the same).
Each with infinite budgets (every ray walks to its end) and with the budgets of
tests/advance_cases.py's recipe drawn from this run's own traverse (u D and v T; D of one density a
medium).  In both arithmetics.  Then, on the CPU checker over the first SAMPLE rays: how many steps
begin in the rock, how many of them meet the box, and how many voxels such a step meets.
Kernel times: run it under `rocprofv3 --kernel-trace --stats`.

    python scripts/exp_advance_grid.py [out.txt]        (RAYS, REPS, SAMPLE: environment)
"""
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import turtle_amd as TA  # noqa: E402
from turtle_amd import sharding, synth  # noqa: E402

import advance_grid_cases as AG  # noqa: E402
import traverse_cases as TC  # noqa: E402

n = int(os.environ.get("RAYS", "1000000"))
reps = int(os.environ.get("REPS", "9"))
sample = int(os.environ.get("SAMPLE", "2000"))
dev = torch.device("cuda", 0)
ceiling = 2000.0

tmp = tempfile.mkdtemp(prefix="turtle_advance_grid_")
terrain = TA.Map.load(synth.write_hgt(tmp, 45, 3))
st = TA.Stepper()
st.add_map(terrain, 0.0)
stream = torch.cuda.Stream()
torch.cuda.set_stream(stream)
TA.set_stream(stream)

lat, lon, az, el = (torch.as_tensor(v, device=dev) for v in sharding.rank_rays(n, 0, (45., 46.), (3., 4.)))
pos0, di = st.position(lat, lon, 500.0)
assert bool((di >= 0).all())
d = TA.ecef_from_horizontal(lat, lon, az, el)
rho = [2650.0, 1.205]
density = torch.tensor(rho, device=dev)
infinite = torch.full((n,), float("inf"), device=dev, dtype=torch.float64)
grids = dict(
    uniform=TA.Grid.enu(AG.LATITUDE, AG.LONGITUDE, AG.HEIGHT, AG.SIZE,
                        torch.full(AG.N[::-1], rho[0], device=dev, dtype=torch.float64), offset=AG.OFFSET),
    grid=TA.Grid.enu(AG.LATITUDE, AG.LONGITUDE, AG.HEIGHT, AG.SIZE, torch.tensor(AG.voxels(), device=dev),
                     offset=AG.OFFSET))


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b)


lines = [f"rays {n}, reps {reps}, ceiling {ceiling} m, device-resident, box {AG.N} voxels of {AG.SIZE} m, "
         f"ms a call: median [least .. most]"]
for math in ("fast", "strict"):
    TA.set_math(math)
    length = st.traverse(pos0.clone(), d, ceiling, want=("length",))["length"]
    rng = np.random.default_rng(0xAD7A2CE)
    u = np.where(rng.random(n) < 0.05, np.inf, rng.uniform(0.05, 1.6, n))
    v = np.where(rng.random(n) < 0.6, np.inf, rng.uniform(0.05, 1.6, n))
    budget = torch.as_tensor(u, device=dev) * (density[:, None] * length).sum(dim=0)
    limit = torch.as_tensor(v, device=dev) * length.sum(dim=0)
    budget = torch.where(length.sum(dim=0) > 0, budget, torch.ones_like(budget))
    limit = torch.where(length.sum(dim=0) > 0, limit, infinite)
    for label, (b, m) in dict(infinite=(infinite, None), budgets=(budget, limit)).items():
        calls = dict(advance=lambda: st.advance(pos0.clone(), d, density, b, m, ceiling))
        for name, g in grids.items():
            calls[name] = lambda g=g: st.advance(pos0.clone(), d, density, b, m, ceiling, grid=g)
        for fn in calls.values():
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in calls}
        for _ in range(reps):
            for k, fn in calls.items():
                ms[k].append(event_ms(fn))
        out = {k: fn() for k, fn in calls.items()}
        torch.cuda.synchronize()
        med = {k: statistics.median(t) for k, t in ms.items()}
        steps = {k: int(t["n_steps"].sum()) for k, t in out.items()}
        for k in calls:
            lines.append(f"{math:6s} {label:8s} {k:8s} {med[k]:8.3f} [{min(ms[k]):8.3f} .. {max(ms[k]):8.3f}]  steps {steps[k]}")
        off = float(((out["uniform"]["depth"] - out["advance"]["depth"]).abs()
                     / out["advance"]["depth"].clamp(min=1e-300)).nan_to_num(0.0).max())
        lines.append(f"{math:6s} {label:8s} uniform / advance {med['uniform'] / med['advance']:.3f}, grid / advance "
                     f"{med['grid'] / med['advance']:.3f}; the walk costs {1e6 * (med['grid'] - med['advance']) / steps['grid']:.3f} "
                     f"ns a step; uniform's depth off advance's by at most {off:.1e} of itself; status of grid "
                     f"{torch.bincount(out['grid']['status'], minlength=5).tolist()}")

# what a step meets, by the CPU checker on a sample of the rays (uncut)
k = min(sample, n)
box = AG.golden_box(grids["grid"].origin, grids["grid"].axis)
t = AG.check(TC.oracle_geometry("hgt", 3601), pos0[:k].cpu().numpy(), d[:k].cpu().numpy(), np.array(rho), box,
             np.full(k, np.inf), None, ceiling, tally=True)
rock, met, faces, pieces = (int(c) for c in t["tally"].astype(np.int64).sum(axis=0))
other = int(t["n_steps"].sum()) - rock
voxels = pieces - other - (rock - met) - 2 * met      # (a walk that meets the box: a piece before, the voxels, a piece after)
lines.append(f"CPU checker, {k} rays uncut: {int(t['n_steps'].sum())} steps, {rock} begin in the rock, {met} of those "
             f"meet the box ({faces} through a face in mid-step) and {voxels / max(met, 1):.2f} voxels each")
print("\n".join(lines), flush=True)

if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
