"""Experiment: turtle_stepper_advance_n next to turtle_stepper_traverse_n on C2's tile.

RAYS rays of BASELINE's C2 recipe (500 m up, -10 .. -1 degrees) over the 3601^2 tile with a 2000 m
ceiling, device-resident.  Three calls, alternated so that all see the same machine, each timed with
device events REPS times after a warm-up (median, least and most):
  traverse   traverse_n with length = NULL;
  advance    advance_n with budget = inf and no distance limit: the same samples as traverse;
  budgets    advance_n with the budgets of tests/advance_cases.py's recipe (u D and v T, the same
             distributions; without the redraw that keeps a stop off a crossing, which matters to a
             check and not to a time).
In both arithmetics.  Kernel times: run it under `rocprofv3 --kernel-trace --stats`.

    python scripts/exp_advance.py [out.txt]        (RAYS, REPS: environment)
"""
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
ceiling = 2000.0

tmp = tempfile.mkdtemp(prefix="turtle_advance_")
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
density = torch.tensor([2650.0, 1.205], device=dev)
infinite = torch.full((n,), float("inf"), device=dev, dtype=torch.float64)


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    fn()
    b.record(stream)
    torch.cuda.synchronize()
    return a.elapsed_time(b)


lines = [f"rays {n}, reps {reps}, ceiling {ceiling} m, device-resident, ms a call: median [least .. most]"]
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
    calls = dict(
        traverse=lambda: st.traverse(pos0.clone(), d, ceiling, want=("n_steps", "n_crossings")),
        advance=lambda: st.advance(pos0.clone(), d, density, infinite, None, ceiling),
        budgets=lambda: st.advance(pos0.clone(), d, density, budget, limit, ceiling))
    for fn in calls.values():
        fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            ms[k].append(event_ms(fn))
    t, a, b = (fn() for fn in calls.values())
    torch.cuda.synchronize()
    same = all(bool(torch.equal(t[k], a[k])) for k in ("position", "index", "n_steps"))
    med = {k: statistics.median(v) for k, v in ms.items()}
    for k in calls:
        lines.append(f"{math:6s} {k:8s} {med[k]:8.3f} [{min(ms[k]):8.3f} .. {max(ms[k]):8.3f}]")
    lines.append(f"{math:6s} advance / traverse {med['advance'] / med['traverse']:.3f}, budgets / traverse "
                 f"{med['budgets'] / med['traverse']:.3f}; same bits as traverse: {same}; steps {int(t['n_steps'].sum())} "
                 f"(budgets: {int(b['n_steps'].sum())}); status of budgets "
                 f"{torch.bincount(b['status'], minlength=5).tolist()}")
print("\n".join(lines), flush=True)

if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        f.write("\n".join(lines) + "\n")
