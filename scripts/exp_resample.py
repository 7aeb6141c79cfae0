"""Experiment: turtle_map_resample's rate (nodes/s), the workload of the reference's
examples/example-projection.c at the size of a local muography map.

A Lambert 93 map of SIDE^2 nodes (default 10 000^2 = 10^8, 10 m apart, 100 km a side around
46N 3E) filled from a 2 x 2 stack of 3601^2 synthetic SRTM tiles (N45-N46 x E002-E003):
  resident  every tile in HBM (a warm-up call first), best of REPS calls;
  paged     the same map over a stack of stack_size 1, which pages the four tiles in round by
            round (one call, from a cold stack);
and, where the reference's build exists (oracle/_ref), the reference's own loop on one CPU core
over a CPU_SIDE^2 map on the same ground (scripts/ref_resample_loop.c).  The kernel's share of a
call comes from a separate run under rocprofv3 --kernel-trace --stats.

    python scripts/exp_resample.py [out.json]        (SIDE, CPU_SIDE, REPS: environment)
"""
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import turtle_amd as TA  # noqa: E402
from turtle_amd import synth  # noqa: E402

side = int(os.environ.get("SIDE", "10000"))
cpu_side = int(os.environ.get("CPU_SIDE", "1000"))
reps = int(os.environ.get("REPS", "3"))
only_cpu = os.environ.get("ONLY_CPU") == "1"
SPAN = 100000.0  # m
X0, Y0 = 700000.0 - SPAN / 2, 6544474.0 - SPAN / 2  # 46N 3E in Lambert 93, at the centre

tmp = tempfile.mkdtemp(prefix="turtle_resample_")
for la in (45, 46):
    for lo in (2, 3):
        synth.write_hgt(tmp, la, lo)
out = dict(side=side, nodes=side * side)


def target(n):
    return TA.Map.create(shape=(n, n), x=(X0, X0 + SPAN), y=(Y0, Y0 + SPAN), z=(0.0, 2000.0),
                         projection="Lambert 93")


if not only_cpu:
    m = target(side)
    stack = TA.Stack(tmp, 0)
    stack.load()
    m.resample(stack=stack)
    times = []
    for _ in range(reps):
        t = time.perf_counter()
        outside, clamped = m.resample(stack=stack)
        times.append(time.perf_counter() - t)
    out["resident_s"] = min(times)
    out["resident_nodes_per_s"] = side * side / min(times)
    out["outside"], out["clamped"] = outside, clamped
    stack.destroy()
    paged = TA.Stack(tmp, 1)
    t = time.perf_counter()
    m.resample(stack=paged)
    out["paged_s"] = time.perf_counter() - t
    out["paged_nodes_per_s"] = side * side / out["paged_s"]
    paged.destroy()
    m.destroy()

ref = os.path.join(ROOT, "oracle", "_ref", "libturtle_ref.so")
if os.path.exists(ref) and cpu_side > 0:
    exe = os.path.join(tmp, "ref_resample_loop")
    subprocess.check_call(["gcc", "-O2", "-std=gnu99", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "scripts", "ref_resample_loop.c"), "-o", exe, ref,
                           "-Wl,-rpath," + os.path.dirname(ref), "-lm"])
    nodes, outside, seconds = subprocess.check_output(
        [exe, tmp, str(cpu_side), str(cpu_side), str(X0), str(X0 + SPAN), str(Y0), str(Y0 + SPAN),
         "0", "2000", "Lambert 93"]).split()
    out["cpu_reference_nodes"] = int(nodes)
    out["cpu_reference_s"] = float(seconds)
    out["cpu_reference_nodes_per_s"] = int(nodes) / float(seconds)
elif cpu_side > 0:
    out["cpu_reference"] = "not built here (oracle/_ref)"

print(json.dumps(out))
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
