"""Experiment: turtle_map_fill_n / turtle_map_node_n on a map of SIDE^2 nodes (default 3601^2: one
SRTM1 tile), best of REPS calls (default 5) after a warm-up, a host clock around calls that end in a
device synchronise.

  device   whole-map fill and read with torch tensors on the GPU (DEVICE space), and a WINDOW^2
           (default 100^2) fill in the middle of the map;
  host     the same from numpy arrays (HOST space: the rows go through HBM);
  loop     what there was before: a C loop of turtle_map_fill over every node
           (scripts/fill_loop.c), then the first turtle_map_elevation_n, which uploads the map;
  profile  a few calls of each kind in DEVICE space and nothing else, to run under rocprofv3:
               rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- \
                   python scripts/exp_fill.py --step profile
               rocprofv3 --pmc SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU \
                   SQ_ACTIVE_INST_VALU SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_WAIT_INST_ANY ... (its own run)

Without --step every step but `profile` runs as a child process under its own time limit, and the
JSON lines are gathered.  Algorithmic bytes: 8 B in + 2 B out a node for a fill, 2 B in + 8 B out
for a read.

    python scripts/exp_fill.py [out.json]        (SIDE, WINDOW, REPS: environment)
"""
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

side = int(os.environ.get("SIDE", "3601"))
window = int(os.environ.get("WINDOW", "100"))
reps = int(os.environ.get("REPS", "5"))
LIMITS = dict(device=240, host=240, loop=240)  # seconds


def best(call):
    call()
    times = []
    for _ in range(reps):
        t = time.perf_counter()
        call()
        times.append(time.perf_counter() - t)
    return min(times)


def rate(seconds, nodes):
    return dict(ms=seconds * 1e3, GB_per_s=10.0 * nodes / seconds * 1e-9)


def terrain(np):
    j = np.arange(side, dtype=np.float64)
    return 500.0 + 400.0 * np.sin(0.01 * j)[None, :] * np.cos(0.013 * j)[:, None]


def step_arrays(space):
    import numpy as np
    import torch  # noqa: F401  (before the library: tests/conftest.py)
    import turtle_amd as TA
    z = terrain(np)
    if space == "device":
        z = torch.as_tensor(z, device="cuda")
        torch.cuda.synchronize()
    m = TA.Map.create(shape=(side, side), x=(3.0, 4.0), y=(45.0, 46.0), z=(0.0, 2000.0))
    out = dict(side=side, nodes=side * side, window=window, reps=reps)
    t = time.perf_counter()
    m.fill_array(z)
    out["first_fill_ms"] = (time.perf_counter() - t) * 1e3  # (no HBM copy yet: nothing is uploaded)
    out["fill"] = rate(best(lambda: m.fill_array(z)), side * side)
    back = m.nodes(device=(space == "device"))

    def read():
        m.nodes(out=back)
        TA.synchronize()

    out["read"] = rate(best(read), side * side)
    at = (side - window) // 2
    patch = z[at:at + window, at:at + window]  # (rows `side` doubles apart)
    out["window_fill"] = rate(best(lambda: m.fill_array(patch, at, at)), window * window)
    wback = back[:window, :window]

    def wread():
        m.nodes(at, at, out=wback)
        TA.synchronize()

    out["window_read"] = rate(best(wread), window * window)
    m.destroy()
    return out


def step_loop():
    import turtle_amd as TA
    tmp = tempfile.mkdtemp(prefix="turtle_fill_")
    exe = os.path.join(tmp, "fill_loop")
    lib_dir = os.path.dirname(TA.library_path())
    subprocess.check_call(["gcc", "-O2", "-std=gnu99", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "scripts", "fill_loop.c"), "-o", exe, "-L" + lib_dir,
                           "-lturtle_amd", "-Wl,-rpath," + lib_dir, "-lm"])
    best_of = None
    for _ in range(reps):
        fill_s, first_s, again_s = (float(v) for v in subprocess.check_output([exe, str(side)]).split())
        if best_of is None or fill_s + first_s < best_of[0] + best_of[1]:
            best_of = (fill_s, first_s, again_s)
    return dict(side=side, fill_loop_ms=best_of[0] * 1e3, first_lookup_ms=best_of[1] * 1e3,
                next_lookup_ms=best_of[2] * 1e3, total_ms=(best_of[0] + best_of[1]) * 1e3)


def step_profile():
    import numpy as np
    import torch
    import turtle_amd as TA
    z = torch.as_tensor(terrain(np), device="cuda")
    torch.cuda.synchronize()
    m = TA.Map.create(shape=(side, side), x=(3.0, 4.0), y=(45.0, 46.0), z=(0.0, 2000.0))
    back = m.nodes(device=True)
    at = (side - window) // 2
    for _ in range(4):
        m.fill_array(z)
        m.nodes(out=back)
        m.fill_array(z[at:at + window, at:at + window], at, at)
    TA.synchronize()
    m.destroy()
    return dict(side=side, window=window, calls=4)


if __name__ == "__main__":
    if "--step" in sys.argv:
        name = sys.argv[sys.argv.index("--step") + 1]
        result = {"device": lambda: step_arrays("device"), "host": lambda: step_arrays("host"),
                  "loop": step_loop, "profile": step_profile}[name]()
        print(json.dumps({name: result}))
        sys.exit(0)
    gathered = {}
    for name, limit in LIMITS.items():
        done = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__),
                               "--step", name], capture_output=True, text=True)
        if done.returncode != 0:  # nothing more is started on the GPU after a step that failed
            sys.stderr.write(done.stdout + done.stderr)
            sys.exit(f"step {name} ended with status {done.returncode}")
        gathered.update(json.loads(done.stdout.strip().splitlines()[-1]))
    print(json.dumps(gathered))
    paths = [a for a in sys.argv[1:] if not a.startswith("-")]
    if paths:
        with open(paths[0], "w") as f:
            json.dump(gathered, f, indent=1)
