"""tests/c/device_loops.hip built once per session into a shared library, and its launchers."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
FLAGS = ["--offload-arch=gfx950", "-ffp-contract=off", "-O3", "-std=c++17", "-Wall", "-Werror",
         "-I", os.path.join(ROOT, "include")]
SOURCE = os.path.join(ROOT, "tests", "c", "device_loops.hip")
MATH = {"fast": 0, "strict": 1}

_lib = None
_dir = None


def compile_object(source, out, extra=()):
    """one translation unit for gfx950 with only include/ on the path; returns the compiler's stderr
    (the resource remarks, when asked for)"""
    run = subprocess.run([HIPCC] + FLAGS + list(extra) + ["-fPIC", "-c", source, "-o", out],
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-4000:]
    return run.stderr


def lib():
    global _lib, _dir
    if _lib is None:
        _dir = tempfile.TemporaryDirectory(prefix="device_loops_")
        so = os.path.join(_dir.name, "libdevice_loops.so")
        run = subprocess.run([HIPCC] + FLAGS + ["-fPIC", "-shared", SOURCE, "-o", so],
                             capture_output=True, text=True)
        assert run.returncode == 0, run.stderr[-4000:]
        L = C.CDLL(so)
        L.loops_view_size.restype = C.c_long
        _lib = L
    return _lib


def _p(t):
    return C.c_void_p(t.data_ptr())


def traverse(view, math, position, direction, ceiling, max_steps, media, simple=0, blocks=0):
    """the traverse test kernels (simple: on step(), else on Stepping::trip()); numpy in and out, in
    the layout of Stepper.traverse"""
    import torch
    pos = torch.tensor(np.ascontiguousarray(position, dtype=np.float64), device="cuda")
    d = torch.tensor(np.ascontiguousarray(direction, dtype=np.float64), device="cuda")
    n = pos.shape[0]
    index = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
    length = torch.zeros((media, n), dtype=torch.float64, device="cuda")
    n_steps = torch.zeros(n, dtype=torch.int32, device="cuda")
    n_cross = torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    blocks = blocks or max(1, min((n + 255) // 256, 4096))
    rc = lib().loops_traverse(view, MATH[math], simple, blocks, None, C.c_long(n), _p(pos), _p(d),
                              C.c_double(ceiling), int(max_steps), _p(index), _p(length), _p(n_steps),
                              _p(n_cross))
    assert rc == 0, f"loops_traverse: {rc}"
    return dict(position=pos.cpu().numpy(), index=index.cpu().numpy(), length=length.cpu().numpy(),
                n_steps=n_steps.cpu().numpy(), n_crossings=n_cross.cpu().numpy())


def records(view, math, position, direction, k_steps):
    import torch
    pos = torch.tensor(np.ascontiguousarray(position, dtype=np.float64), device="cuda")
    d = torch.tensor(np.ascontiguousarray(direction, dtype=np.float64), device="cuda")
    n = pos.shape[0]
    rec = torch.zeros((k_steps, n, 11), dtype=torch.float64, device="cuda")
    taken = torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = lib().loops_records(view, MATH[math], (n + 255) // 256, None, C.c_long(n), _p(pos), _p(d),
                             int(k_steps), _p(rec), _p(taken))
    assert rc == 0, f"loops_records: {rc}"
    return rec.cpu().numpy(), taken.cpu().numpy()


def walk(view, math, state, seed, n_steps, first_ray=0, first_step=0, blocks=0):
    """the scattering walk kernel from a state as Stepper.scatter keeps it (numpy arrays); returns
    the new state"""
    import torch
    t = {k: torch.tensor(np.ascontiguousarray(v), device="cuda") for k, v in state.items()}
    n = t["position"].shape[0]
    torch.cuda.synchronize()
    blocks = blocks or max(1, min((n + 255) // 256, 4096))
    rc = lib().loops_walk(view, MATH[math], blocks, None, C.c_long(n), C.c_ulonglong(seed),
                          C.c_long(first_ray), int(first_step), int(n_steps), _p(t["position"]),
                          _p(t["altitude"]), _p(t["elevation"]), _p(t["index"]), _p(t["length"]),
                          _p(t["steps"]))
    assert rc == 0, f"loops_walk: {rc}"
    return {k: v.cpu().numpy() for k, v in t.items()}
