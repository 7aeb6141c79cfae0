"""The CPU checker of turtle_stepper_crossings_n (tests/c/crossings_loop.c over the oracle's
restatement of turtle_stepper_step) and the ragged form the crossings are compared in, shared by
the crossings tests.  The geometries are those of traverse_cases.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from oracle import ffi as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_checker = None


def checker():
    """tests/c/crossings_loop.c, compiled against oracle/libturtle_oracle.so"""
    global _checker
    if _checker is None:
        O.lib()  # builds libturtle_oracle.so if needed
        odir = os.path.join(ROOT, "oracle")
        out = tempfile.mkdtemp(prefix="turtle_crossings_")
        so = os.path.join(out, "libcrossings_loop.so")
        subprocess.check_call(["gcc", "-O2", "-std=gnu99", "-fPIC", "-ffp-contract=off", "-pthread",
                               "-shared", "-I" + odir, "-o", so,
                               os.path.join(ROOT, "tests", "c", "crossings_loop.c"),
                               "-L" + odir, "-lturtle_oracle", "-Wl,-rpath," + odir, "-lm"])
        _checker = C.CDLL(so)
    return _checker


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def check(geometry, position, direction, altitude_max=np.inf, max_steps=1000000, threads=None, slope=0.4,
          resolution=1e-2):
    """The loop over the CPU restatement, twice (the counts, then every crossing): traverse's
    outputs (index, length [media][n], n_steps, n_crossings, position) and the crossings, ragged:
    ray r's are rows offset[r] .. offset[r + 1] - 1 of point [rows][3], distance [rows] and
    media [rows][2]."""
    pos0 = np.array(position, dtype=np.float64, order="C").reshape(-1, 3)
    d = np.ascontiguousarray(direction, dtype=np.float64).reshape(-1, 3)
    n = pos0.shape[0]
    media = geometry.n_layers + 1
    threads = threads or min(64, os.cpu_count() or 1)
    offset = None
    for _ in range(2):
        pos = pos0.copy()
        out = dict(index=np.empty((n, 2), dtype=np.int32), length=np.zeros((media, n)),
                   n_steps=np.empty(n, dtype=np.int32), n_crossings=np.empty(n, dtype=np.int32))
        rows = 0 if offset is None else int(offset[-1])
        rec = dict(point=np.zeros((rows, 3)), distance=np.zeros(rows), media=np.zeros((rows, 2), np.int32))
        checker().crossings_loop(geometry.ref, C.c_double(slope), C.c_double(resolution), C.c_long(n), _p(pos),
                                 _p(d), C.c_double(altitude_max), C.c_int(max_steps), _p(out["index"]),
                                 _p(out["length"]), _p(out["n_steps"]), _p(out["n_crossings"]),
                                 _p(offset), _p(rec["point"]), _p(rec["distance"]), _p(rec["media"]),
                                 C.c_int(threads))
        if offset is None:
            offset = np.zeros(n + 1, dtype=np.int64)
            np.cumsum(out["n_crossings"], out=offset[1:])
    out.update(rec, offset=offset, position=pos)
    return out


def ragged(t):
    """The recorded crossings of a crossings() result (numpy arrays), ray by ray as check() has
    them: offset [n + 1] over min(n_crossings, capacity) rows a ray, point, distance, media."""
    capacity = t["distance"].shape[0]
    kept = np.minimum(t["n_crossings"], capacity)
    sel = np.arange(capacity)[None, :] < kept[:, None]   # [n][capacity]: ray-major
    offset = np.zeros(kept.shape[0] + 1, dtype=np.int64)
    np.cumsum(kept, out=offset[1:])
    return dict(offset=offset, point=t["point"].transpose(1, 0, 2)[sel], distance=t["distance"].T[sel],
                media=t["media"].transpose(1, 0, 2)[sel])


def first(rows, capacity):
    """rows (offset, point, distance, media) cut to the first `capacity` crossings of each ray"""
    counts = np.diff(rows["offset"])
    slot = np.arange(int(rows["offset"][-1])) - np.repeat(rows["offset"][:-1], counts)
    keep = slot < capacity
    offset = np.zeros(counts.shape[0] + 1, dtype=np.int64)
    np.cumsum(np.minimum(counts, capacity), out=offset[1:])
    return dict(offset=offset, point=rows["point"][keep], distance=rows["distance"][keep],
                media=rows["media"][keep])
