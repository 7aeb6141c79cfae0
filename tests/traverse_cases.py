"""Geometries and the CPU checker of turtle_stepper_traverse_n, shared by
tests/golden/generate_traverse.py and the traverse tests.

Three geometries on one 1201^2 tile at (45N, 3E): "hgt" the sin.cos ground of
synth.srtm_like_nodes with one map layer, "two" the same tile in the two-layer
shape of amd_build.two_layer_stepper (offsets -0.5 / 0, three media), "rough"
synth.rough_nodes.  The checker (tests/c/traverse_loop.c) runs the loop over
the oracle's restatement of turtle_stepper_step, built at test time.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from oracle import ffi as O
from turtle_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAT0, LON0, N = 45, 3, 1201
ROUGH_SEED, ROUGH_AMPLITUDE = 1, 800
CASES = ("hgt", "two", "rough")


def nodes(case, n=N):
    if case == "rough":
        return synth.rough_nodes(n, ROUGH_SEED, ROUGH_AMPLITUDE)
    return synth.srtm_like_nodes(LAT0, LON0, n)


def layers(case):
    if case == "two":
        return [[(O.FLAT, 0, off), (O.MAP, 0, off)] for off in (-0.5, 0.0)]
    return [[(O.MAP, 0, 0.0)]]


def oracle_geometry(case, n=N):
    return O.OracleGeometry(grids=[O.hgt_grid(LAT0, LON0, nodes(case, n))], layers=layers(case))


def write_tile(directory, case, n=N):
    """the case's tile as an .hgt file in `directory` (one case a directory: the names agree)"""
    if case == "rough":
        return synth.write_rough_hgt(str(directory), LAT0, LON0, n, ROUGH_SEED, ROUGH_AMPLITUDE)
    return synth.write_hgt(str(directory), LAT0, LON0, n)


_checker = None


def checker():
    """tests/c/traverse_loop.c, compiled against oracle/libturtle_oracle.so"""
    global _checker
    if _checker is None:
        O.lib()  # builds libturtle_oracle.so if needed
        odir = os.path.join(ROOT, "oracle")
        out = tempfile.mkdtemp(prefix="turtle_traverse_")
        so = os.path.join(out, "libtraverse_loop.so")
        subprocess.check_call(["gcc", "-O2", "-std=gnu99", "-fPIC", "-ffp-contract=off", "-pthread",
                               "-shared", "-I" + odir, "-o", so,
                               os.path.join(ROOT, "tests", "c", "traverse_loop.c"),
                               "-L" + odir, "-lturtle_oracle", "-Wl,-rpath," + odir, "-lm"])
        _checker = C.CDLL(so)
    return _checker


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def check(geometry, position, direction, altitude_max=np.inf, max_steps=1000000, threads=None, slope=0.4,
          resolution=1e-2):
    """The loop over the CPU restatement: index, length [media][n], n_steps, n_crossings, position"""
    pos = np.array(position, dtype=np.float64, order="C").reshape(-1, 3)
    d = np.ascontiguousarray(direction, dtype=np.float64).reshape(-1, 3)
    n = pos.shape[0]
    media = geometry.n_layers + 1
    out = dict(index=np.empty((n, 2), dtype=np.int32), length=np.zeros((media, n)),
               n_steps=np.empty(n, dtype=np.int32), n_crossings=np.empty(n, dtype=np.int32))
    threads = threads or min(64, os.cpu_count() or 1)
    checker().traverse_loop(geometry.ref, C.c_double(slope), C.c_double(resolution), C.c_long(n), _p(pos), _p(d),
                            C.c_double(altitude_max), C.c_int(max_steps), _p(out["index"]),
                            _p(out["length"]), _p(out["n_steps"]), _p(out["n_crossings"]),
                            C.c_int(threads))
    out["position"] = pos
    return out
