#!/usr/bin/env python3
"""resample.npz: maps filled node by node by the REAL reference.  Build container only:

    make -C oracle ref && python tests/golden/generate_resample.py

For each case of tests/resample_cases.py the reference runs the loop of its
examples/example-projection.c, as turtle_map_resample states it (include/turtle_amd.h), on a map
whose nodes first hold resample_cases.sentinel:

    turtle_map_node(map, ix, iy, &x, &y, NULL);
    if projected: turtle_projection_unproject(turtle_map_projection(map), x, y, &lat, &lon);
    else          lat = y, lon = x;
    stack:  turtle_stack_elevation(stack, lat, lon, &z, &inside);
    map:    (u, v) = same projection ? (x, y) : projected source ? turtle_projection_project(
                     turtle_map_projection(source), lat, lon) : (lon, lat);
            turtle_map_elevation(source, u, v, &z, &inside);
    if (inside) turtle_map_fill(map, ix, iy, z);

Stored per case: the codes afterwards ([ny, nx] uint16, read back through turtle_map_node), the
outside mask, and the mask of nodes turtle_map_fill refused (outside the span: case f).  For f
the loop runs a second time with z clamped to the span first (TURTLE_AMD_RESAMPLE_CLAMP).  Map d
and e read map a as the reference left it."""
from __future__ import annotations

import ctypes as C
import hashlib
import os
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_ffi as R  # noqa: E402

import resample_cases as RC  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
D = C.c_double


def ref_map(case):
    nx, ny, x, y, z, proj, _ = RC.CASES[case]
    L = R.lib()
    h = C.c_void_p()
    info = R.MapInfo(nx, ny, (D * 2)(*x), (D * 2)(*y), (D * 2)(*z), None)
    assert L.turtle_map_create(C.byref(h), C.byref(info), proj.encode() if proj else None) == 0, R.errors()
    m = RC.meta(case)
    before = RC.sentinel(nx, ny)
    for iy in range(ny):
        for ix in range(nx):
            assert L.turtle_map_fill(h, ix, iy, D(m["z0"] + int(before[iy, ix]) * m["dz"])) == 0
    assert np.array_equal(codes_of(h, m), before)
    return h


def codes_of(h, m):
    L = R.lib()
    out = np.empty((m["ny"], m["nx"]), dtype=np.uint16)
    z = D()
    for iy in range(m["ny"]):
        for ix in range(m["nx"]):
            assert L.turtle_map_node(h, ix, iy, None, None, C.byref(z)) == 0
            out[iy, ix] = int(np.rint((z.value - m["z0"]) / m["dz"]))
    return out


def run(case, h, stack=None, source=None, clamp=False):
    """the loop; -> (outside mask, refused mask)"""
    L = R.lib()
    L.turtle_map_projection.restype = C.c_void_p
    m = RC.meta(case)
    proj = L.turtle_map_projection(h)
    sproj, same = None, False
    if source is not None:
        sproj = L.turtle_map_projection(source[0])
        same = RC.same_projection(m["projection"], RC.meta(source[1])["projection"])
    outside = np.zeros((m["ny"], m["nx"]), dtype=bool)
    refused = np.zeros_like(outside)
    x, y, la, lo, u, v, z = (D() for _ in range(7))
    inside = C.c_int()
    top = m["z0"] + 65535 * m["dz"]
    for ix in range(m["nx"]):
        for iy in range(m["ny"]):
            assert L.turtle_map_node(h, ix, iy, C.byref(x), C.byref(y), None) == 0
            if proj:
                assert L.turtle_projection_unproject(C.c_void_p(proj), x, y, C.byref(la), C.byref(lo)) == 0
            else:
                la.value, lo.value = y.value, x.value
            z.value = 0.0
            if stack is not None:
                assert L.turtle_stack_elevation(stack, la, lo, C.byref(z), C.byref(inside)) == 0
            else:
                if same:
                    u.value, v.value = x.value, y.value
                elif sproj:
                    assert L.turtle_projection_project(C.c_void_p(sproj), la, lo, C.byref(u), C.byref(v)) == 0
                else:
                    u.value, v.value = lo.value, la.value
                assert L.turtle_map_elevation(source[0], u, v, C.byref(z), C.byref(inside)) == 0
            if not inside.value:
                outside[iy, ix] = True
                continue
            zz = z.value
            if clamp and not (m["z0"] <= zz <= top):
                zz = m["z0"] if zz < m["z0"] else top
            if L.turtle_map_fill(h, ix, iy, D(zz)) != 0:
                refused[iy, ix] = True
    R.errors()
    return outside, refused


def main():
    assert R.available(), "build the reference first: make -C oracle ref"
    work = tempfile.mkdtemp()
    out = {}
    try:
        stacks = {}
        for which in ("stack", "void"):
            s = C.c_void_p()
            d = RC.tile_dir(work, "void" if which == "void" else "ground")
            assert R.lib().turtle_stack_create(C.byref(s), d.encode(), 0, None, None) == 0, R.errors()
            stacks[which] = s
        maps = {}
        for case in RC.CASES:
            m = RC.meta(case)
            h = ref_map(case)
            src = m["source"]
            if src in stacks:
                outside, refused = run(case, h, stack=stacks[src])
            else:
                outside, refused = run(case, h, source=(maps[src], src))
            maps[case] = h
            out[f"{case}_codes"] = codes_of(h, m)
            out[f"{case}_outside"] = outside
            out[f"{case}_refused"] = refused
            print(case, m["nx"], m["ny"], "outside", int(outside.sum()), "refused", int(refused.sum()))
            if refused.any():
                hc = ref_map(case)
                outside_c, refused_c = run(case, hc, stack=stacks[src], clamp=True)
                assert np.array_equal(outside_c, outside) and not refused_c.any()
                out[f"{case}_clamped_codes"] = codes_of(hc, m)
        for which in ("stack", "void"):
            R.lib().turtle_stack_destroy(C.byref(stacks[which]))
    finally:
        shutil.rmtree(work)
    # arrays that do not compress go as their sha256 (none so far: the codes of smooth ground do)
    path = os.path.join(OUT, "resample.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", hashlib.sha256(open(path, "rb").read()).hexdigest())


if __name__ == "__main__":
    main()
