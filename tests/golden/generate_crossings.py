#!/usr/bin/env python3
"""crossings.npz: every crossing of the lines of sight of traverse.npz, computed by the REAL
reference.  Build container only:

    make -C oracle ref && python tests/golden/generate_crossings.py

The geometries and ray recipes are those of generate_traverse.py (imported: the 1201^2 tiles of
tests/traverse_cases.py, the "ground" and "c2" recipes of 1000 rays each, their ceilings).  The
reference (turtle_stepper_range_set(0)) runs, ray by ray with a fresh stepper history, the loop of
turtle_stepper_crossings_n:

    turtle_stepper_step(s, pos, NULL, NULL, NULL, &alt, NULL, NULL, idx);  d = 0;
    while (idx[0] >= 0 && alt < altitude_max && steps < max_steps) {
            m = idx[0];  turtle_stepper_step(s, pos, dir, NULL, NULL, &alt, NULL, &ds, idx);
            length[m][r] += ds;  d += ds;  steps++;
            if (idx[0] != m) record (pos, d, {m, idx[0]}) as the ray's next crossing;
    }

Stored per case and recipe, ragged (some rough rays have more than 50 crossings): the rows of ray r
are offset[r] .. offset[r + 1] - 1 of point [rows][3], distance [rows] and media [rows][2].  The
rays themselves are traverse.npz's."""
from __future__ import annotations

import ctypes as C
import os
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import ref_ffi as R  # noqa: E402

import generate_traverse as GT  # noqa: E402
import traverse_cases as TC  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
D = C.c_double


def loop(st, pos, d, altitude_max):
    step = R.lib().turtle_stepper_step
    n = pos.shape[0]
    offset = np.zeros(n + 1, dtype=np.int64)
    point, distance, media = [], [], []
    p, q = (D * 3)(), (D * 3)()
    alt, ds = D(), D()
    idx = (C.c_int * 2)()
    for r in range(n):
        st.reset()
        p[:] = pos[r]
        q[:] = d[r]
        assert step(st.h, p, None, None, None, C.byref(alt), None, None, idx) == 0
        k, total = 0, 0.0
        while idx[0] >= 0 and alt.value < altitude_max and k < GT.MAX_STEPS:
            m = idx[0]
            assert step(st.h, p, q, None, None, C.byref(alt), None, C.byref(ds), idx) == 0
            total += ds.value
            k += 1
            if idx[0] != m:
                point.append(tuple(p))
                distance.append(total)
                media.append((m, idx[0]))
        offset[r + 1] = len(distance)
    return offset, np.array(point).reshape(-1, 3), np.array(distance), np.array(media, np.int32).reshape(-1, 2)


def main():
    if not R.available():
        sys.exit("oracle/_ref/libturtle_ref.so missing: run `make -C oracle ref`")
    rays = np.load(os.path.join(OUT, "traverse.npz"))
    out = {}
    for case in TC.CASES:
        tmp = tempfile.mkdtemp(prefix="turtle_crossings_")
        try:
            m = R.RefMap.load(TC.write_tile(tmp, case))
            st = GT.ref_stepper(case, m)
            for recipe in ("ground", "c2"):
                key = f"{case}_{recipe}_"
                pos, d = GT.rays(st, recipe, len(TC.layers(case)) - 1)
                # the same rays as traverse.npz's, bit for bit
                assert np.array_equal(pos, rays[key + "position"]) and np.array_equal(d, rays[key + "direction"])
                offset, point, distance, media = loop(st, pos, d, float(rays[key + "ceiling"]))
                assert np.array_equal(np.diff(offset), rays[key + "n_crossings"])
                out.update({key + "offset": offset, key + "point": point, key + "distance": distance,
                            key + "media": media})
                print(f"{case:5s} {recipe:6s}: {offset[-1]} crossings")
            st.destroy()
            m.destroy()
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    np.savez_compressed(os.path.join(OUT, "crossings.npz"), **out)
    print("wrote", os.path.join(OUT, "crossings.npz"))


if __name__ == "__main__":
    main()
