#!/usr/bin/env python3
"""fill.npz: what the REAL reference's turtle_map_fill stores.  Build container only:

    make -C oracle ref && python tests/golden/generate_fill.py

For each span of tests/fill_cases.py the reference makes a map of one row (turtle_map_create,
default encoding) and takes turtle_map_fill(map, k, 0, values[k]) for every value.  Stored per
span: the values, the mask of the values it refused (DOMAIN_ERROR: the node keeps the 0 of a new
map), and the code of every node afterwards, read back through turtle_map_node."""
from __future__ import annotations

import ctypes as C
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ref_ffi as R  # noqa: E402

import fill_cases as FC  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
D = C.c_double


def main():
    assert R.available(), "build the reference first: make -C oracle ref"
    L = R.lib()
    out = {}
    for name, span in FC.SPANS.items():
        v = FC.values(name)
        n = len(v)
        h = C.c_void_p()
        info = R.MapInfo(n, 1, (D * 2)(0.0, 1.0), (D * 2)(0.0, 0.0), (D * 2)(*span), None)
        assert L.turtle_map_create(C.byref(h), C.byref(info), None) == 0, R.errors()
        refused = np.zeros(n, dtype=bool)
        for k in range(n):
            rc = L.turtle_map_fill(h, k, 0, D(float(v[k])))
            assert rc in (0, 6), rc  # (TURTLE_RETURN_DOMAIN_ERROR)
            refused[k] = rc != 0
        texts = {m.split("} ")[-1] for _, m in R.errors()}
        assert texts <= {"elevation is outside of map span"}, texts
        codes = np.empty(n, dtype=np.uint16)
        z = D()
        dz = FC.dz_of(span)
        for k in range(n):
            assert L.turtle_map_node(h, k, 0, None, None, C.byref(z)) == 0
            code = int(np.rint((z.value - span[0]) / dz))
            assert span[0] + code * dz == z.value
            codes[k] = code
        L.turtle_map_destroy(C.byref(h))
        assert not codes[refused].any()
        out[f"{name}_values"], out[f"{name}_refused"], out[f"{name}_codes"] = v, refused, codes
        print(name, n, "values,", int(refused.sum()), "refused")
    path = os.path.join(OUT, "fill.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes;", hashlib.sha256(open(path, "rb").read()).hexdigest())


if __name__ == "__main__":
    main()
