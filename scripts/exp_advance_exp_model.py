"""Experiment (CPU only): what turtle_stepper_advance_exp_n's model costs -- within a step the altitude
is taken as linear in the path, while along a straight line it bends away from linear by the
Earth's curvature.

The rays are the "ground" batch of tests/golden/traverse.npz over the hgt tile (1000 rays from the
ground, climbing to the batch's ceiling), air 1.205 kg/m^3 with a scale height of 8400 m.  For each
ray that stays in the air, the definition's depth to the end (tests/c/advance_exp_loop.c over the
oracle's restatement of turtle_stepper_step, uncut) is compared with a quadrature of
rho0 exp(-h(s) / H) along the true line: Simpson's rule at a spacing of at most SPACING metres, h from
the oracle's ecef_to_geodetic.  Next to the largest relative difference: the bound it should sit
under, ds^2 / (8 R H) for the ray's longest step ds (over a chord of length ds the altitude lies at
most ds^2 / (8 R) under the straight line between its ends), R = 6.371e6 m.

    python scripts/exp_advance_exp_model.py [out.txt]
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import ffi as O  # noqa: E402

import advance_exp_cases as AE  # noqa: E402
import traverse_cases as TC  # noqa: E402

SPACING = 5.0
R_EARTH = 6.371e6
CAPACITY = 100000

g = np.load(os.path.join(ROOT, "tests", "golden", "traverse.npz"))
k = "hgt_ground_"
pos, d, ceiling = g[k + "position"], g[k + "direction"], float(g[k + "ceiling"])
rho, sh = AE.DENSITY[2], AE.SCALE_HEIGHT[2]
rho0, H = float(rho[1]), float(sh[1])
n = pos.shape[0]
geo = TC.oracle_geometry("hgt")
full = AE.check(geo, pos, d, rho, sh, np.full(n, np.inf), None, ceiling)
air = (g[k + "length"][0] == 0) & (full["distance"] > 0)

profile = AE.checker().advance_exp_profile
profile.restype = C.c_int
path, alt, med = np.empty(CAPACITY + 1), np.empty(CAPACITY + 1), np.empty(CAPACITY, dtype=np.int32)
rel, bound, longest, top = [], [], [], []
for r in np.flatnonzero(air):
    steps = profile(geo.ref, C.c_double(0.4), C.c_double(1e-2), pos[r].ctypes.data_as(C.c_void_p),
                    d[r].ctypes.data_as(C.c_void_p), C.c_double(ceiling), CAPACITY,
                    path.ctypes.data_as(C.c_void_p), alt.ctypes.data_as(C.c_void_p), med.ctypes.data_as(C.c_void_p))
    assert steps == full["n_steps"][r] and path[steps] == full["distance"][r]
    T = float(path[steps])
    m = 2 * max(1, int(np.ceil(T / SPACING / 2)))              # (an even number of intervals)
    s = np.linspace(0.0, T, m + 1)
    h = O.ecef_to_geodetic(pos[r] + s[:, None] * d[r])[2]
    f = rho0 * np.exp(-h / H)
    true = (T / m) / 3.0 * (f[0] + f[-1] + 4.0 * f[1:-1:2].sum() + 2.0 * f[2:-1:2].sum())
    ds = float(np.diff(path[:steps + 1]).max())
    rel.append(abs(full["depth"][r] - true) / true)
    bound.append(ds * ds / (8.0 * R_EARTH * H))
    longest.append(ds)
    top.append(float(alt[steps]))
rel, bound, longest, top = (np.array(v) for v in (rel, bound, longest, top))
worst = int(np.argmax(rel))
lines = [
    f"hgt 'ground' batch: {int(air.sum())} of {n} rays stay in the air and move; ceiling {ceiling:.0f} m, "
    f"H {H:.0f} m, quadrature at <= {SPACING} m",
    f"steps a ray: median {int(np.median(full['n_steps'][air]))}, most {int(full['n_steps'][air].max())}; longest step "
    f"of a ray: median {np.median(longest):.1f} m, most {longest.max():.1f} m; end altitude up to {top.max():.0f} m",
    f"largest relative difference, definition against quadrature: {rel.max():.3e} "
    f"(its ray's longest step {longest[worst]:.1f} m, bound ds^2 / (8 R H) = {bound[worst]:.3e})",
    f"largest bound of any ray: {bound.max():.3e}; rays above their own bound: {int((rel > bound).sum())}; "
    f"median difference {np.median(rel):.3e}",
]
print("\n".join(lines))
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as fh:
        fh.write("\n".join(lines) + "\n")
