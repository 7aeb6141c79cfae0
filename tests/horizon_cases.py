"""Geometries, inputs and the restatement of turtle_stepper_horizon_n, shared by
tests/golden/generate_horizon.py and the horizon tests.

The geometries are four of tests/normal_cases.py (which see), each with the layer whose top is
looked at:
  "map"           one geodetic map of 17 x 17 nodes, 1/8 degree apart: the one-map kernel;
  "stack"         2 x 2 tiles with the north-east one missing: the one-stack kernel -- lines cross
                  the seams and run over the missing tile;
  "lambert"       one projected map of 3.2 km a side: the generic kernel, most samples outside;
  "layers_geoid"  layer 1 of three: the map over the stack, then the stack where the map ends,
                  plus the geoid.
Per case 4 observers at heights 0, 2, 30 and 800 m above the layer's top (placed with the
reference's turtle_stepper_position; the one at height 0 is there for the sample at its own foot,
one of the others stands near a rim of the data), 5 azimuths and 130 distances: 0, then 129 in a
geometric progression from 500 m to 150 km, in whole millimetres.  130 makes lanes 0 and 1 of the
kernel's wave take a third sample and the others two.

restate() evaluates the definition of include/turtle_amd.h over the compiled reference.
"""
from __future__ import annotations

import math

import numpy as np

import normal_cases as NC

CASES = ("map", "stack", "lambert", "layers_geoid")
LAYER = {"map": 0, "stack": 0, "lambert": 0, "layers_geoid": 1}
HEIGHTS = (0.0, 2.0, 30.0, 800.0)
AZIMUTHS = (0.0, 72.5, 135.0, 210.0, 333.0)
SENTINEL = -7.0
FLT_EPSILON = float(np.finfo(np.float32).eps)

# where the observers stand: (latitude, longitude), or map coordinates for the projected case
SPOTS = {
    "map": ((0.1, 0.2), (-0.5, 0.6), (0.93, -0.4), (-0.3, -0.7)),             # the third: the northern rim
    "stack": ((0.5, 10.5), (0.9, 10.95), (1.5, 10.3), (0.08, 11.6)),         # seams, the hole, the southern rim
    "lambert": ((701600.0, 6601600.0), (700300.0, 6600400.0), (702900.0, 6602000.0), (701000.0, 6602800.0)),
    "layers_geoid": ((0.7, 11.0), (0.5, 10.2), (1.2, 11.45), (1.6, 10.6)),   # the third: where the map ends
}


def distances():
    """0, then 129 values from 500 m to 150 km in a geometric progression, in whole millimetres
    (so that the last ulp of a platform's pow() does not reach them)"""
    j = np.arange(129, dtype=np.float64)
    return np.concatenate([[0.0], np.rint(500e3 * 300.0 ** (j / 128.0)) / 1e3])


def azimuths():
    return np.array(AZIMUTHS)


def reference_stepper(geo):
    """the reference's stepper over a normal_cases.reference_geometry"""
    from oracle import ref_ffi as R
    st = R.RefStepper()
    if geo["geoid"] is not None:
        st.geoid_set(geo["geoid"])
    for layer in geo["layers"]:
        if len(geo["layers"]) > 1:
            st.add_layer()
        for kind, data, offset, _ in layer:
            if kind == NC.FLAT:
                st.add_flat(offset)
            elif kind == NC.MAP:
                st.add_map(data, offset)
            else:
                st.add_stack(data, offset)
    return st


def observers(case, stepper):
    """the case's observers [4][3], placed by the reference's turtle_stepper_position"""
    from oracle import ref_ffi as R
    spots = np.array(SPOTS[case])
    if case == "lambert":
        proj = R.RefProjection(NC.LAMBERT)
        lat, lon = proj.unproject(spots[:, 0], spots[:, 1])
        proj.destroy()
    else:
        lat, lon = spots[:, 0], spots[:, 1]
    pos = np.empty((len(HEIGHTS), 3))
    for r, height in enumerate(HEIGHTS):
        rc, pos[r], di = stepper.position(float(lat[r]), float(lon[r]), height, LAYER[case])
        assert rc == 0 and di >= 0, (case, r)
    return pos


def restate(stepper, position, azimuth, distance, layer, sentinel=SENTINEL):
    """turtle_stepper_horizon_n as its header comment defines it, over the reference's stepper:
    dict(elevation, sample, range [n][n_az]; sine, data_index [n][n_az][n_d]: the whole profile,
    NaN / -1 where a sample was skipped).  Lines without a sample keep `sentinel`."""
    from oracle import ref_ffi as R
    pos = np.asarray(position, dtype=np.float64).reshape(-1, 3)
    n, n_az, n_d = pos.shape[0], len(azimuth), len(distance)
    out = dict(elevation=np.full((n, n_az), sentinel), sample=np.zeros((n, n_az), dtype=np.int32),
               range=np.full((n, n_az), sentinel), sine=np.full((n, n_az, n_d), np.nan),
               data_index=np.full((n, n_az, n_d), -1, dtype=np.int8))
    lat0, lon0, _ = R.ecef_to_geodetic(pos)
    for r in range(n):
        p = [float(v) for v in pos[r]]
        lam, phi = float(lon0[r]) * math.pi / 180.0, float(lat0[r]) * math.pi / 180.0
        sl, cl, sp, cp = math.sin(lam), math.cos(lam), math.sin(phi), math.cos(phi)
        up = (cl * cp, sl * cp, sp)                                      # [ref ecef.c:151-153]
        for a in range(n_az):
            h = [float(v) for v in R.ecef_from_horizontal(lat0[r:r + 1], lon0[r:r + 1], [azimuth[a]], [0.0])[0]]
            best, best_k, best_range = -math.inf, 0, 0.0
            for k in range(n_d):
                s = float(distance[k])
                q = [p[j] + s * h[j] for j in range(3)]
                la, lo, _ = R.ecef_to_geodetic(q)
                rc, g, di = stepper.position(float(la[0]), float(lo[0]), 0.0, layer)
                assert rc == 0
                if di < 0:
                    continue
                d = [float(g[j]) - p[j] for j in range(3)]
                rr = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
                if rr <= FLT_EPSILON:
                    continue
                arg = (up[0] * d[0] + up[1] * d[1] + up[2] * d[2]) / math.sqrt(rr)
                out["sine"][r, a, k], out["data_index"][r, a, k] = arg, di
                if arg > best:
                    best, best_k, best_range = arg, k + 1, math.sqrt(rr)
            out["sample"][r, a] = best_k
            if best_k:
                out["elevation"][r, a] = 90.0 if best > 1.0 else -90.0 if best < -1.0 else \
                    math.asin(best) * 180.0 / math.pi
                out["range"][r, a] = best_range
    return out


def gaps(sine):
    """per line, the best sine minus the second best (inf with fewer than two samples)"""
    s = np.where(np.isnan(sine), -np.inf, sine)
    s = np.concatenate([np.full(s.shape[:-1] + (1,), -np.inf), s], -1)      # (a line of one sample)
    top = np.sort(s, axis=-1)[..., -2:]
    with np.errstate(invalid="ignore"):
        gap = top[..., 1] - top[..., 0]
    return np.where(np.isfinite(top[..., 0]), gap, np.inf)
