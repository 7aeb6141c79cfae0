"""Inputs and the restatement of turtle_stepper_viewshed_n, shared by
tests/golden/generate_viewshed.py and the viewshed tests.

The geometries, observers, azimuths and distances are those of tests/horizon_cases.py (which see):
four cases, each 4 observers x 5 azimuths x 130 distances, so a line is two whole chunks of the
kernel's 64 samples and two samples of a third.  Two target heights: 0 (the ground itself) and
that of a mast.

restate() evaluates the definition of include/turtle_amd.h over the compiled reference;
follows() derives the flags from a profile of sines, which is how the expected viewshed at height
0 follows from tests/golden/horizon.npz without a run of the reference.
"""
from __future__ import annotations

import math

import numpy as np

import horizon_cases as HC

CASES = HC.CASES
LAYER = HC.LAYER
TARGET_HEIGHTS = (0.0, 10.0)
OUTPUTS = ("visible", "sine", "horizon", "n_visible")


def tag(height):
    """the fixture's name of a target height: h0, h10"""
    return "h%g" % height


def restate(stepper, position, azimuth, distance, layer, target_height):
    """turtle_stepper_viewshed_n as its header comment defines it, over the reference's stepper:
    dict(visible int8, sine, horizon [n][n_az][n_d]; n_visible int32 [n][n_az])"""
    from oracle import ref_ffi as R
    pos = np.asarray(position, dtype=np.float64).reshape(-1, 3)
    n, n_az, n_d = pos.shape[0], len(azimuth), len(distance)
    out = dict(visible=np.full((n, n_az, n_d), -2, dtype=np.int8), sine=np.full((n, n_az, n_d), -7.0),
               horizon=np.full((n, n_az, n_d), -7.0), n_visible=np.full((n, n_az), -2, dtype=np.int32))
    lat0, lon0, _ = R.ecef_to_geodetic(pos)

    def sine_of(point, p, up):
        d = [float(point[j]) - p[j] for j in range(3)]
        rr = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
        if rr <= HC.FLT_EPSILON:
            return None
        return (up[0] * d[0] + up[1] * d[1] + up[2] * d[2]) / math.sqrt(rr)

    for r in range(n):
        p = [float(v) for v in pos[r]]
        lam, phi = float(lon0[r]) * math.pi / 180.0, float(lat0[r]) * math.pi / 180.0
        sl, cl, sp, cp = math.sin(lam), math.cos(lam), math.sin(phi), math.cos(phi)
        up = (cl * cp, sl * cp, sp)                                      # [ref ecef.c:151-153]
        for a in range(n_az):
            h = [float(v) for v in R.ecef_from_horizontal(lat0[r:r + 1], lon0[r:r + 1], [azimuth[a]], [0.0])[0]]
            best, count = -math.inf, 0
            for k in range(n_d):
                s = float(distance[k])
                q = [p[j] + s * h[j] for j in range(3)]
                la, lo, _ = R.ecef_to_geodetic(q)
                rc, g, di = stepper.position(float(la[0]), float(lo[0]), 0.0, layer)
                assert rc == 0
                ground = target = None
                if di >= 0:
                    ground = sine_of(g, p, up)
                if ground is not None:
                    if target_height == 0.0:
                        target = ground
                    else:
                        rc, t, di = stepper.position(float(la[0]), float(lo[0]), float(target_height), layer)
                        assert rc == 0 and di >= 0
                        target = sine_of(t, p, up)
                out["horizon"][r, a, k] = best
                if target is None:
                    out["visible"][r, a, k], out["sine"][r, a, k] = -1, math.nan
                    continue
                out["sine"][r, a, k] = target
                v = 1 if target >= best else 0
                out["visible"][r, a, k] = v
                count += v
                if ground > best:
                    best = ground
            out["n_visible"][r, a] = count
    return out


def running_maximum(sine):
    """the exclusive running maximum along the last axis of a profile of GROUND sines: skipped and
    NaN samples count as -inf, and -inf stands in front of the first sample.  A maximum rounds
    nothing: these are the bits of the sequential loop."""
    s = np.where(np.isnan(sine), -np.inf, sine)
    inclusive = np.maximum.accumulate(s, axis=-1)
    return np.concatenate([np.full(s.shape[:-1] + (1,), -np.inf), inclusive[..., :-1]], -1)


def follows(target, horizon, skipped):
    """visible int8 and n_visible int32 from the target's sines, the horizon in front of each and
    the samples the definition skips"""
    with np.errstate(invalid="ignore"):
        visible = np.where(skipped, -1, target >= horizon).astype(np.int8)
    return visible, (visible == 1).sum(-1).astype(np.int32)


def margins(target, horizon, visible):
    """|target sine - horizon| of the samples with data and a finite horizon"""
    pick = (visible >= 0) & np.isfinite(horizon) & ~np.isnan(target)
    return np.abs(target[pick] - horizon[pick])
