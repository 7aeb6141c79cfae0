"""Inputs and the restatement of turtle_stepper_clearance_n, shared by
tests/golden/generate_clearance.py and the clearance tests.

The geometries, layers and the 4 observers are those of tests/horizon_cases.py (which see).  Per
case 6 targets: five placed by the reference's turtle_stepper_position at heights from 0 to 4 km
above the layer's top, and one that stands where the layer has NO data (beyond a rim of the map,
over the stack's missing tile, outside the Lambert map), which turtle_stepper_position cannot
place: that one is turtle_ecef_from_geodetic of an altitude.  Lines to it lose their last samples,
and lines across the hole or the rims lose others.  The low targets behind rough ground are clearly
blocked, the high ones clearly open.

130 fractions (2k + 1) / 260: interior, so no sample sits on an end point, where the clearance is
the end point's own height above the ground it was placed on, rounding noise for a height of 0;
130 makes lanes 0 and 1 of the kernel's wave take a third sample and the others two.

restate() evaluates the definition of include/turtle_amd.h over the compiled reference.
"""
from __future__ import annotations

import math

import numpy as np

import horizon_cases as HC
import normal_cases as NC

CASES = HC.CASES
LAYER = HC.LAYER
SENTINEL = HC.SENTINEL
N_FRACTIONS = 130
OUTPUTS = ("clearance", "sample", "n_data")
NUDGE = 4                       # ulp: no sample's data index may hang on less (see data_is_robust)

# where the targets stand: (latitude, longitude, height above the layer's top) -- map coordinates
# for the projected case -- and, last, the one over missing data: (.., .., ALTITUDE)
TARGETS = {
    "map": ((0.6, 0.5, 0.0), (-0.2, -0.3, 40.0), (0.4, -0.6, 1500.0), (-0.7, 0.3, 4000.0), (0.05, 0.15, 300.0),
            (1.4, 0.2, 2500.0)),                                           # beyond the northern rim
    "stack": ((0.3, 10.4, 0.0), (0.6, 11.5, 50.0), (1.6, 10.7, 1500.0), (0.2, 11.8, 4000.0), (1.2, 10.2, 300.0),
              (1.5, 11.5, 2500.0)),                                        # over the missing tile
    "lambert": ((700800.0, 6600900.0, 0.0), (702500.0, 6602500.0, 20.0), (701200.0, 6601000.0, 500.0),
                (702000.0, 6600600.0, 3000.0), (700500.0, 6602900.0, 100.0),
                (705000.0, 6604000.0, 1800.0)),                            # outside the map
    "layers_geoid": ((0.8, 11.2, 0.0), (0.4, 10.3, 50.0), (1.5, 10.4, 1500.0), (0.3, 11.7, 4000.0),
                     (1.0, 10.8, 300.0),
                     (1.7, 11.7, 2500.0)),                                 # past the map, over the missing tile
}


def fractions(n=N_FRACTIONS):
    """(2k + 1) / (2n): one division each, the same bits on any platform"""
    return (2.0 * np.arange(n, dtype=np.float64) + 1.0) / (2.0 * n)


def targets(case, stepper):
    """the case's targets [6][3]: five placed by the reference's turtle_stepper_position, the last
    (no data under it) by turtle_ecef_from_geodetic"""
    from oracle import ref_ffi as R
    spots = np.array(TARGETS[case])
    if case == "lambert":
        proj = R.RefProjection(NC.LAMBERT)
        lat, lon = proj.unproject(spots[:, 0], spots[:, 1])
        proj.destroy()
    else:
        lat, lon = spots[:, 0], spots[:, 1]
    pos = np.empty((len(spots), 3))
    for t in range(len(spots) - 1):
        rc, pos[t], di = stepper.position(float(lat[t]), float(lon[t]), float(spots[t, 2]), LAYER[case])
        assert rc == 0 and di >= 0, (case, t)
    rc, _, di = stepper.position(float(lat[-1]), float(lon[-1]), 0.0, LAYER[case])
    assert rc == 0 and di < 0, (case, "the last target is meant to stand over missing data")
    pos[-1] = R.ecef_from_geodetic(lat[-1:], lon[-1:], spots[-1:, 2])[0]
    return pos


def restate(stepper, observer, target, fraction, layer, paired=False, sentinel=SENTINEL):
    """turtle_stepper_clearance_n as its header comment defines it, over the reference's stepper:
    dict(clearance, sample, n_data [n][m] (or [n]); profile, data_index, latitude, longitude
    [n][m][K] (or [n][K]): every sample's clearance (NaN where it was skipped), data index (-1
    there) and the geodetic coordinates the reference was asked at).  Lines without a sample keep
    `sentinel`."""
    from oracle import ref_ffi as R
    obs = np.asarray(observer, dtype=np.float64).reshape(-1, 3)
    tgt = np.asarray(target, dtype=np.float64).reshape(-1, 3)
    n, m, n_f = obs.shape[0], tgt.shape[0], len(fraction)
    assert (not paired) or (m == n)
    shape = (n,) if paired else (n, m)
    out = dict(clearance=np.full(shape, sentinel), sample=np.zeros(shape, dtype=np.int32),
               n_data=np.zeros(shape, dtype=np.int32), profile=np.full(shape + (n_f,), np.nan),
               data_index=np.full(shape + (n_f,), -1, dtype=np.int8),
               latitude=np.zeros(shape + (n_f,)), longitude=np.zeros(shape + (n_f,)))
    for r in range(n):
        p = [float(v) for v in obs[r]]
        for t in ([r] if paired else range(m)):
            i = (r,) if paired else (r, t)
            d = [float(tgt[t, j]) - p[j] for j in range(3)]
            best, best_k, count = math.inf, 0, 0
            for k in range(n_f):
                f = float(fraction[k])
                q = [p[j] + f * d[j] for j in range(3)]
                la, lo, _ = R.ecef_to_geodetic(q)
                la, lo = float(la[0]), float(lo[0])
                out["latitude"][i + (k,)], out["longitude"][i + (k,)] = la, lo
                rc, g, di = stepper.position(la, lo, 0.0, layer)
                assert rc == 0
                if di < 0:
                    continue
                count += 1
                lam, phi = lo * math.pi / 180.0, la * math.pi / 180.0
                sl, cl, sp, cp = math.sin(lam), math.cos(lam), math.sin(phi), math.cos(phi)
                up = (cl * cp, sl * cp, sp)                                  # [ref ecef.c:151-153]
                c = up[0] * (q[0] - float(g[0])) + up[1] * (q[1] - float(g[1])) + up[2] * (q[2] - float(g[2]))
                out["profile"][i + (k,)], out["data_index"][i + (k,)] = c, di
                if c < best:
                    best, best_k = c, k + 1
            out["sample"][i], out["n_data"][i] = best_k, count
            if best_k:
                out["clearance"][i] = best
    return out


def expected(profile, data_index, sentinel=SENTINEL):
    """the outputs that follow from a profile: the minimum (NaN: skipped), the first of equals"""
    filled = np.where(np.isnan(profile), np.inf, profile)
    low = filled.min(-1)
    sample = np.where(np.isinf(low), 0, filled.argmin(-1) + 1).astype(np.int32)
    return dict(clearance=np.where(sample == 0, sentinel, low), sample=sample,
                n_data=(data_index >= 0).sum(-1).astype(np.int32))


def gaps(profile):
    """per line, the second lowest clearance minus the lowest (inf with fewer than two samples)"""
    s = np.where(np.isnan(profile), np.inf, profile)
    s = np.concatenate([s, np.full(s.shape[:-1] + (1,), np.inf)], -1)       # (a line of one sample)
    low = np.sort(s, axis=-1)[..., :2]
    with np.errstate(invalid="ignore"):
        gap = low[..., 1] - low[..., 0]
    return np.where(np.isfinite(low[..., 1]), gap, np.inf)


def data_is_robust(stepper, latitude, longitude, data_index, layer, ulps=NUDGE):
    """n_data is compared exactly, which is fair only if no sample's data index hangs on an ulp:
    the reference asked again at each sample's latitude and longitude moved by +-`ulps` ulp, each
    alone and both together (8 neighbours) -> the number of samples whose data index changes"""
    def moved(x, steps):
        for _ in range(abs(steps)):
            x = np.nextafter(x, np.inf if steps > 0 else -np.inf)
        return x

    la, lo, di = latitude.ravel(), longitude.ravel(), data_index.ravel()
    changed = np.zeros(la.size, dtype=bool)
    for a in (-ulps, 0, ulps):
        for b in (-ulps, 0, ulps):
            if a == 0 and b == 0:
                continue
            la2, lo2 = moved(la, a), moved(lo, b)
            for j in range(la.size):
                rc, _, dj = stepper.position(float(la2[j]), float(lo2[j]), 0.0, layer)
                assert rc == 0
                changed[j] |= (dj != di[j])
    return int(changed.sum())
