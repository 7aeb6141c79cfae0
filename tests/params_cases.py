"""Slope and resolution other than the defaults: the table of settings, the ray recipes and the
mask of ill-conditioned rays, shared by tests/golden/generate_params.py and the tests
(tests/test_oracle_golden.py, tests/test_oracle_vs_reference.py, tests/test_params_host.py,
tests/test_gpu_params.py).

The geometries are the 1201^2 tiles of traverse_cases ("hgt", "two", "rough") and a 2 x 2 stack of
1201^2 sin.cos tiles.  Which rays count is decided by the reference's arithmetic alone (the CPU
restatement, pinned to the reference bit for bit): ill_conditioned() retraces a batch from origins
moved by the closed form's noise and by the bisection's bracket, and sets apart every ray whose own
answer moves.  No GPU output enters it.
"""
from __future__ import annotations

import os

import numpy as np

from oracle import ffi as O
from turtle_amd import synth

import terrains as T
import traverse_cases as TC

DEFAULT = (0.4, 1e-2)
# name -> (slope, resolution)
SETTINGS = {
    "example": (1.0, 1e-2),     # the reference example's own setting
    "steep": (2.0, 1e-2),       # steps larger than the clearance (smooth ground only)
    "fine": (0.4, 1e-3),        # ten times as many minimum steps on a line
    "coarse": (0.4, 1.0),       # a minimum step of a metre
    "mixed": (1.0, 0.25),       # both moved at once
    "slow": (0.1, 1e-2),        # thousands of steps per ray
}
CASES = ("hgt", "rough")
RECIPES = ("ground", "c2", "graze")
RAYS = 1000
MAX_STEPS = 100000
BAR = 1e-6                      # BASELINE's bar on the path length
# lines of sight (traverse_n, crossings_n, advance_n, advance_exp_n): traverse_cases' geometries
SIGHT_CASES = ("hgt", "two")
SIGHT_SETTINGS = ("example", "fine", "coarse")
# traverse.npz's own "two" rays: at `example` and `fine` the mask exceeds its cap
SHALLOW_SETTINGS = ("coarse",)

# the perturbations of ill_conditioned(): metres along each of two seeded random unit vectors
TAU0 = 2e-9                     # kLineTau0, the closed form's noise
BRACKET = 1e-8                  # the bisection's bracket
MASK_SEED = 0x3A5C
MASK_REL = 1e-7


def settings(case):
    """the settings a geometry is run at: `steep` tunnels through the rough tile's slivers for 5 %
    of the C2 rays by the reference alone, and is not run there"""
    return tuple(s for s in SETTINGS if not (case == "rough" and s == "steep"))


def cap(case, setting):
    """the largest share of a batch that may be masked"""
    return 0.05 if case == "rough" and setting in ("example", "mixed") else 0.005


# "ground" is generate_traverse.py's recipe (azimuth U[0, 360), elevation U[0, 30] degrees, from 0.5 m
# above the ground), but on the rough tile from 2 m up: from 0.5 m, 7 to 9 rays of the 1000 end in
# rock within 0.2 m, where moving an origin by the bracket's 1e-8 m is itself more than 1e-7 of the
# path, and the reference alone exceeds the cap of the mask (at `fine` and `coarse`; 1 ray from 2 m)
GROUND_HEIGHT = {"hgt": 0.5, "rough": 2.0}


def draws(case, recipe, n=RAYS):
    """(lat, lon, height, az, el) of "ground" and of "graze": from 30 m above the ground in the
    middle of the tile, elevation -3 .. 1 degrees.  ("c2" is generate_traverse.py's, special rays
    and all.)"""
    if recipe == "ground":
        lat, lon, az, el = synth.uniform_rays(n, (TC.LAT0, TC.LAT0 + 1), (TC.LON0, TC.LON0 + 1), seed=0x7A5E,
                                              el_range=(0.0, 30.0))
        return lat, lon, np.full(n, GROUND_HEIGHT[case]), az, el
    assert recipe == "graze"
    lat, lon, az, el = synth.uniform_rays(n, (45.2, 45.8), (3.2, 3.8), seed=11, el_range=(-3, 1))
    return lat, lon, np.full(n, 30.0), az, el


def sight_rays(case, recipe, traverse, shallow=False):
    """(position, direction, ceiling) of a line-of-sight batch; `traverse` is traverse.npz.  "hgt":
    the fixture's own rays, and with `shallow` those of "two" as well (run at SHALLOW_SETTINGS, where
    the mask stays under its cap: shallow climbing rays over flat layers, crossings included).  "two":
    the same recipes with the elevations kept off the horizontal ("ground" 4 .. 30 degrees, "c2"
    -10 .. -4), by the restatement's transforms: a ray that climbs
    to the 2000 m ceiling over flat layers at less than 3.6 degrees takes steps of slope x its
    height, from a height of 1e-8 m where a crossing left it, so that the overshoot of its last step
    -- up to 1e-6 of its path -- depends on the origin's last digits, and by the reference alone 2.4
    to 13.5 % of the fixture's "two" rays are ill-conditioned at `example` and `fine`."""
    k = f"{case}_{recipe}_"
    if case != "two" or shallow:
        return traverse[k + "position"], traverse[k + "direction"], float(traverse[k + "ceiling"])
    box = (TC.LAT0, TC.LAT0 + 1), (TC.LON0, TC.LON0 + 1)
    if recipe == "ground":
        lat, lon, az, el = synth.uniform_rays(RAYS, *box, seed=0x7A5E, el_range=(4.0, 30.0))
        height = 0.5
    else:
        lat, lon, az, el = synth.uniform_rays(RAYS, *box, seed=0x5EED2026, el_range=(-10.0, -4.0))
        height = 500.0
    pos, di = TC.oracle_geometry("two").position(lat, lon, height, layer=1)
    assert (di >= 0).all()
    return pos, O.ecef_from_horizontal(lat, lon, az, el), 2000.0


# ---- the generic step machine: composite_cases' "layers" ---------------------
GENERIC_CASE = "layers"
GENERIC_SETTINGS = ("example", "coarse")


def generic_sight():
    """(position, direction): composite_cases.sight("layers") without the rays within 4 degrees of the
    horizontal -- the layers end in flats, and those rays climb to the ceiling as the shallow rays of
    "two" do (sight_rays): at `example` 83 of the 2000 are ill-conditioned by the reference alone"""
    import composite_cases as CO
    pos, d = CO.sight(GENERIC_CASE)
    lat, lon, _ = O.ecef_to_geodetic(pos)
    _, el = O.ecef_to_horizontal(lat, lon, d)
    keep = np.abs(el) >= 4.0
    return np.ascontiguousarray(pos[keep]), np.ascontiguousarray(d[keep])


# ---- the 2 x 2 stack --------------------------------------------------------
STACK_TILES = [(45, 3), (45, 4), (46, 3), (46, 4)]
STACK_RAYS = 2000


def stack_oracle():
    return T.mosaic_oracle(STACK_TILES, TC.N, 45, 3, 2, 2)


def stack_rays(n=STACK_RAYS, seed=0x57AC):
    """fresh seeded rays over the stack, by the oracle: half of them BASELINE's C2 shape (500 m up,
    elevation -10 .. -1 degrees), half shallow from 30 m up (thousands of steps, across the seams)"""
    geo = stack_oracle()
    h = n // 2
    lat, lon, az, el = synth.uniform_rays(h, (45.05, 46.95), (3.05, 4.95), seed=seed)
    lat2, lon2, az2, el2 = synth.uniform_rays(n - h, (45.3, 46.7), (3.3, 4.7), seed=seed + 1, el_range=(-3, 1))
    lat, lon, az, el = (np.concatenate(v) for v in ((lat, lat2), (lon, lon2), (az, az2), (el, el2)))
    height = np.concatenate([np.full(h, 500.0), np.full(n - h, 30.0)])
    pos, di = geo.position(lat, lon, height)
    assert (di == 0).all()
    return pos, O.ecef_from_horizontal(lat, lon, az, el)


# ---- which rays count --------------------------------------------------------

def offsets(seed=MASK_SEED):
    """the origin offsets of the retraces [8][3]: +-TAU0 and +-BRACKET along two seeded unit vectors"""
    u = np.random.default_rng(seed).normal(size=(2, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    return np.array([sign * size * v for size in (TAU0, BRACKET) for v in u for sign in (1.0, -1.0)])


# The rays outside the bar, by name: test_gpu_params.trace_bar's tag -> rays.  A ray may be named only
# if the WIDER reference-only set flags it and the mask's own does not: the origin moved by +-1e-7 m
# along eight seeded unit vectors (wider_offsets(); tests/test_params_host.py checks each name).
# "trace rough mixed fast" 1639 ("c2" 639): at slope 1 over the rough tile the reference itself
# answers 87 steps and 38 636.5 m, or 97 to 99 steps and 39 024.6 m, by which way the origin moved
# by 1e-7 m; FAST takes 96 steps to 39 024.6 m, the same medium and data.
OUTSIDE = {
    "trace rough mixed fast": [1639],
}
WIDER = 1e-7


def wider_offsets(seed=MASK_SEED + 1):
    u = np.random.default_rng(seed).normal(size=(8, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    return np.array([sign * WIDER * v for v in u for sign in (1.0, -1.0)])


def ill_conditioned(run, position, shifts=None):
    """The mask.  run(position) -> dict(index [n][2], n_steps [n], length [n] or [media][n]) is the
    CPU restatement's loop over a batch's origins (the directions and settings are run's own).  A
    ray is ill-conditioned if, with every origin moved by one of `shifts` (default: offsets()), its
    index or step count changes or a length moves by more than MASK_REL of its total path."""
    pos = np.asarray(position, dtype=np.float64)
    base = run(pos)
    total = np.atleast_2d(base["length"]).sum(axis=0)
    scale = MASK_REL * np.maximum(np.abs(total), 1e-300)
    bad = np.zeros(pos.shape[0], dtype=bool)
    with np.errstate(invalid="ignore"):
        for shift in (offsets() if shifts is None else shifts):
            t = run(pos + shift)
            bad |= (t["index"] != base["index"]).any(axis=1) | (t["n_steps"] != base["n_steps"])
            moved = np.abs(np.atleast_2d(t["length"]) - np.atleast_2d(base["length"])).max(axis=0)
            bad |= ~(moved <= scale)
    return bad, base


def trace_run(geo, direction, slope, resolution, max_steps=MAX_STEPS, threads=None):
    threads = threads or min(16, os.cpu_count() or 1)
    return lambda pos: geo.trace(pos, direction, max_steps=max_steps, slope=slope, resolution=resolution,
                                 threads=threads)


def traverse_run(geo, direction, ceiling, slope, resolution, max_steps=1000000, threads=None):
    threads = threads or min(16, os.cpu_count() or 1)
    return lambda pos: TC.check(geo, pos, direction, ceiling, max_steps=max_steps, threads=threads, slope=slope,
                                resolution=resolution)


_masks = {}


def trace_mask(key, geo, position, direction, slope, resolution):
    """ill_conditioned() of a trace and the unmoved trace itself, kept by `key` for the session"""
    if key not in _masks:
        _masks[key] = ill_conditioned(trace_run(geo, direction, slope, resolution), position)
    return _masks[key]


def traverse_mask(key, geo, position, direction, ceiling, slope, resolution, max_steps=1000000):
    """the same of a line of sight through every medium (traverse_cases.check): the lengths are per
    medium, and each must stay within MASK_REL of the ray's total path"""
    if key not in _masks:
        _masks[key] = ill_conditioned(traverse_run(geo, direction, ceiling, slope, resolution, max_steps),
                                      position)
    return _masks[key]


# ---- edges: settings no harness should make --------------------------------------------------
EDGES = {
    "a step longer than a line": (0.4, 5000.0),      # resolution 5000 m > kLineRange
    "slope 50": (50.0, 1e-2),
    "no step at all": (0.0, 0.0),                    # every live ray ends at the cap with length 0
    "slope 1e-6": (1e-6, 1e-2),
    "resolution below the bracket": (0.4, 1e-9),     # the bisection's bracket is 1e-8 m
}
EDGE_MAX_STEPS = 600


def edge_batches():
    """[(position, direction)]: test_degenerate_inputs' 12 rays (NaN and infinite coordinates, the
    centre of the Earth, a pole, 10^9 m away; zero, NaN, non-unit and reversed directions) and a
    ragged batch of 65 seeded rays, over terrains.c1_oracle()"""
    geo = T.c1_oracle()
    n = 12
    lat, lon = np.full(n, 45.5), np.full(n, 3.5)
    pos, _ = geo.position(lat, lon, 500.0)
    d = O.ecef_from_horizontal(lat, lon, np.full(n, 30.0), np.full(n, -5.0))
    pos[1, 0] = np.nan
    pos[2, 1] = np.inf
    pos[3] = 0.0
    pos[4] = (0.0, 0.0, 6.4e6)
    pos[5] = (1e9, 1e9, 1e9)
    pos[10] = (0.0, 0.0, -6.4e6)
    d[6] = 0.0
    d[7, 2] = np.nan
    d[8] *= 1e6
    d[9] *= -1.0
    lat, lon, az, el = synth.uniform_rays(65, T.C1_Y, T.C1_X, seed=5)
    p65, _ = geo.position(lat, lon, 300.0)
    return [(pos, d), (p65, O.ecef_from_horizontal(lat, lon, az, el))]
