"""Rough and void ground: the geometries and ray recipes shared by tests/golden/generate_rough.py
and the tests (tests/test_oracle_golden.py, tests/test_gpu_rough.py).

Tiles at (45N, 3E): "rough", synth.rough_nodes(1201, 1, 800) -- 800 m of value noise and 200 m of
per-node noise, so that a line of sight meets brackets with several crossings in them; "void", the
same tile with HGT voids (-32768 m, which the reference reads as an elevation): a 40 x 60 block
inside the tile, a one-node-wide row of 200 nodes (a trench one cell wide on either side), a
single node and a block on the tile's south-east corner.  nodes("rough", 3601): the full-size
rough tile (FULL_NOISE).
STACK: a 2 x 2 stack over (45..47N, 3..5E) of rough tiles with different seeds (the seams are
cliffs), one of them with voids and one missing.

Every origin and direction comes from a recipe: the reference's (and the oracle's, which is pinned
to it bit for bit) turtle_stepper_position and turtle_ecef_from_horizontal of seeded draws.
"""
from __future__ import annotations

import hashlib

import numpy as np

from oracle import ffi as O
from turtle_amd import synth

LAT0, LON0, N = 45, 3, 1201
SEED, AMPLITUDE = 1, 800
CASES = ("rough", "void")
# (row0, row1, col0, col1), half-open, rows south -> north
VOID_BLOCKS = ((400, 440, 500, 560),     # a block inside the tile
               (800, 801, 300, 500),     # one row: a trench
               (600, 601, 900, 901),     # a single node
               (0, 30, 1160, 1201))      # a block on the rim (south-east corner)
RAYS = 10000
EDGE_RAYS = 1000                         # a void block, aimed at its edge from outside
RECIPES = ("c2", "ground")
# the 2 x 2 stack: (lat, lon) -> (seed, voids); (46, 4) is missing
STACK_TILES = {(45, 3): (1, False), (45, 4): (2, True), (46, 3): (3, False)}
STACK_BOX = ((45.0, 47.0), (3.0, 5.0))


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# the full-size tile (3601^2 nodes, 31 m apart): per-node noise of +-67 m, the rough tile's slopes.
# With the +-200 m of the 1201^2 tile there, slopes of 13 make the stepping chaotic: a step is 0.4 x
# the clearance, so an ulp of a sample grows by up to 0.4 x 13 a step, and the reference's own result
# moves beyond the bar for 7 % of C2's rays when an origin moves by an ulp (0 of 10^5 at +-67 m)
FULL_N, FULL_NOISE = 3601, 67


def nodes(case, n=N):
    if n == FULL_N:
        return synth.rough_nodes(FULL_N, SEED, AMPLITUDE, FULL_NOISE)
    z = synth.rough_nodes(n, SEED, AMPLITUDE)
    return synth.with_voids(z, VOID_BLOCKS) if case == "void" else z


def write_tile(directory, case, n=N):
    """the case's tile as an .hgt file in `directory`"""
    return synth.write_nodes_hgt(str(directory), LAT0, LON0, nodes(case, n))


def oracle_geometry(case, n=N):
    return O.OracleGeometry(grids=[O.hgt_grid(LAT0, LON0, nodes(case, n))], layers=[[(O.MAP, 0, 0.0)]])


def ray_draws(recipe, n=RAYS, box=((LAT0, LAT0 + 1), (LON0, LON0 + 1))):
    """(lat, lon, height, az, el) of a recipe: "c2" is BASELINE's C2 (500 m above the ground,
    elevation -10 .. -1 degrees), "ground" starts 0.5 m above the ground, elevation -30 .. 30"""
    if recipe == "c2":
        lat, lon, az, el = synth.uniform_rays(n, box[0], box[1], seed=0x5EED2026)
        return lat, lon, np.full(n, 500.0), az, el
    lat, lon, az, el = synth.uniform_rays(n, box[0], box[1], seed=0x6A0D, el_range=(-30.0, 30.0))
    return lat, lon, np.full(n, 0.5), az, el


def edge_draws(block, n=EDGE_RAYS, seed=0xED6E):
    """Rays aimed from outside a void block at its edge: a target node on the block's rim (the
    side facing the tile's interior for a block on the rim), an origin 100 m .. 3 km away from it
    on the outward side, 0.5 .. 600 m above the ground, azimuth at the target within +-20 degrees
    and elevation -25 .. +2 degrees"""
    r0, r1, c0, c1 = block
    rng = np.random.default_rng([seed, r0, c0])
    side = rng.integers(0, 4, n)      # 0 south, 1 north, 2 west, 3 east
    if c1 >= N:                       # a rim block: never from beyond the tile
        side = np.where(side == 3, 2, side)
    if r0 == 0:
        side = np.where(side == 0, 1, side)
    u = rng.random(n)
    row = np.where(side == 0, r0 - 1, np.where(side == 1, r1, r0 + u * (r1 - 1 - r0)))
    col = np.where(side == 2, c0 - 1, np.where(side == 3, c1, c0 + u * (c1 - 1 - c0)))
    step = 1.0 / (N - 1)
    tlat, tlon = LAT0 + row * step, LON0 + col * step
    # the azimuth from the origin to the target (clockwise from north), the side's outward normal
    inward = np.choose(side, [0.0, 180.0, 90.0, 270.0])
    az = (inward + rng.uniform(-20.0, 20.0, n)) % 360.0
    dist = rng.uniform(100.0, 3000.0, n)
    back = np.radians(az + 180.0)
    lat = tlat + np.degrees(dist * np.cos(back) / 6.371e6)
    lon = tlon + np.degrees(dist * np.sin(back) / (6.371e6 * np.cos(np.radians(tlat))))
    lat = np.clip(lat, LAT0 + 1e-4, LAT0 + 1 - 1e-4)
    lon = np.clip(lon, LON0 + 1e-4, LON0 + 1 - 1e-4)
    height = rng.uniform(0.5, 600.0, n)
    el = rng.uniform(-25.0, 2.0, n)
    return lat, lon, height, az, el


def rays(case, recipe, position, ecef_from_horizontal, n=RAYS):
    """origins and directions of a recipe ("c2", "ground", "edge<k>" for VOID_BLOCKS[k]), computed
    by `position(lat, lon, height) -> (pos, data index)` and `ecef_from_horizontal` -- the
    reference's, the oracle's or the library's"""
    if recipe.startswith("edge"):
        lat, lon, h, az, el = edge_draws(VOID_BLOCKS[int(recipe[4:])])
    else:
        lat, lon, h, az, el = ray_draws(recipe, n)
    pos, di = position(lat, lon, h)
    assert (np.asarray(di) >= 0).all()
    return np.ascontiguousarray(pos), np.ascontiguousarray(ecef_from_horizontal(lat, lon, az, el))


def recipes(case):
    extra = tuple(f"edge{k}" for k in range(len(VOID_BLOCKS))) if case == "void" else ()
    return RECIPES + extra


def oracle_rays(case, recipe, n=RAYS):
    geo = oracle_geometry(case)
    return rays(case, recipe, geo.position, O.ecef_from_horizontal, n)


# ---- per-step records: the first STEP_RAYS rays of "ground", STEPS steps each ----
STEP_RAYS, STEPS = 2000, 32

def oracle_step_records(geo, pos, d):
    """the per-step records of generate_rough.py, replayed with the oracle: (ds, index, position)
    [ray, step], ds = NaN and index = -2 once the ray has left the data"""
    n = pos.shape[0]
    ds = np.full((n, STEPS), np.nan)
    index = np.full((n, STEPS, 2), -2, dtype=np.int32)
    position = np.full((n, STEPS, 3), np.nan)
    p = np.array(pos, dtype=np.float64)
    live = geo.step(p)["index"][:, 0] >= 0
    for k in range(STEPS):
        rays_ = np.flatnonzero(live)
        o = geo.step(p[rays_], d[rays_])
        p[rays_] = o["position"]
        ds[rays_, k], index[rays_, k], position[rays_, k] = o["step"], o["index"], o["position"]
        live[rays_] = o["index"][:, 0] >= 0
    return ds, index, position


# ---- deep points for ECEF -> geodetic: -40 .. -25 km, every latitude ----
def deep_points(n=2000, seed=0xDEE9):
    rng = np.random.default_rng(seed)
    lat = rng.uniform(-89.9, 89.9, n)
    lat[:8] = (-89.999, -60.0, -30.0, -1e-3, 1e-3, 30.0, 60.0, 89.999)
    return lat, rng.uniform(-180.0, 180.0, n), rng.uniform(-40e3, -25e3, n)


def deep_transforms(ecef_from_geodetic, ecef_to_geodetic):
    """the deep points to ECEF and back (the reference's or the oracle's transforms): (ecef,
    [lat, lon, alt])"""
    e = np.ascontiguousarray(ecef_from_geodetic(*deep_points()))
    return e, np.stack(ecef_to_geodetic(e))


# ---- the 2 x 2 stack ----
def stack_nodes(n=N):
    out = {}
    for (la, lo), (seed, voids) in STACK_TILES.items():
        z = synth.rough_nodes(n, seed, AMPLITUDE)
        out[(la, lo)] = synth.with_voids(z, VOID_BLOCKS) if voids else z
    return out


def write_stack(directory, n=N):
    for (la, lo), z in stack_nodes(n).items():
        synth.write_nodes_hgt(str(directory), la, lo, z)
    return str(directory)
