"""Composite geometries -- a stack beside maps and flats in one layer, overlapping maps, layers
without data, a geoid -- with their rays and the three ways to build them, shared by
tests/golden/generate_composite.py and the tests (tests/test_oracle_golden.py,
tests/test_composite_host.py, tests/test_gpu_composite.py).

Every one of them is TAMD_MODE_GENERIC for tamd_stepper_flatten (turtle_amd/csrc/stepper.c): the
instances of the stepping kernels that a caller of the reference's own example geometry runs
[ref examples/example-stepper.c:100-110].  The cases, each the smallest that still forks the code
(the data of a layer in the order ADDED: the reference consults the last added first
[ref stepper.c:722-724] and skips a layer that has no data at a point [ref stepper.c:719-744]):

  "example"  geoid; [flat 0, the 2 x 2 .asc stack of normal_cases (north-east tile missing), a
             UTM 32N map of 33 x 33 nodes, 40 km a side, inside tile (0N, 11E)]; [flat 3000]
  "layers"   geoid; [flat 0]; [the stack, normal_cases' geodetic map of 17 x 17 nodes over it];
             [flat 3000].  Layer 1 has no data over the missing tile outside the map
  "overlap"  no geoid; [map A 17 x 17 over 1 degree, map B 33 x 33 over 0.5 degree at +20 m];
             [map C 17 x 17 over 0.4 degree at +150 m, no data elsewhere]; [flat 3000]
  "offsets"  geoid; [flat 0, the stack at -35.5, the UTM map at +12.25]; [the same stack at +400:
             one data object in two layers]; [flat 3000]

A layer of flats never ends, so every geometry is closed by a flat at 3000 m; "example_open" (not
in CASES) is "example" without that lid (tests/test_gpu_composite.py::test_a_flat_world_has_no_end).

The geoid is synthetic, 361 x 181 nodes over (0..360, -90..90) made of integers only (the same on
any platform): two triangle waves, within +-34 m.
"""
from __future__ import annotations

import os

import numpy as np

from oracle import ffi as O

import irregular_cases as IC
import normal_cases as NC

CASES = ("example", "layers", "overlap", "offsets")
FLAT, MAP, STACK = "flat", "map", "stack"
LID = 3000.0
GEOID_X, GEOID_Y, GEOID_Z = (0.0, 360.0), (-90.0, 90.0), (-40.0, 40.0)
UTM, UTM_X, UTM_Y, UTM_Z, UTM_N = "UTM 32N", (758000.0, 798000.0), (35000.0, 75000.0), (0.0, 2000.0), 33
STACK_LAT0, STACK_LON0, STACK_N = 0.0, 10.0, 2

# name -> (nodes, x, y, z, projection)
MAPS = {
    "utm": (lambda: NC.rough(UTM_N, UTM_N, 5), UTM_X, UTM_Y, UTM_Z, UTM),
    "top": (NC.top_nodes, NC.TOP_X, NC.TOP_Y, NC.TOP_Z, None),
    # (low ground, 25 .. 100 m: the rays that start 30 m above the ellipsoid graze it)
    "A": (lambda: np.rint(NC.rough(17, 17, 6) / 16.0), (10.0, 11.0), (0.0, 1.0), (0.0, 200.0), None),
    "B": (lambda: np.rint(NC.rough(33, 33, 7) / 16.0), (10.3, 10.8), (0.2, 0.7), (0.0, 200.0), None),
    "C": (lambda: np.rint(NC.rough(17, 17, 8) / 16.0), (10.35, 10.75), (0.4, 0.8), (0.0, 200.0), None),
}

# case -> (geoid?, layers bottom -> top of (kind, name, offset) in the order ADDED)
RECIPES = {
    "example": (True, [[(FLAT, None, 0.0), (STACK, None, 0.0), (MAP, "utm", 0.0)], [(FLAT, None, LID)]]),
    "layers": (True, [[(FLAT, None, 0.0)], [(STACK, None, 0.0), (MAP, "top", 0.0)], [(FLAT, None, LID)]]),
    "overlap": (False, [[(MAP, "A", 0.0), (MAP, "B", 20.0)], [(MAP, "C", 150.0)], [(FLAT, None, LID)]]),
    "offsets": (True, [[(FLAT, None, 0.0), (STACK, None, -35.5), (MAP, "utm", 12.25)],
                       [(STACK, None, 400.0)], [(FLAT, None, LID)]]),
}
RECIPES["example_open"] = (True, RECIPES["example"][1][:-1])
# ((south, north), (west, east)) the rays start over
BOXES = {"example": ((0.0, 2.0), (10.0, 12.0)), "layers": ((0.0, 2.0), (10.0, 12.0)),
         "overlap": ((0.0, 1.0), (10.0, 11.0)), "offsets": ((0.0, 2.0), (10.0, 12.0)),
         "example_open": ((0.0, 2.0), (10.0, 12.0))}

COMPOSITE_LAYER = {"example": 0, "layers": 1, "overlap": 0, "offsets": 0}
GRAZE, UNDER, SIGHT, GOLDEN_RAYS, RIM_POINTS = 1500, 750, 2000, 500, 1000
# "example_open": 300 of graze's rays, 3000 steps at most.  Rays 17 and 75 overflow between 2800
# and 3200 steps in the restatement -- finite or not by where the cap falls -- and are left out
OPEN_RAYS, OPEN_MAX_STEPS, OPEN_LEFT_OUT = 300, 3000, (17, 75)
GRAZE_MAX_STEPS, SIGHT_MAX_STEPS, CEILING = 100000, 20000, 5000.0
WALK_RAYS, WALK_GENERATIONS = 512, 48

sha = IC.sha


def recipe(case):
    return RECIPES[case]


def geoid_nodes():
    """[181][361] metres: two triangle waves of whole eighths of a metre"""
    iy, ix = np.meshgrid(np.arange(181), np.arange(361), indexing="ij")
    return (np.abs((ix * 4) % 360 - 180) - 90) / 4.0 + (np.abs((iy * 6) % 360 - 180) - 90) / 8.0


def tile_nodes():
    """{(iy, ix): z} of the stack's three tiles, as normal_cases.write_tiles writes them"""
    return {(lat0, lon0 - 10): NC.rough(NC.TILE_N, NC.TILE_N, 4, (lon0 - 10) * (NC.TILE_N - 1),
                                        lat0 * (NC.TILE_N - 1)) for lat0, lon0 in NC.TILES}


def nodes_sha(case):
    """one sha256 over every node array of the case, the geoid included"""
    geoid, layers = recipe(case)
    parts = [geoid_nodes().ravel()] if geoid else []
    for layer in layers:
        for kind, name, _ in layer:
            if kind == MAP:
                parts.append(MAPS[name][0]().ravel())
            elif kind == STACK:
                parts += [z.ravel() for _, z in sorted(tile_nodes().items())]
    return sha(np.concatenate(parts)) if parts else sha(np.zeros(0))


# ---- the three builds ---------------------------------------------------------------------

def _assemble(case, make_map, make_stack, stepper):
    """dict(stepper, data: what to destroy) through the verbs both libraries share"""
    geoid, layers = recipe(case)
    made, keep = {}, []

    def get(kind, name):
        if (kind, name) not in made:
            if kind == MAP:
                z, x, y, zr, projection = MAPS[name]
                made[kind, name] = make_map(z(), x, y, zr, projection)
            else:
                made[kind, name] = make_stack()
            keep.append(made[kind, name])
        return made[kind, name]

    st = stepper()
    if geoid:
        g = make_map(geoid_nodes(), GEOID_X, GEOID_Y, GEOID_Z, None)
        keep.append(g)
        st.geoid_set(g)
    for layer in layers:
        st.add_layer()
        for kind, name, offset in layer:
            if kind == FLAT:
                st.add_flat(offset)
            elif kind == MAP:
                st.add_map(get(kind, name), offset)
            else:
                st.add_stack(get(kind, name), offset)
    return dict(stepper=st, data=keep, stack=made.get((STACK, None)))


def amd_geometry(case, directory, stack_size=0):
    """the case in libturtle_amd: dict(stepper, data, stack).  stack_size 0: every tile resident"""
    import turtle_amd as TA

    def stack():
        s = TA.Stack(NC.write_tiles(os.path.join(str(directory), "tiles")), stack_size)
        if stack_size == 0:
            s.load()
        return s

    return _assemble(case, lambda z, x, y, zr, p: TA.Map.create(z, x, y, zr, projection=p), stack, TA.Stepper)


def reference_geometry(case, directory, local_range=None):
    """the case in the compiled reference (oracle.ref_ffi)"""
    from oracle import ref_ffi as R

    def stack():
        s = R.RefStack(NC.write_tiles(os.path.join(str(directory), "tiles")), 0)
        s.load()
        return s

    def stepper():
        st = R.RefStepper()
        if local_range is not None:
            st.range_set(local_range)
        return st

    return _assemble(case, lambda z, x, y, zr, p: R.RefMap.create(z, x, y, zr, p), stack, stepper)


def destroy(geo):
    geo["stepper"].destroy()
    for d in geo["data"]:
        d.destroy()


def oracle_geometry(case):
    """the case as the CPU restatement's geometry"""
    geoid, layers = recipe(case)
    grids, stacks, index = [], [], {}
    for layer in layers:
        for kind, name, _ in layer:
            if (kind, name) in index or kind == FLAT:
                continue
            if kind == MAP:
                z, x, y, zr, projection = MAPS[name]
                index[kind, name] = len(grids)
                grids.append(O.default_grid(z(), x, y, zr, projection=projection))
            else:
                table = -np.ones((STACK_N, STACK_N), dtype=np.int32)
                for (iy, ix), z in sorted(tile_nodes().items()):
                    table[iy, ix] = len(grids)
                    grids.append(IC.asc_grid(z, STACK_LON0 + ix, STACK_LAT0 + iy, NC.TILE_CELL))
                index[kind, name] = len(stacks)
                stacks.append(dict(lat0=STACK_LAT0, lon0=STACK_LON0, dlat=1.0, dlon=1.0, nlat=STACK_N,
                                   nlon=STACK_N, tile=table))
    g = -1
    if geoid:
        g = len(grids)
        grids.append(O.default_grid(geoid_nodes(), GEOID_X, GEOID_Y, GEOID_Z))
    kinds = {FLAT: O.FLAT, MAP: O.MAP, STACK: O.STACK}
    spec = [[(kinds[kind], index.get((kind, name), 0), offset) for kind, name, offset in layer]
            for layer in layers]
    return O.OracleGeometry(grids=grids, stacks=stacks, layers=spec, geoid=g)


def utm_footprint():
    """(latitude, longitude) of the UTM map's corners, by the restatement's inverse projection"""
    x = np.array([UTM_X[0], UTM_X[1], UTM_X[0], UTM_X[1]])
    y = np.array([UTM_Y[0], UTM_Y[0], UTM_Y[1], UTM_Y[1]])
    return O.unproject(UTM, x, y)


# ---- rays -----------------------------------------------------------------------------------

def _box(case):
    return BOXES[case]


def graze(case, geo=None, n=GRAZE, height=30.0, layer=None):
    """(position, direction, has data): grazing rays from 30 m above the top of the layer below the
    lid (30 m above the ellipsoid where that layer has no data: the third item says where it has),
    any azimuth, elevation -3 .. +1 degrees; by the restatement's transforms (pinned bit for bit to
    the reference's).  `height` and `layer`: see under()."""
    geo = geo or oracle_geometry(case)
    (s, nth), (w, e) = _box(case)
    rng = np.random.default_rng(31)
    assert n <= GRAZE       # (a shorter set is the head of the whole one)
    lat, lon = rng.uniform(s, nth, GRAZE)[:n], rng.uniform(w, e, GRAZE)[:n]
    az, el = rng.uniform(0.0, 360.0, GRAZE)[:n], rng.uniform(-3.0, 1.0, GRAZE)[:n]
    if layer is None:
        layer = len(RECIPES[case][1]) - (2 if case in CASES else 1)
    pos, di = geo.position(lat, lon, height, layer=layer)
    bare = O.ecef_from_geodetic(lat, lon, np.full(n, 30.0))
    pos = np.where((di >= 0)[:, None], pos, bare)
    return (np.ascontiguousarray(pos), np.ascontiguousarray(O.ecef_from_horizontal(lat, lon, az, el)), di >= 0)


def under(case, geo=None, n=UNDER):
    """(position, direction, has data): graze's first rays from 30 m BELOW the top of the case's
    composite layer.  A ray between a layer and the lid reports the lid's data index (the last layer
    that bounds it writes index[1] [ref stepper.c:690-699]), so graze's rays cannot show a change of
    data on their way; these are bounded from above by the composite layer, and index[1] changes
    under a map's rim and under the edges of the stack while the medium stays."""
    return graze(case, geo, n, height=-30.0, layer=COMPOSITE_LAYER[case])


def data_switches(geo, pos, d, max_steps=4000):
    """how many rays change data (index[1]) on their way, the medium staying: the harness loop over
    the restatement's single steps, all rays a step at a time"""
    pos = pos.copy()
    o = geo.step(pos)
    medium, data = o["index"][:, 0].copy(), o["index"][:, 1].copy()
    alive, switched = medium >= 0, np.zeros(pos.shape[0], dtype=bool)
    for _ in range(max_steps):
        if not alive.any():
            break
        rows = np.flatnonzero(alive)
        o = geo.step(pos[rows], d[rows])
        pos[rows] = o["position"]
        same = o["index"][:, 0] == medium[rows]
        switched[rows] |= same & (o["index"][:, 1] != data[rows])
        data[rows] = o["index"][:, 1]
        alive[rows] = same
    return int(switched.sum())


def sight(case, n=SIGHT):
    """(position, direction): lines of sight from over the case's box and 2 % around it, -200 ..
    4000 m above the ellipsoid, any azimuth, elevation -30 .. +3 degrees (ceiling CEILING,
    SIGHT_MAX_STEPS steps at most)"""
    (s, nth), (w, e) = _box(case)
    m = 0.02 * (nth - s)
    rng = np.random.default_rng(32)
    assert n <= SIGHT
    lat, lon = rng.uniform(s - m, nth + m, SIGHT)[:n], rng.uniform(w - m, e + m, SIGHT)[:n]
    height = rng.uniform(-200.0, 4000.0, SIGHT)[:n]
    az, el = rng.uniform(0.0, 360.0, SIGHT)[:n], rng.uniform(-30.0, 3.0, SIGHT)[:n]
    return (np.ascontiguousarray(O.ecef_from_geodetic(lat, lon, height)),
            np.ascontiguousarray(O.ecef_from_horizontal(lat, lon, az, el)))


def walk_origins(case):
    """(latitude, longitude, height) of the scattering walk's 512 origins: every fourth at 30 km
    (above the lid: steps of 10 km), the rest at 60 m, above the bottom layer"""
    (s, nth), (w, e) = _box(case)
    rng = np.random.default_rng(21)
    lat, lon = rng.uniform(s, nth, WALK_RAYS), rng.uniform(w, e, WALK_RAYS)
    return lat, lon, np.where(np.arange(WALK_RAYS) % 4 == 0, 30000.0, 60.0)


# ---- rims -----------------------------------------------------------------------------------

def rim_lines(case):
    """the rim lines of the case's data: [(projection or None, axis 0: a line x = c / 1: y = c, c,
    (from, to) along it)], x = longitude and y = latitude without a projection.  Map rims, the
    stack's outer rim and the two edges of its missing tile."""
    lines, seen = [], set()
    for layer in recipe(case)[1]:
        for kind, name, _ in layer:
            if kind == FLAT or (kind, name) in seen:
                continue
            seen.add((kind, name))
            if kind == MAP:
                _, x, y, _, projection = MAPS[name]
                lines += [(projection, 0, c, y) for c in x] + [(projection, 1, c, x) for c in y]
            else:
                lines += [(None, 0, 10.0, (0.0, 2.0)), (None, 0, 12.0, (0.0, 1.0)), (None, 0, 11.0, (1.0, 2.0)),
                          (None, 1, 0.0, (10.0, 12.0)), (None, 1, 2.0, (10.0, 11.0)), (None, 1, 1.0, (11.0, 12.0))]
    return lines


def rim_points(case, n=RIM_POINTS):
    """(latitude, longitude, eps): about n points 1e-12 .. 1e-4 degree (for the projected map: that
    many times 1e5 metres) either side of every rim line, irregular_cases.edge_points' pattern; eps
    is each point's distance from its line, in degrees"""
    lines = rim_lines(case)
    off = np.concatenate([-IC.EPS[::-1], IC.EPS])
    along_n = max(2, n // (len(lines) * off.size))
    lat, lon, eps = [], [], []
    for projection, axis, c, (a, b) in lines:
        scale = 1e5 if projection else 1.0
        # (0.03 .. 0.96: off the lattice lines that cross this one, where an ulp of the longitude a
        # sample recovers from its ECEF position decides which tile answers)
        t = a + (b - a) * np.linspace(0.03, 0.96, along_n)
        for o in off:
            u, v = np.full(along_n, c + o * scale), t
            x, y = (u, v) if axis == 0 else (v, u)
            if projection:
                y, x = O.unproject(projection, x, y)
            lat.append(y)
            lon.append(x)
            eps.append(np.full(along_n, abs(o)))
    return np.concatenate(lat), np.concatenate(lon), np.concatenate(eps)


def on_a_rim(case, point, within=1e-9):
    """whether each ECEF point lies within `within` degree (times 1e5 metres for the projected
    map) of a rim line of the case's data, between the line's ends"""
    lat, lon, _ = O.ecef_to_geodetic(point)
    hit = np.zeros(lat.size, dtype=bool)
    xy = {}
    for projection, axis, c, (a, b) in rim_lines(case):
        if projection not in xy:
            xy[projection] = O.project(projection, lat, lon) if projection else (lon, lat)
        x, y = xy[projection]
        scale = 1e5 if projection else 1.0
        across, along = (x, y) if axis == 0 else (y, x)
        hit |= (np.abs(across - c) <= within * scale) & (along >= a - within * scale) & (along <= b + within * scale)
    return hit
