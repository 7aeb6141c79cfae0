"""Geometries, points and the restatement of turtle_stepper_normal_n, shared by
tests/golden/generate_normal.py and the normal tests.

Four kinds of geometry, each the smallest that can still go wrong (include/turtle_amd.h has the
definition of the call as a loop):
  "map"    one geodetic map of 17 x 17 nodes around (0N, 0E), rough ground: the one-map kernel;
  "stack"  2 x 2 tiles of 9 x 9 nodes (ESRI .asc, one degree each) at (0..2N, 10..12E) with the
           north-east tile missing: the one-stack kernel, resident and paged;
  "utm", "lambert"   one projected map: the UTM fixture tests/golden/map_utm.png, and a Lambert 93
           map of 33 x 33 nodes made with turtle_map_create: the chain rule of the generic kernel;
  "layers", "layers_geoid"   three layers -- a flat at 0; the stack with a geodetic map of 17 x 17
           nodes added on top of it (data_index 0: the map, 1: the stack where the map ends); a
           flat at 3000 m -- without and with the geoid tests/golden/geoid_small.grd.
The same recipes build the geometry for libturtle_amd (amd_geometry) and for the compiled
reference (reference_geometry); restate() evaluates the call's definition over the latter.
"""
from __future__ import annotations

import math
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = ("map", "stack", "utm", "lambert", "layers", "layers_geoid")
FLAT, MAP, STACK = "flat", "map", "stack"

MAP_X, MAP_Y, MAP_Z, MAP_N = (-1.0, 1.0), (-1.0, 1.0), (0.0, 2000.0), 17      # dx = dy = 1/8 degree
TILES, TILE_N, TILE_CELL = ((0, 10), (0, 11), (1, 10)), 9, 0.125              # (1, 11) is missing
TOP_X, TOP_Y, TOP_Z, TOP_N = (10.5, 11.5), (0.25, 1.25), (0.0, 2000.0), 17    # the map over the stack
LAMBERT, LAMBERT_X, LAMBERT_Y, LAMBERT_Z, LAMBERT_N = \
    "Lambert 93", (700000.0, 703200.0), (6600000.0, 6603200.0), (0.0, 2000.0), 33
UTM, UTM_X, UTM_Y = "UTM 31N", (495000.0, 497000.0), (5066000.0, 5068000.0)
FLAT_TOP = 3000.0
DELTA = 1e-3                    # degrees: the step of the projection's central differences
A, E = 6378137.0, 0.081819190842622   # [ref ecef.c:36-38]


def _hash(ix, iy, salt):
    """integer noise in [0, 2^16): the same on any platform"""
    h = (ix.astype(np.uint64) * np.uint64(0x8DA6B343)) ^ (iy.astype(np.uint64) * np.uint64(0xD8163841))
    h = (h ^ np.uint64(salt * 0x9E3779B1)) & np.uint64(0xFFFFFFFF)
    h = ((h ^ (h >> np.uint64(15))) * np.uint64(0x2C1B3C6D)) & np.uint64(0xFFFFFFFF)
    return ((h ^ (h >> np.uint64(13))) >> np.uint64(8)) & np.uint64(0xFFFF)


def rough(nx, ny, salt, ix0=0, iy0=0):
    """z[iy, ix]: 1000 m, a swell of 400 m and 200 m of node-to-node noise, in whole metres"""
    iy, ix = np.meshgrid(np.arange(ny) + iy0, np.arange(nx) + ix0, indexing="ij")
    noise = _hash(ix, iy, salt).astype(np.float64) * (400.0 / 65536.0) - 200.0
    return np.rint(1000.0 + 400.0 * np.sin(0.9 * ix) * np.cos(0.7 * iy) + noise)


def map_nodes():
    return rough(MAP_N, MAP_N, 1)


def top_nodes():
    return rough(TOP_N, TOP_N, 2)


def lambert_nodes():
    return rough(LAMBERT_N, LAMBERT_N, 3)


def write_tiles(directory):
    """the stack's tiles as .asc files: nodes on a global lattice, so neighbours agree on their seam"""
    os.makedirs(directory, exist_ok=True)
    for lat0, lon0 in TILES:
        z = rough(TILE_N, TILE_N, 4, (lon0 - 10) * (TILE_N - 1), lat0 * (TILE_N - 1))
        with open(os.path.join(directory, f"tile_{lat0}_{lon0}.asc"), "w") as f:
            f.write(f"ncols {TILE_N}\nnrows {TILE_N}\nxllcorner {lon0 - 0.5 * TILE_CELL!r}\n"
                    f"yllcorner {lat0 - 0.5 * TILE_CELL!r}\ncellsize {TILE_CELL!r}\nNODATA_value -9999\n")
            for row in z[::-1]:                           # north row first
                f.write(" ".join(f"{v:.1f}" for v in row) + "\n")
    return directory


# ---- geometries ------------------------------------------------------------------

def _geometry(case, directory, make_map, load_map, make_stack, projection, utm_map=None):
    """layers = [[(kind, data, offset, projection or None), ...] in the order ADDED], geoid"""
    geoid = None
    if case == "map":
        layers = [[(MAP, make_map(map_nodes(), MAP_X, MAP_Y, MAP_Z, None), 0.0, None)]]
    elif case == "stack":
        layers = [[(STACK, make_stack(write_tiles(os.path.join(directory, "tiles"))), 0.0, None)]]
    elif case == "utm":
        layers = [[(MAP, (utm_map or load_map)(os.path.join(GOLDEN, "map_utm.png")), 0.0, projection(UTM))]]
    elif case == "lambert":
        layers = [[(MAP, make_map(lambert_nodes(), LAMBERT_X, LAMBERT_Y, LAMBERT_Z, LAMBERT), 0.0,
                    projection(LAMBERT))]]
    else:
        layers = [[(FLAT, None, 0.0, None)],
                  [(STACK, make_stack(write_tiles(os.path.join(directory, "tiles"))), 0.0, None),
                   (MAP, make_map(top_nodes(), TOP_X, TOP_Y, TOP_Z, None), 0.0, None)],
                  [(FLAT, None, FLAT_TOP, None)]]
        if case == "layers_geoid":
            geoid = load_map(os.path.join(GOLDEN, "geoid_small.grd"))
    return dict(layers=layers, geoid=geoid)


def reference_geometry(case, directory):
    from oracle import ref_ffi as R

    def stack(path):
        s = R.RefStack(path, 0)
        s.load()
        return s

    def utm_map(path):
        # the reference reads a .png through libpng, which it looks for under a name that only a
        # development package installs: the same map from the nodes it was dumped from (png.npz)
        g = np.load(os.path.join(GOLDEN, "png.npz"))
        return R.RefMap.create(g["nodes"], tuple(g["x"]), tuple(g["y"]), tuple(g["z"]), str(g["projection"]))

    return _geometry(case, directory, lambda z, x, y, zr, p: R.RefMap.create(z, x, y, zr, p),
                     R.RefMap.load, stack, R.RefProjection, utm_map)


def amd_geometry(case, directory, stack_size=0):
    """the same geometry in libturtle_amd, with its stepper: dict(stepper, layers, geoid)"""
    import turtle_amd as TA
    geo = _geometry(case, directory, lambda z, x, y, zr, p: TA.Map.create(z, x, y, zr, projection=p),
                    TA.Map.load, lambda path: TA.Stack(path, stack_size), lambda name: None)
    st = TA.Stepper()
    if geo["geoid"] is not None:
        st.geoid_set(geo["geoid"])
    for layer in geo["layers"]:
        if len(geo["layers"]) > 1:
            st.add_layer()
        for kind, data, offset, _ in layer:
            if kind == FLAT:
                st.add_flat(offset)
            elif kind == MAP:
                st.add_map(data, offset)
            else:
                st.add_stack(data, offset)
    geo["stepper"] = st
    return geo


def destroy(geo):
    if "stepper" in geo:
        geo["stepper"].destroy()
    for layer in geo["layers"]:
        for _, data, _, proj in layer:
            for h in (data, proj):
                if h is not None:
                    h.destroy()
    if geo["geoid"] is not None:
        geo["geoid"].destroy()


# ---- points ----------------------------------------------------------------------

def _cell(x, i, h):
    """coordinate of fraction h of cell i of an axis x = (x0, x1) of MAP_N nodes"""
    return x[0] + (i + h) * (x[1] - x[0]) / (MAP_N - 1)


def geodetic_points(case, unproject=None):
    """(latitude, longitude, layer) the case's positions are made from.  unproject(name, x, y): the
    reference's inverse projection (the projected cases choose their points in map coordinates)."""
    rng = np.random.Generator(np.random.Philox(20260 + CASES.index(case)))
    if case == "map":
        spots = [(_cell(MAP_X, 5, hx), _cell(MAP_Y, 6, hy)) for hx in (0.25, 0.75) for hy in (0.25, 0.75)]
        spots += [(_cell(MAP_X, 0, 0.2), _cell(MAP_Y, 7, 0.6)), (_cell(MAP_X, 0, 0.7), _cell(MAP_Y, 7, 0.3)),
                  (_cell(MAP_X, 15, 0.3), _cell(MAP_Y, 3, 0.6)), (_cell(MAP_X, 15, 0.8), _cell(MAP_Y, 3, 0.3)),
                  (_cell(MAP_X, 4, 0.6), _cell(MAP_Y, 0, 0.7)),
                  (_cell(MAP_X, 4, 0.6), _cell(MAP_Y, 0, 0.3)),    # the first half-row: [ref map.c:352-353]
                  (_cell(MAP_X, 9, 0.4), _cell(MAP_Y, 15, 0.3)), (_cell(MAP_X, 9, 0.4), _cell(MAP_Y, 15, 0.8)),
                  (_cell(MAP_X, 0, 0.2), _cell(MAP_Y, 0, 0.2)), (_cell(MAP_X, 15, 0.8), _cell(MAP_Y, 15, 0.8)),
                  (0.0, 0.0),                                       # node (8, 8), exactly (see positions)
                  (1.5, 0.0), (0.3, -1.2)]                          # outside
        n = 257                                                     # not a multiple of a wave or a block
        lon = rng.uniform(-1.05, 1.05, n)
        lat = rng.uniform(-1.05, 1.05, n)
        for k, (x, y) in enumerate(spots):
            lon[k], lat[k] = x, y
        layer = np.zeros(n, dtype=np.int32)
        layer[-3:] = (-1, 1, 7)                                     # no such layer
        return lat, lon, layer
    if case == "stack":
        n = 300
        lat = rng.uniform(-0.05, 2.05, n)
        lon = rng.uniform(9.95, 12.05, n)
        k = 0
        for la, lo in ((0.4, 10.3), (0.6, 11.7), (1.7, 10.2), (1.5, 11.5), (1.99, 11.01)):
            lat[k], lon[k] = la, lo                                 # tile interiors, and the missing tile
            k += 1
        for side in (-1.0, 1.0):                                    # within half a cell of a seam
            for h in (0.45, 0.2, 1e-3):
                lat[k], lon[k] = 0.37, 11.0 + side * h * TILE_CELL
                lat[k + 1], lon[k + 1] = 1.0 + side * h * TILE_CELL, 10.61
                lat[k + 2], lon[k + 2] = 1.0 + side * h * TILE_CELL, 11.0 + side * h * TILE_CELL
                k += 3
        return lat, lon, np.zeros(n, dtype=np.int32)
    if case in ("utm", "lambert"):
        n = 200
        bx, by = (UTM_X, UTM_Y) if case == "utm" else (LAMBERT_X, LAMBERT_Y)
        x = rng.uniform(bx[0] + 0.03 * (bx[1] - bx[0]), bx[1] - 0.03 * (bx[1] - bx[0]), n)
        y = rng.uniform(by[0] + 0.03 * (by[1] - by[0]), by[1] - 0.03 * (by[1] - by[0]), n)
        lat, lon = unproject(UTM if case == "utm" else LAMBERT, x, y)
        return lat, lon, np.zeros(n, dtype=np.int32)
    n = 400
    lat = rng.uniform(-0.05, 2.05, n)
    lon = rng.uniform(9.9, 12.05, n)                                # (the geoid begins at 10E)
    layer = rng.integers(-1, 4, n).astype(np.int32)
    return lat, lon, layer


def positions(case):
    """the case's positions [n][3] and layers, made with the reference's own transforms"""
    from oracle import ref_ffi as R
    projections = {}

    def unproject(name, x, y):
        if name not in projections:
            projections[name] = R.RefProjection(name)
        return projections[name].unproject(x, y)

    lat, lon, layer = geodetic_points(case, unproject)
    for p in projections.values():
        p.destroy()
    rng = np.random.Generator(np.random.Philox(4040 + CASES.index(case)))
    pos = R.ecef_from_geodetic(lat, lon, rng.uniform(-1000.0, 5000.0, lat.size))
    if case == "map":
        k = int(np.flatnonzero((lat == 0.0) & (lon == 0.0))[0])
        pos[k] = (A + 1234.5, 0.0, 0.0)   # to_geodetic gives latitude 0 and longitude 0 exactly
    return pos, layer


# ---- the definition, over the reference's functions ---------------------------------

def surface_normal(lat, lon, hs, glat, glon, pole):
    """step 6 of the definition, in its operand order, in IEEE doubles (sin, cos: the C library's)"""
    lam, phi = lon * math.pi / 180.0, lat * math.pi / 180.0
    sl, cl, sp, cp = math.sin(lam), math.cos(lam), math.sin(phi), math.cos(phi)
    e = (-sl, cl, 0.0)
    n = (-cl * sp, -sl * sp, cp)
    u = (cl * cp, sl * cp, sp)
    g = 1.0 - E * E * sp * sp
    rn = A / math.sqrt(g)
    rm = rn * (1.0 - E * E) / g
    a_ = (rn + hs) * cp * math.pi / 180.0
    b_ = (rm + hs) * math.pi / 180.0
    a, b = glon / a_, glat / b_
    w = [u[i] - b * n[i] if pole else u[i] - a * e[i] - b * n[i] for i in range(3)]
    norm = math.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    return [w[i] / norm for i in range(3)]


def _slopes(kind, data, proj, lat, lon):
    """z, inside, glat, glon of one data at every point (step 4)"""
    n = lat.size
    if kind == FLAT:
        return np.zeros(n), np.ones(n, dtype=np.int32), np.zeros(n), np.zeros(n)
    if kind == STACK:
        z, inside = data.elevation(lat, lon)
        glat, glon, _ = data.gradient(lat, lon, fill=0.0)
        return z, inside, glat, glon
    if proj is None:
        z, inside = data.elevation(lon, lat)
        glon, glat, _ = data.gradient(lon, lat, fill=0.0)
        return z, inside, glat, glon
    x, y = proj.project(lat, lon)
    z, inside = data.elevation(x, y)
    gx, gy, _ = data.gradient(x, y, fill=0.0)
    d = DELTA
    xp, yp = proj.project(lat + d, lon)
    xm, ym = proj.project(lat - d, lon)
    glat = gx * (xp - xm) / (2.0 * d) + gy * (yp - ym) / (2.0 * d)
    xp, yp = proj.project(lat, lon + d)
    xm, ym = proj.project(lat, lon - d)
    glon = gx * (xp - xm) / (2.0 * d) + gy * (yp - ym) / (2.0 * d)
    return z, inside, glat, glon


def restate(geo, position, layer, sentinel=-7.0):
    """turtle_stepper_normal_n as its header comment defines it, over a reference_geometry:
    dict(normal, data_index, latitude, longitude, glat, glon, hs).  Rows without data keep `sentinel`."""
    from oracle import ref_ffi as R
    pos = np.asarray(position, dtype=np.float64).reshape(-1, 3)
    n = pos.shape[0]
    lat, lon, _ = R.ecef_to_geodetic(pos)
    out = dict(normal=np.full((n, 3), sentinel), data_index=np.full(n, -1, dtype=np.int32), latitude=lat,
               longitude=lon, glat=np.zeros(n), glon=np.zeros(n), hs=np.zeros(n))
    table = [[_slopes(kind, data, proj, lat, lon) + (offset,) for kind, data, offset, proj in reversed(metas)]
             for metas in geo["layers"]]                                  # last added first
    if geo["geoid"] is not None:
        lo = np.where(lon >= 0, lon, lon + 360.0)
        u, u_in = geo["geoid"].elevation(lo, lat)
        ugx, ugy, _ = geo["geoid"].gradient(lo, lat, fill=0.0)
    for r in range(n):
        if (layer[r] < 0) or (layer[r] >= len(table)):
            continue
        for k, (z, inside, glat, glon, offset) in enumerate(table[layer[r]]):
            if not inside[r]:
                continue
            hs, ga, go = float(z[r]) + offset, float(glat[r]), float(glon[r])
            if geo["geoid"] is not None and u_in[r]:
                hs += float(u[r])
                go += float(ugx[r])
                ga += float(ugy[r])
            pole = (pos[r, 0] == 0.0) and (pos[r, 1] == 0.0)
            out["normal"][r] = surface_normal(float(lat[r]), float(lon[r]), hs, ga, go, pole)
            out["data_index"][r], out["glat"][r], out["glon"][r], out["hs"][r] = k, ga, go, hs
            break
    return out
