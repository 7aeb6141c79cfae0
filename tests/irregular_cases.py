"""Irregular tile stacks: the directories, rays and CPU restatement shared by
tests/golden/generate_irregular.py and the tests (tests/test_oracle_golden.py,
tests/test_gpu_irregular.py).

tamd_stepper_flatten (turtle_amd/csrc/stepper.c) calls a stack regular when its resident tiles
share one shape (nx, ny, dx, dy, z0, dz, signedness), sit on the directory's lattice, hold at most
2^24 cells and the directory has at most 254 slots; the device code forks on that.  The reference
asks only for equal tile spans [ref stack.c:90-105].  Four directories, all from (0N, 10E), of
ESRI .asc tiles whose nodes are normal_cases.rough on a lattice per tile size (tiles of one size
agree on their seams, tiles of different sizes do not: cliffs):

  "mixed"     3 x 3 slots of one degree; tiles of 9, 17, 33, 17, 5, 9, 33 and 3 nodes a side and
              (2, 1) missing: irregular by shape, and by z0 / dz (an .asc tile's own range);
  "slots255"  15 x 17 slots of 1/8 degree, 5 nodes a side, (7, 8) missing: by count, and z0 / dz;
  "slots254"  2 x 127 slots of 1/8 degree, 5 nodes a side, (1, 60) missing: by z0 / dz alone;
  "slots256"  16 x 16 slots of 1/8 degree, 3 nodes a side, none missing: by count, and z0 / dz.

The int16 twins (the same nodes as GeoTIFF-16: z0 = -32767, dz = 1 everywhere) single the
criteria out: "mixed" by shape only, "slots255" by count only, and "slots254" is regular.
"""
from __future__ import annotations

import hashlib
import os

import numpy as np

from oracle import ffi as O

import normal_cases as NC
import tiff_cases as TC

LAT0, LON0 = 0.0, 10.0
NODATA = -9999.0


def _uniform(nlat, nlon, n, salt, missing):
    return {(iy, ix): (n, salt) for iy in range(nlat) for ix in range(nlon) if (iy, ix) not in missing}


# case -> (nlat, nlon, tile span in degrees, {(iy, ix): (nodes a side, salt)})
DIRECTORIES = {
    "mixed": (3, 3, 1.0, {(0, 0): (9, 1), (0, 1): (17, 2), (0, 2): (33, 3), (1, 0): (17, 4), (1, 1): (5, 5),
                          (1, 2): (9, 6), (2, 0): (33, 7), (2, 2): (3, 8)}),
    "slots255": (15, 17, 0.125, _uniform(15, 17, 5, 9, {(7, 8)})),
    "slots254": (2, 127, 0.125, _uniform(2, 127, 5, 9, {(1, 60)})),
    "slots256": (16, 16, 0.125, _uniform(16, 16, 3, 9, set())),
}
CASES = tuple(DIRECTORIES)
TWINS = ("mixed", "slots255", "slots254")
RAYS, GOLDEN_RAYS, MAX_STEPS = 2000, 500, 20000
CEILING = 5000.0


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def tile_nodes(case):
    """{(iy, ix): z[row south -> north, column]} in whole metres"""
    return {(iy, ix): NC.rough(n, n, salt, ix * (n - 1), iy * (n - 1))
            for (iy, ix), (n, salt) in DIRECTORIES[case][3].items()}


def box(case):
    """((south, north), (west, east)) of the directory"""
    nlat, nlon, span, _ = DIRECTORIES[case]
    return (LAT0, LAT0 + nlat * span), (LON0, LON0 + nlon * span)


def write_asc(directory, case):
    """the case's tiles as ESRI .asc files (north row first, the corner half a cell out)"""
    directory = str(directory)
    os.makedirs(directory, exist_ok=True)
    span = DIRECTORIES[case][2]
    for (iy, ix), z in tile_nodes(case).items():
        n = z.shape[0]
        cell = span / (n - 1)
        with open(os.path.join(directory, f"tile_{iy:03d}_{ix:03d}.asc"), "w") as f:
            f.write(f"ncols {n}\nnrows {n}\nxllcorner {LON0 + ix * span - 0.5 * cell!r}\n"
                    f"yllcorner {LAT0 + iy * span - 0.5 * cell!r}\ncellsize {cell!r}\n"
                    f"NODATA_value {NODATA:.0f}\n")
            for row in z[::-1]:
                f.write(" ".join(f"{v:.1f}" for v in row) + "\n")
    return directory


def write_twin(directory, case):
    """the same nodes as int16 GeoTIFF tiles"""
    directory = str(directory)
    span = DIRECTORIES[case][2]
    for (iy, ix), z in tile_nodes(case).items():
        cell = span / (z.shape[0] - 1)
        TC.write_tiff(os.path.join(directory, f"tile_{iy:03d}_{ix:03d}.tif"), z.astype(np.int16),
                      x0=LON0 + ix * span, y_top=LAT0 + (iy + 1) * span, dx=cell, dy=cell)
    return directory


def asc_range(z):
    """(z0, dz) as the reference's .asc reader finds them [ref asc.c:87-111]: one scan in file
    order (the north row first) that starts zmax at -DBL_MIN and raises it only in the `else` of
    the zmin test -- a tile whose first node is its highest gets the second highest as zmax"""
    zmin, zmax = np.finfo(np.float64).max, -np.finfo(np.float64).tiny
    for d in z[::-1].ravel().tolist():
        if d == NODATA:
            continue
        elif d < zmin:
            zmin = d
        elif d > zmax:
            zmax = d
    return zmin, (zmax - zmin) / 65535


def asc_grid(z, x0, y0, cell):
    """an .asc tile as the reader holds it: uint16 codes over the scan's range, rows south -> north
    [ref asc.c:132-148]; a code beyond 65535 (the highest node, when the scan missed it) keeps its
    low 16 bits, as the conversion to uint16_t does on the build's compiler"""
    z0, dz = asc_range(z)
    codes = np.floor((z - z0) / dz + 0.5).astype(np.int64) & 0xFFFF     # round(): values are >= 0
    n = z.shape[0]
    return dict(nx=n, ny=n, x0=x0, y0=y0, dx=cell, dy=cell, z0=z0, dz=dz, layout=O.LAYOUT_DEFAULT,
                data=codes.astype(np.uint16))


def twin_grid(z, x0, y0, cell):
    """a GeoTIFF-16 tile: the raw int16 payload in the HGT layout (north row first)"""
    g = O.hgt_grid(0, 0, z)
    g.update(x0=x0, y0=y0, dx=cell, dy=cell)
    return g


def oracle_geometry(case, twin=False):
    """the CPU restatement's geometry: one stack in one layer"""
    nlat, nlon, span, _ = DIRECTORIES[case]
    grids, table = [], -np.ones((nlat, nlon), dtype=np.int32)
    for (iy, ix), z in tile_nodes(case).items():
        table[iy, ix] = len(grids)
        cell = span / (z.shape[0] - 1)
        grids.append((twin_grid if twin else asc_grid)(z, LON0 + ix * span, LAT0 + iy * span, cell))
    stack = dict(lat0=LAT0, lon0=LON0, dlat=span, dlon=span, nlat=nlat, nlon=nlon, tile=table)
    return O.OracleGeometry(grids=grids, stacks=[stack], layers=[[(O.STACK, 0, 0.0)]])


def rays(case, n=RAYS):
    """(position, direction): origins uniform over the directory and 2 % of a tile around it,
    1500 .. 4000 m above the ellipsoid (the ground is at 400 .. 1600 m), any azimuth, elevation
    -30 .. +3 degrees; by the restatement's transforms (pinned bit for bit to the reference's)"""
    (s, nth), (w, e) = box(case)
    m = 0.02 * DIRECTORIES[case][2]
    rng = np.random.default_rng(2)
    assert n <= RAYS       # (a shorter set is the head of the whole one)
    lat, lon = rng.uniform(s - m, nth + m, RAYS)[:n], rng.uniform(w - m, e + m, RAYS)[:n]
    height = rng.uniform(1500.0, 4000.0, RAYS)[:n]
    az, el = rng.uniform(0.0, 360.0, RAYS)[:n], rng.uniform(-30.0, 3.0, RAYS)[:n]
    return (np.ascontiguousarray(O.ecef_from_geodetic(lat, lon, height)),
            np.ascontiguousarray(O.ecef_from_horizontal(lat, lon, az, el)))


EPS = np.array([1e-12, 1e-11, 1e-10, 1e-9, 1e-8, 1e-7, 1e-6, 1e-5, 1e-4])


def edge_points(case):
    """(latitude, longitude) 1e-12 .. 1e-4 degree either side of lines of the directory's lattice --
    the rim, seams and the edges of the missing tile -- 23 samples along each, and the corners"""
    nlat, nlon, span, tiles = DIRECTORIES[case]
    (s, n), (w, e) = box(case)
    off = np.concatenate([-EPS[::-1], EPS])
    missing = [(iy, ix) for iy in range(nlat) for ix in range(nlon) if (iy, ix) not in tiles]
    hole = missing[0] if missing else (nlat // 2, nlon // 2)
    lat_lines = sorted({0, hole[0], hole[0] + 1, nlat})
    lon_lines = sorted({0, hole[1], hole[1] + 1, nlon})
    if case == "mixed":
        lat_lines, lon_lines = list(range(nlat + 1)), list(range(nlon + 1))
    # along a line: across the whole directory when it is small, else around the hole
    lo, hi = (0.03, max(nlat, nlon) - 0.03) if case == "mixed" else (-1.47, 2.47)
    along = np.linspace(lo, hi, 23) * span
    lat, lon = [], []
    for k in lat_lines:
        for o in off:
            lat.append(np.full(along.size, LAT0 + k * span + o))
            lon.append(LON0 + (0 if case == "mixed" else hole[1] * span) + along)
    for k in lon_lines:
        for o in off:
            lat.append(LAT0 + (0 if case == "mixed" else hole[0] * span) + along)
            lon.append(np.full(along.size, LON0 + k * span + o))
    cl, co = np.meshgrid(LAT0 + np.array(lat_lines) * span, LON0 + np.array(lon_lines) * span)
    for o1 in off[::4]:
        for o2 in off[::4]:
            lat.append((cl + o1).ravel())
            lon.append((co + o2).ravel())
    return np.concatenate(lat), np.concatenate(lon)


def lookup_points(case, n_random=1000, n_edge=1000):
    """(latitude, longitude) of the lookups pinned in irregular.npz: random points over the
    directory and a margin, and every k-th of edge_points"""
    (s, n), (w, e) = box(case)
    m = 0.05 * DIRECTORIES[case][2]
    rng = np.random.default_rng(5)
    lat, lon = rng.uniform(s - m, n + m, n_random), rng.uniform(w - m, e + m, n_random)
    elat, elon = edge_points(case)
    k = max(1, elat.size // n_edge)
    return np.concatenate([lat, elat[::k]]), np.concatenate([lon, elon[::k]])


def stack_gradient(geo, case, latitude, longitude):
    """turtle_stack_gradient restated: the gradient of the tile of the point's slot
    [ref stack.c:364-388]; (glat, glon, inside), zeros outside"""
    table = np.ctypeslib.as_array(O.C.cast(geo.stacks[0].tile, O.c_int_p),
                                  (geo.stacks[0].nlat * geo.stacks[0].nlon,))
    slot = slot_of(case, latitude, longitude)
    tile = np.where(slot >= 0, table[np.maximum(slot, 0)], -1)
    glat, glon = np.zeros(latitude.size), np.zeros(latitude.size)
    inside = np.zeros(latitude.size, dtype=np.int32)
    for t in np.unique(tile[tile >= 0]):
        sel = np.flatnonzero(tile == t)
        gx, gy, ins = geo.grid_gradient(int(t), longitude[sel], latitude[sel], fill=0.0)
        glat[sel], glon[sel], inside[sel] = gy, gx, ins
    return glat, glon, inside


def slot_of(case, latitude, longitude):
    """the directory slot of each point, -1 outside the directory [ref stack.c:415-423]"""
    nlat, nlon, span, _ = DIRECTORIES[case]
    with np.errstate(invalid="ignore"):
        ix = np.floor((longitude - LON0) / span).astype(np.int64)
        iy = np.floor((latitude - LAT0) / span).astype(np.int64)
    ok = (longitude >= LON0) & (latitude >= LAT0) & (ix < nlon) & (iy < nlat)
    return np.where(ok, iy * nlon + ix, -1)
