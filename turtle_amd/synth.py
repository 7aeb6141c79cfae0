"""Synthetic terrain and ray recipes for tests and bench (harness inputs).

No real DEM data exists in the build container or on the GPU box, so every
configuration in BASELINE.json runs on terrain regenerated from a formula
(SURVEY.md 8d).  Pure numpy; nothing here computes elevations, transforms or
steps -- that is the library's job.
"""
from __future__ import annotations

import os

import numpy as np

HGT_N = 3601  # SRTMGL1 nodes per tile edge (reference: src/turtle/io/hgt.c:98-104)


def c1_gradient_nodes(nx: int = 256, ny: int = 256) -> np.ndarray:
    """C1 map elevations z[iy, ix] = 200 + 1500*ix/(nx-1) (flat gradient along x)."""
    ix = np.arange(nx, dtype=np.float64)
    return np.broadcast_to(200.0 + 1500.0 * ix / (nx - 1), (ny, nx)).copy()


def srtm_like_nodes(lat0: int, lon0: int, n: int = HGT_N) -> np.ndarray:
    """Elevations of one 1x1 degree tile, as int16 [row south->north, col west->east].

    z = round(500 + 400 sin(0.01 J) cos(0.013 I)) with GLOBAL node indices
    J = (lon0)*(n-1)+j, I = (lat0)*(n-1)+i counted from (0N, 0E), so that
    adjacent tiles agree on their shared edge row/column like real SRTM tiles.
    """
    j = (lon0 * (n - 1) + np.arange(n, dtype=np.int64)).astype(np.float64)
    i = (lat0 * (n - 1) + np.arange(n, dtype=np.int64)).astype(np.float64)
    z = 500.0 + 400.0 * np.sin(0.01 * j)[None, :] * np.cos(0.013 * i)[:, None]
    return np.rint(z).astype(np.int16)


def hgt_name(lat0: int, lon0: int, n: int = HGT_N) -> str:
    ns = "N" if lat0 >= 0 else "S"
    ew = "E" if lon0 >= 0 else "W"
    # a bare name or an SRTMGL1 suffix means 3601 nodes, anything else 1201
    suffix = "" if n == HGT_N else ".SRTMGL3"
    return f"{ns}{abs(lat0):02d}{ew}{abs(lon0):03d}{suffix}.hgt"


def hgt_bytes(nodes_s2n: np.ndarray) -> bytes:
    """Serialise south->north int16 nodes as an .hgt payload (big-endian, north row first)."""
    return np.ascontiguousarray(nodes_s2n[::-1, :]).astype(">i2").tobytes()


def write_hgt(directory: str, lat0: int, lon0: int, n: int = HGT_N) -> str:
    os.makedirs(directory, exist_ok=True)
    path = os.path.join(directory, hgt_name(lat0, lon0, n))
    with open(path, "wb") as f:
        f.write(hgt_bytes(srtm_like_nodes(lat0, lon0, n)))
    return path


def uniform_rays(n: int, lat_range, lon_range, seed: int = 0x5EED2026,
                 margin: float = 0.1, el_range=(-10.0, -1.0), jump: int = 0):
    """The common ray recipe: origin (lat, lon) uniform inside the
    box shrunk by `margin` of its span, azimuth U[0,360), elevation U[el_range].
    Counter-based Philox stream: `jump` = r selects the r-th jumped stream, so
    rank r of a sharded run draws block r of one global ray array."""
    bits = np.random.Philox(seed)
    if jump:
        bits = bits.jumped(jump)
    rng = np.random.Generator(bits)
    u = rng.random((4, n))
    dlat = lat_range[1] - lat_range[0]
    dlon = lon_range[1] - lon_range[0]
    lat = lat_range[0] + dlat * (margin + (1 - 2 * margin) * u[0])
    lon = lon_range[0] + dlon * (margin + (1 - 2 * margin) * u[1])
    az = 360.0 * u[2]
    el = el_range[0] + (el_range[1] - el_range[0]) * u[3]
    return lat, lon, az, el


def geotiff_name(lat0: int, lon0: int) -> str:
    """ASTER-GDEM2's tile name (the terrain BASELINE's C5 names)"""
    ns = "N" if lat0 >= 0 else "S"
    ew = "E" if lon0 >= 0 else "W"
    return f"ASTGTM2_{ns}{abs(lat0):02d}{ew}{abs(lon0):03d}_dem.tif"


def geotiff_bytes(nodes_s2n: np.ndarray, lon0: float, lat1: float, dx: float, dy: float) -> bytes:
    """The grid as an uncompressed single-strip GeoTIFF of int16 samples, little-endian, scan
    lines north->south, with the two GeoTIFF tags the reference reads: ModelPixelScale (33550)
    and ModelTiepoint (33922) [ref src/turtle/io/geotiff16.c:205-214]."""
    import struct
    ny, nx = nodes_s2n.shape
    data = np.ascontiguousarray(nodes_s2n[::-1, :]).astype("<i2").tobytes()
    scale = struct.pack("<3d", dx, dy, 0.0)
    tie = struct.pack("<6d", 0.0, 0.0, 0.0, lon0, lat1, 0.0)
    n_tags = 12
    ifd_at = 8
    extra_at = ifd_at + 2 + 12 * n_tags + 4
    scale_at, tie_at = extra_at, extra_at + len(scale)
    data_at = tie_at + len(tie)
    def tag(code, kind, count, value):
        return struct.pack("<HHII", code, kind, count, value)
    tags = [tag(256, 4, 1, nx), tag(257, 4, 1, ny), tag(258, 3, 1, 16), tag(259, 3, 1, 1),
            tag(262, 3, 1, 1), tag(273, 4, 1, data_at), tag(277, 3, 1, 1), tag(278, 4, 1, ny),
            tag(279, 4, 1, len(data)), tag(339, 3, 1, 2), tag(33550, 12, 3, scale_at),
            tag(33922, 12, 6, tie_at)]
    return (b"II" + struct.pack("<HI", 42, ifd_at) + struct.pack("<H", n_tags) + b"".join(tags) +
            struct.pack("<I", 0) + scale + tie + data)


def write_geotiff(directory: str, lat0: int, lon0: int, n: int = HGT_N) -> str:
    """One 1x1 degree tile of the synthetic terrain as ASTER-GDEM2 ships it: GeoTIFF, int16"""
    os.makedirs(directory, exist_ok=True)
    path = os.path.join(directory, geotiff_name(lat0, lon0))
    step = 1.0 / (n - 1)
    with open(path, "wb") as f:
        f.write(geotiff_bytes(srtm_like_nodes(lat0, lon0, n), float(lon0), float(lat0 + 1), step, step))
    return path


def _hash32(x: np.ndarray, y: np.ndarray, salt: int) -> np.ndarray:
    """A 32-bit integer hash of integer lattice coordinates (uint64 arithmetic, masked): the same
    words on any platform and any numpy, which np.random does not promise across versions."""
    m = np.uint64(0xFFFFFFFF)
    h = (x.astype(np.uint64) * np.uint64(0x8DA6B343)) & m
    h ^= (y.astype(np.uint64) * np.uint64(0xD8163841)) & m
    h ^= np.uint64((salt * 0xCB1AB31F) & 0xFFFFFFFF)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x7FEB352D)) & m
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x846CA68B)) & m
    h ^= h >> np.uint64(16)
    return h


def rough_nodes(n: int = 1201, seed: int = 1, amplitude: int = 800, noise: int = 200) -> np.ndarray:
    """Rough ground on one tile, as int16 [row south->north, col west->east]: 1000 m plus five
    octaves of integer value noise (lattice cells of 256 down to 16 nodes, bilinear weights in
    integers, octave o weighing amplitude / 2^o) plus per-node noise in [-noise, noise] m.  Every
    value comes from an integer hash of (node or lattice point, seed): ridges and hollows at
    every scale, so lines of sight cross the ground many times."""
    iy, ix = np.meshgrid(np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int64), indexing="ij")
    z = np.full((n, n), 1000, dtype=np.int64)
    for o, cell in enumerate((256, 128, 64, 32, 16)):
        cx, cy = ix // cell, iy // cell
        fx, fy = ix % cell, iy % cell
        def lattice(dx, dy):
            return (_hash32(cx + dx, cy + dy, 16 * seed + o) >> np.uint64(16)).astype(np.int64) - 32768
        v = (lattice(0, 0) * (cell - fx) * (cell - fy) + lattice(1, 0) * fx * (cell - fy) +
             lattice(0, 1) * (cell - fx) * fy + lattice(1, 1) * fx * fy) // (cell * cell)
        z += (amplitude * v) // (32768 << o)
    z += (_hash32(ix, iy, 16 * seed + 15) % np.uint64(2 * noise + 1)).astype(np.int64) - noise
    return np.clip(z, -32767, 32767).astype(np.int16)


VOID = -32768  # an HGT void [ref src/turtle/io/hgt.c reads it as an elevation, unmasked]


def with_voids(nodes: np.ndarray, blocks) -> np.ndarray:
    """A copy of int16 nodes [row south->north, col west->east] with each block (row0, row1, col0,
    col1), half-open, set to the HGT void value"""
    out = np.array(nodes, dtype=np.int16, copy=True)
    for r0, r1, c0, c1 in blocks:
        out[r0:r1, c0:c1] = VOID
    return out


def write_nodes_hgt(directory: str, lat0: int, lon0: int, nodes_s2n: np.ndarray) -> str:
    """Any square int16 nodes [row south->north] as an .hgt tile named for (lat0, lon0)"""
    os.makedirs(directory, exist_ok=True)
    path = os.path.join(directory, hgt_name(lat0, lon0, nodes_s2n.shape[0]))
    with open(path, "wb") as f:
        f.write(hgt_bytes(nodes_s2n))
    return path


def write_rough_hgt(directory: str, lat0: int, lon0: int, n: int = 1201, seed: int = 1,
                    amplitude: int = 800) -> str:
    """rough_nodes as an .hgt tile named for (lat0, lon0)"""
    os.makedirs(directory, exist_ok=True)
    path = os.path.join(directory, hgt_name(lat0, lon0, n))
    with open(path, "wb") as f:
        f.write(hgt_bytes(rough_nodes(n, seed, amplitude)))
    return path
