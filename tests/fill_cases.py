"""What the turtle_map_fill_n tests share: the spans and values of tests/golden/fill.npz (written
by tests/golden/generate_fill.py from the compiled reference), and the maps and windows of the
comparisons against the scalar loop."""
import ctypes as C

import numpy as np

# name -> the z range given to turtle_map_create (dz = (z1 - z0) / 65535).  "unit" and "quarter"
# have a power of two for dz, so z0 + (k + 0.5) * dz is exact; "negative" has z0 < 0 and a dz
# that is no machine number.
SPANS = {"unit": (0.0, 65535.0), "negative": (-100.0, 3000.0), "quarter": (-128.0, 16255.75)}
N_RANDOM = 3000
HALF_K = (0, 1, 2, 3, 7, 100, 32767, 32768, 65533, 65534)


def dz_of(span):
    return (span[1] - span[0]) / 65535


def values(name):
    """the elevations of span `name`: edge cases first, then seeded random ones (a fifth or so
    outside the span)"""
    z0, z1 = SPANS[name]
    dz = dz_of((z0, z1))
    top = z0 + 65535 * dz
    v = [z0, top, z1, np.nextafter(z0, -np.inf), np.nextafter(top, np.inf), np.nextafter(z0, np.inf),
         np.nextafter(top, -np.inf), -0.0, 0.0]
    for k in HALF_K:
        h = z0 + (k + 0.5) * dz
        v += [h, np.nextafter(h, -np.inf), np.nextafter(h, np.inf)]
    rng = np.random.default_rng(sorted(SPANS).index(name) + 20)
    width = z1 - z0
    v += list(z0 - 0.1 * width + 1.2 * width * rng.random(N_RANDOM))
    return np.array(v, dtype=np.float64)


def window_shape(n):
    """a 2-D window for n values: rows of 57 (no multiple of 8), the last one padded by the caller"""
    nx = 57
    return (n + nx - 1) // nx, nx


# the twin-map comparisons: (nx, ny) of the map; windows as (ix0, iy0, nx, ny, ld - nx)
SHAPES = [(19, 13), (8, 8), (65, 9)]


def windows(nx, ny):
    w = [(0, 0, nx, ny, 0),                 # the whole map
         (0, ny // 2, nx, 1, 0),            # one full row
         (nx // 2, 0, 1, ny, 0),            # one full column
         (max(nx - 5, 0), max(ny - 3, 0), min(5, nx), min(3, ny), 0),  # ends in the last (partial) block
         (1, 1, min(6, nx - 1), min(5, ny - 1), 5)]                   # ld = nx + 5
    if nx > 11 and ny > 10:
        w.append((9, 9, 3, 2, 0))           # inside one block
    if nx > 8 and ny > 8:
        w.append((7, 7, 2, 2, 0))           # across four blocks
    return w


def scalar_fill(lib, h, ix0, iy0, z):
    fill = lib.turtle_map_fill
    for j in range(z.shape[0]):
        for i in range(z.shape[1]):
            assert fill(h, ix0 + i, iy0 + j, C.c_double(float(z[j, i]))) == 0


def scalar_nodes(lib, h, nx, ny):
    """the node values through a turtle_map_node loop"""
    node = lib.turtle_map_node
    z = C.c_double()
    out = np.empty((ny, nx), dtype=np.float64)
    for iy in range(ny):
        for ix in range(nx):
            assert node(h, ix, iy, None, None, C.byref(z)) == 0
            out[iy, ix] = z.value
    return out
