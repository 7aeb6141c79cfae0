"""What the tests of turtle_stepper_advance_grid_n share: the box of voxels and the formula of its
densities, the walk through it in Python floats (a third statement of include/turtle_amd.h's
grid_depth, beside the C checker's and the device's), the CPU checker (tests/c/advance_grid_loop.c
over the oracle's restatement of turtle_stepper_step), the same loop over the compiled reference,
and the recipe that gives each ray of a batch a depth budget and a distance limit.  The geometries,
rays and crossings are those of traverse_cases / advance_cases; as in advance_exp_cases a budget is
drawn from the profile (d, X) that an uncut run of the loop records after every step, and inside a
step the stop comes from the Python walk.
"""
from __future__ import annotations

import ctypes as C
import math
import os
import subprocess
import tempfile

import numpy as np

from oracle import ffi as O

import advance_cases as AC

ROOT = AC.ROOT
SPENT, DISTANCE, LEFT, CEILING, MAX_STEPS = range(5)
OUTPUTS = AC.OUTPUTS
INF = float("inf")
DENSITY = AC.DENSITY          # outside the box: rock, (water,) air, kg / m^3
SEED = 0x6A1DBAD
MARGIN = AC.MARGIN
BATCHES = AC.BATCHES

# ---- the box ----------------------------------------------------------------------
# An east-north-up box at the middle of the 45N 3E tile: 64 x 64 x 16 voxels of 1000 x 1000 x 150 m,
# from 400 m under the ellipsoid there (below the lowest ground of the three cases, the tangent
# plane's rise over the ellipsoid towards the rim included: 80 m at 32 km) to 2000 m above it: the
# rough tile's ground rises past its top on purpose.
LATITUDE, LONGITUDE, HEIGHT = 45.5, 3.5, 0.0
N = (64, 64, 16)                      # voxels along east, north, up
SIZE = (1000.0, 1000.0, 150.0)        # metres
OFFSET = (-32000.0, -32000.0, -400.0)  # the corner of voxel (0, 0, 0) from the centre, metres
MEDIUM = 0                            # the rock
BLOCK = ((20, 28), (30, 40), (2, 8))  # a light body: voxels [lo, hi) along each axis
BLOCK_DENSITY = 1000.0


def voxels(n=N, block=BLOCK):
    """[n2][n1][n0]: a smooth field between 1800 and 3200 kg / m^3 and one block at 1000; no zero
    anywhere (where rock is void the reach is discontinuous in the budget: tested apart)"""
    i2, i1, i0 = np.meshgrid(np.arange(n[2]), np.arange(n[1]), np.arange(n[0]), indexing="ij")
    rho = 2500.0 + 700.0 * np.sin(0.37 * i0 + 0.21 * i2) * np.cos(0.23 * i1 - 0.4 * i2)
    if block is not None:
        (a0, b0), (a1, b1), (a2, b2) = block
        rho[a2:b2, a1:b1, a0:b0] = BLOCK_DENSITY
    return np.ascontiguousarray(rho)


class Box:
    """a struct turtle_amd_grid in numpy: origin (3), axis (3, 3), size (3), n (3), medium, density
    [n2][n1][n0]"""

    def __init__(self, origin, axis, size, density, medium=0):
        self.origin = np.ascontiguousarray(origin, dtype=np.float64).reshape(3)
        self.axis = np.ascontiguousarray(axis, dtype=np.float64).reshape(3, 3)
        self.size = np.ascontiguousarray(size, dtype=np.float64).reshape(3)
        self.density = np.ascontiguousarray(density, dtype=np.float64)
        self.n = tuple(int(v) for v in self.density.shape[::-1])
        self.medium = int(medium)
        self._flat = self.density.reshape(-1).tolist()
        self._o, self._a, self._s = self.origin.tolist(), self.axis.tolist(), self.size.tolist()

    def struct(self):
        g = _Grid()
        g.origin[:] = self._o
        for a in range(3):
            g.axis[a][:] = self._a[a]
        g.size[:] = self._s
        g.n[:] = self.n
        g.medium = self.medium
        g.density = self.density.ctypes.data
        return g


def enu_frame(latitude, longitude, height, offset):
    """turtle_amd_grid_enu in numpy, by the oracle's transforms: -> origin, axis"""
    axis = np.array([O.ecef_from_horizontal(latitude, longitude, az, el).reshape(3)
                     for az, el in ((90.0, 0.0), (0.0, 0.0), (0.0, 90.0))])
    origin = np.asarray(O.ecef_from_geodetic(latitude, longitude, height), dtype=np.float64).reshape(3)
    origin = origin + offset[0] * axis[0] + offset[1] * axis[1] + offset[2] * axis[2]
    return origin, axis


def golden_box(origin=None, axis=None):
    """the fixture's box (origin and axis: those the fixture stores, or the oracle's)"""
    if origin is None:
        origin, axis = enu_frame(LATITUDE, LONGITUDE, HEIGHT, OFFSET)
    return Box(origin, axis, SIZE, voxels(), MEDIUM)


class _Grid(C.Structure):
    _fields_ = [("origin", C.c_double * 3), ("axis", (C.c_double * 3) * 3), ("size", C.c_double * 3),
                ("n", C.c_int * 3), ("medium", C.c_int), ("density", C.c_void_p)]


# ---- the walk, in Python floats ---------------------------------------------------

def grid_depth(G, rho_out, m, p0, dr, L, R, pieces=None):
    """include/turtle_amd.h's grid_depth, statement for statement -> (x, f, stopped).  pieces: a
    list that gets every piece (a, b, rho) the walk went through."""
    acc = 0.0

    def piece(a, b, rho):
        nonlocal acc
        if pieces is not None:
            pieces.append((a, b, rho))
        x = rho * (b - a)
        if x > 0 and acc + x >= R:
            return a + (R - acc) / rho
        acc += x
        return None

    f = 0.0
    if G is not None and m == G.medium:
        o, ax, size, n, rho = G._o, G._a, G._s, G.n, G._flat
        s = [ax[a][0] * (p0[0] - o[0]) + ax[a][1] * (p0[1] - o[1]) + ax[a][2] * (p0[2] - o[2]) for a in range(3)]
        t = [ax[a][0] * dr[0] + ax[a][1] * dr[1] + ax[a][2] * dr[2] for a in range(3)]
        f0, f1, hit = 0.0, L, True
        for a in range(3):
            E = n[a] * size[a]
            if t[a] == 0:
                if not (s[a] >= 0 and s[a] < E):
                    hit = False
            else:
                u, v = (0 - s[a]) / t[a], (E - s[a]) / t[a]
                if u > v:
                    u, v = v, u
                if u > f0:
                    f0 = u
                if v < f1:
                    f1 = v
        if hit and f0 < f1:
            stop = piece(0.0, f0, rho_out)
            if stop is not None:
                return acc, stop, True
            i, nxt = [0, 0, 0], [INF, INF, INF]
            for a in range(3):
                c = math.floor((s[a] + f0 * t[a]) / size[a])
                i[a] = min(max(int(c), 0), n[a] - 1)
                nxt[a] = INF if t[a] == 0 else ((i[a] + (1 if t[a] > 0 else 0)) * size[a] - s[a]) / t[a]
            f = f0
            while True:
                a = 0 if (nxt[0] <= nxt[1] and nxt[0] <= nxt[2]) else (1 if nxt[1] <= nxt[2] else 2)
                g = nxt[a] if nxt[a] < f1 else f1
                if g < f:
                    g = f
                stop = piece(f, g, rho[(i[2] * n[1] + i[1]) * n[0] + i[0]])
                if stop is not None:
                    return acc, stop, True
                f = g
                if not nxt[a] < f1:
                    break
                i[a] += 1 if t[a] > 0 else -1
                if i[a] < 0 or i[a] >= n[a]:
                    break
                nxt[a] = ((i[a] + (1 if t[a] > 0 else 0)) * size[a] - s[a]) / t[a]
    stop = piece(f, L, rho_out)
    if stop is not None:
        return acc, stop, True
    return acc, L, False


# ---- the CPU checker ---------------------------------------------------------------

_checker = None


def checker():
    """tests/c/advance_grid_loop.c, compiled against oracle/libturtle_oracle.so"""
    global _checker
    if _checker is None:
        O.lib()  # builds libturtle_oracle.so if needed
        odir = os.path.join(ROOT, "oracle")
        out = tempfile.mkdtemp(prefix="turtle_advance_grid_")
        so = os.path.join(out, "libadvance_grid_loop.so")
        subprocess.check_call(["gcc", "-O2", "-std=gnu99", "-fPIC", "-ffp-contract=off", "-pthread",
                               "-shared", "-I" + odir, "-o", so,
                               os.path.join(ROOT, "tests", "c", "advance_grid_loop.c"),
                               "-L" + odir, "-lturtle_oracle", "-Wl,-rpath," + odir, "-lm"])
        _checker = C.CDLL(so)
    return _checker


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def check(geometry, position, direction, density, box, budget, distance_max=None, altitude_max=np.inf,
          max_steps=1000000, threads=None, slope=0.4, resolution=1e-2, tally=False):
    """The definition's loop over the CPU restatement -> dict(OUTPUTS) (tally: plus `tally` [n][4]:
    per ray the steps begun in the box's medium, those that met a voxel, those that met a face of
    the box in mid-step, and the pieces of all its walks)"""
    pos = np.array(position, dtype=np.float64, order="C").reshape(-1, 3)
    d = np.ascontiguousarray(direction, dtype=np.float64).reshape(-1, 3)
    n = pos.shape[0]
    rho = np.ascontiguousarray(density, dtype=np.float64)
    assert rho.shape == (geometry.n_layers + 1,)
    b = np.ascontiguousarray(budget, dtype=np.float64)
    dm = None if distance_max is None else np.ascontiguousarray(distance_max, dtype=np.float64)
    assert b.shape == (n,) and (dm is None or dm.shape == (n,))
    out = dict(position=pos, index=np.empty((n, 2), dtype=np.int32), depth=np.empty(n), distance=np.empty(n),
               n_steps=np.empty(n, dtype=np.int32), status=np.empty(n, dtype=np.int32))
    if tally:
        out["tally"] = np.zeros((n, 4), dtype=np.int32)
    threads = threads or min(64, os.cpu_count() or 1)
    g = None if box is None else box.struct()
    checker().advance_grid_loop(geometry.ref, C.c_double(slope), C.c_double(resolution), C.c_long(n), _p(pos), _p(d),
                                _p(rho), None if g is None else C.byref(g), _p(b), _p(dm), C.c_double(altitude_max),
                                C.c_int(max_steps), _p(out["index"]), _p(out["depth"]), _p(out["distance"]),
                                _p(out["n_steps"]), _p(out["status"]), _p(out.get("tally")), C.c_int(threads))
    return out


def walk_c(box, rho_out, m, p0, dr, L, R):
    """the C checker's walk over n segments -> x, f, stopped"""
    p0 = np.ascontiguousarray(p0, dtype=np.float64).reshape(-1, 3)
    n = p0.shape[0]
    dr = np.ascontiguousarray(dr, dtype=np.float64).reshape(-1, 3)
    full = [np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), (n,))) for v in (rho_out, L, R)]
    med = np.ascontiguousarray(np.broadcast_to(np.asarray(m, dtype=np.int32), (n,)))
    x, f, stopped = np.empty(n), np.empty(n), np.empty(n, dtype=np.int32)
    g = box.struct()
    checker().grid_depth_n(C.byref(g), C.c_long(n), _p(full[0]), _p(med), _p(p0), _p(dr), _p(full[1]), _p(full[2]),
                           _p(x), _p(f), _p(stopped))
    return x, f, stopped


# ---- the same loop over the compiled reference (oracle/_ref) ------------------

reference_stepper = AC.reference_stepper


def reference_loop(st, position, direction, density, box, budget, distance_max, altitude_max,
                   max_steps=1000000, record=None, tally=None):
    """include/turtle_amd.h's definition of turtle_stepper_advance_grid_n, statement for statement,
    over the reference's own turtle_stepper_step -> dict(OUTPUTS).  record: a list that gets, per
    ray, (d, X, m): path and depth after every step (and at the origin), and the medium each step
    began in.  tally: an int array [n][3] that gets, per ray, the steps begun in the box's medium,
    those that met a voxel and those that met a face of the box in mid-step."""
    from oracle import ref_ffi as R
    D = C.c_double
    step = R.lib().turtle_stepper_step
    n = position.shape[0]
    out = dict(position=np.empty((n, 3)), index=np.empty((n, 2), dtype=np.int32), depth=np.empty(n),
               distance=np.empty(n), n_steps=np.empty(n, dtype=np.int32), status=np.empty(n, dtype=np.int32))
    p, q = (D * 3)(), (D * 3)()
    alt, ds_ = D(), D()
    idx = (C.c_int * 2)()
    rho = [float(v) for v in density]
    for r in range(n):
        st.reset()
        p[:] = position[r]
        q[:] = direction[r]
        dr = [float(v) for v in direction[r]]
        B = float(budget[r])
        M = INF if distance_max is None else float(distance_max[r])
        assert step(st.h, p, None, None, None, C.byref(alt), None, None, idx) == 0
        X = d = 0.0
        steps = 0
        rec = ([0.0], [0.0], []) if record is not None else None
        while True:
            if idx[0] < 0:
                status = LEFT
                break
            if not X < B:
                status = SPENT
                break
            if not d < M:
                status = DISTANCE
                break
            if not alt.value < altitude_max:
                status = CEILING
                break
            if steps >= max_steps:
                status = MAX_STEPS
                break
            m, k = idx[0], idx[1]
            p0 = list(p)
            assert step(st.h, p, q, None, None, C.byref(alt), None, C.byref(ds_), idx) == 0
            ds = ds_.value
            far = d + ds >= M
            L = M - d if far else ds
            if L > ds:
                L = ds
            pieces = [] if (tally is not None and box is not None and m == box.medium) else None
            x, f, stopped = grid_depth(box, rho[m], m, p0, dr, L, B - X, pieces)
            if pieces is not None:
                hit = len(pieces) > 1
                tally[r, 0] += 1
                tally[r, 1] += hit
                tally[r, 2] += hit and (pieces[0][1] > 0 or (not stopped and pieces[-1][0] < L))
            if stopped or far:
                at = f if stopped else L
                for j in range(3):
                    p[j] = p0[j] + dr[j] * at
                if stopped:
                    X, d, status = B, d + f, SPENT
                else:
                    X, d, status = X + x, M, DISTANCE
                steps += 1
                idx[0], idx[1] = m, k
                break
            X, d, steps = X + x, d + ds, steps + 1
            if rec is not None:
                rec[0].append(d), rec[1].append(X), rec[2].append(m)
        if record is not None:
            record.append(tuple(np.array(v) for v in rec))
        out["position"][r] = p[:]
        out["index"][r] = idx[:]
        out["depth"][r], out["distance"][r], out["n_steps"][r], out["status"][r] = X, d, steps, status
    return out


# ---- budgets ------------------------------------------------------------------

def _step_start(origin, dr, s):
    return [origin[j] + dr[j] * s for j in range(3)]


def _stop_by_budget(profile, origin, dr, density, box, B, rho_max):
    """where along the ray the depth B is reached: by the recorded profile, and inside a step by the
    Python walk; past the end (by the budget left over, in the densest medium) where the budget
    outlasts the ray"""
    d, X, med = profile
    if not np.isfinite(B):
        return INF
    if B < X[-1]:
        i = int(np.searchsorted(X, B, side="right")) - 1          # X[i] <= B < X[i + 1]
        m = int(med[i])
        _, f, stopped = grid_depth(box, float(density[m]), m, _step_start(origin, dr, float(d[i])), dr,
                                   float(d[i + 1] - d[i]), B - float(X[i]))
        return float(d[i]) + f
    return float(d[-1]) + (B - float(X[-1])) / rho_max


def _depth_at(profile, origin, dr, density, box, s):
    d, X, med = profile
    if s >= d[-1]:
        return float(X[-1])
    i = int(np.searchsorted(d, s, side="right")) - 1
    m = int(med[i])
    x, _, _ = grid_depth(box, float(density[m]), m, _step_start(origin, dr, float(d[i])), dr, s - float(d[i]), INF)
    return float(X[i]) + x


def faces(box, origin, dr):
    """where the ray's line crosses the six planes of the box's faces, as distances from its origin"""
    out = []
    for a in range(3):
        s = sum(box._a[a][j] * (origin[j] - box._o[j]) for j in range(3))
        t = sum(box._a[a][j] * dr[j] for j in range(3))
        if t != 0:
            out += [(0 - s) / t, (box.n[a] * box._s[a] - s) / t]
    return np.array(out)


def inside(box, point):
    s = box.axis @ (np.asarray(point) - box.origin)
    return bool(((s > 0) & (s < np.array(box.n) * box.size)).all())


def budgets(rng, profiles, position, direction, index, offset, distance, density, box):
    """advance_exp_cases.budgets' recipe over the recorded profiles.  Per ray, D = the depth and T =
    the path at the end of its uncut run: budget = u D with u ~ U(0.05, 1.6), infinite with
    probability 0.05; distance_max = v T with v ~ U(0.05, 1.6), infinite with probability 0.6; a ray
    with T = 0 gets budget 1 and no limit.  A ray draws again until its two candidate stops are
    MARGIN x T from every crossing (the ragged (offset, distance) of crossings_cases), from its end
    and from each other, and its depth stop MARGIN x T from the planes of the box's faces
    (asserted).  -> dict(budget, distance_max, stop, depth, status, medium, margin, T, D)"""
    rho = np.asarray(density, dtype=np.float64)
    n = len(profiles)
    out = dict(budget=np.ones(n), distance_max=np.full(n, INF), stop=np.zeros(n), depth=np.zeros(n),
               status=np.empty(n, dtype=np.int32), medium=np.full(n, -1, dtype=np.int32),
               margin=np.full(n, INF), T=np.zeros(n), D=np.zeros(n))
    for r in range(n):
        prof = profiles[r]
        T, D = float(prof[0][-1]), float(prof[1][-1])
        out["T"][r], out["D"][r] = T, D
        geometry = LEFT if index[r, 0] < 0 else CEILING
        if T == 0:
            out["status"][r] = geometry
            continue
        origin, dr = [float(v) for v in position[r]], [float(v) for v in direction[r]]
        edges = np.concatenate(([0.0], distance[int(offset[r]):int(offset[r + 1])], [T]))
        planes = faces(box, origin, dr)
        while True:
            u, pu, v, pv = rng.uniform(0.05, 1.6), rng.random(), rng.uniform(0.05, 1.6), rng.random()
            B = INF if pu < 0.05 else u * D
            M = INF if pv < 0.6 else v * T
            s_b = _stop_by_budget(prof, origin, dr, rho, box, B, rho.max())
            gap = AC._margin(edges, T, s_b, M)
            if np.isfinite(s_b) and planes.size:
                gap = min(gap, float(np.abs(planes - s_b).min()))
            if gap >= MARGIN * T:
                break
        assert gap >= MARGIN * T
        stop = min(s_b, M, T)
        status = SPENT if (s_b <= T and s_b < M) else DISTANCE if M < T else geometry
        out["budget"][r], out["distance_max"][r], out["stop"][r], out["status"][r] = B, M, stop, status
        out["depth"][r] = B if status == SPENT else _depth_at(prof, origin, dr, rho, box, stop)
        if status in (SPENT, DISTANCE):
            out["medium"][r] = int(prof[2][int(np.searchsorted(prof[0], stop, side="right")) - 1])
        out["margin"][r] = gap / T
    return out
