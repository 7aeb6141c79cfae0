"""What the tests of turtle_stepper_advance_n share: the CPU checker (tests/c/advance_loop.c over the
oracle's restatement of turtle_stepper_step), the same loop over the compiled reference, the
densities, and the recipe that gives each ray of a batch a depth budget and a distance limit from
the batch's own traverse and crossings results.  The geometries are those of traverse_cases.
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

from oracle import ffi as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPENT, DISTANCE, LEFT, CEILING, MAX_STEPS = range(5)
OUTPUTS = ("position", "index", "depth", "distance", "n_steps", "status")
# rock, (water,) air, kg / m^3: a budget is then a column depth in kg / m^2
DENSITY = {2: np.array([2650.0, 1.205]), 3: np.array([2650.0, 1000.0, 1.205])}
SEED = 0xAD7A2CE
MARGIN = 1e-4          # x the ray's total path: what a stop keeps from everything that could swap it
BATCHES = tuple((case, recipe) for case in ("hgt", "two", "rough") for recipe in ("ground", "c2"))

_checker = None


def checker():
    """tests/c/advance_loop.c, compiled against oracle/libturtle_oracle.so"""
    global _checker
    if _checker is None:
        O.lib()  # builds libturtle_oracle.so if needed
        odir = os.path.join(ROOT, "oracle")
        out = tempfile.mkdtemp(prefix="turtle_advance_")
        so = os.path.join(out, "libadvance_loop.so")
        subprocess.check_call(["gcc", "-O2", "-std=gnu99", "-fPIC", "-ffp-contract=off", "-pthread",
                               "-shared", "-I" + odir, "-o", so,
                               os.path.join(ROOT, "tests", "c", "advance_loop.c"),
                               "-L" + odir, "-lturtle_oracle", "-Wl,-rpath," + odir, "-lm"])
        _checker = C.CDLL(so)
    return _checker


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def check(geometry, position, direction, density, budget, distance_max=None, altitude_max=np.inf,
          max_steps=1000000, threads=None, slope=0.4, resolution=1e-2):
    """The definition's loop over the CPU restatement -> dict(OUTPUTS)"""
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
    threads = threads or min(64, os.cpu_count() or 1)
    checker().advance_loop(geometry.ref, C.c_double(slope), C.c_double(resolution), C.c_long(n), _p(pos), _p(d),
                           _p(rho), _p(b), _p(dm), C.c_double(altitude_max), C.c_int(max_steps),
                           _p(out["index"]), _p(out["depth"]), _p(out["distance"]), _p(out["n_steps"]),
                           _p(out["status"]), C.c_int(threads))
    return out


# ---- the same loop over the compiled reference (oracle/_ref) ------------------

def reference_stepper(case, m):
    """the geometry of traverse_cases' `case` over the reference's map m, turtle_stepper_range_set(0)"""
    from oracle import ref_ffi as R
    st = R.RefStepper()
    st.range_set(0.0)
    if case == "two":
        for off in (-0.5, 0.0):
            st.add_layer()
            st.add_flat(off)
            st.add_map(m, off)
    else:
        st.add_map(m, 0.0)
    return st


def reference_loop(st, position, direction, density, budget, distance_max, altitude_max, max_steps=1000000):
    """include/turtle_amd.h's definition of turtle_stepper_advance_n, statement for statement, over
    the reference's own turtle_stepper_step -> dict(OUTPUTS)"""
    from oracle import ref_ffi as R
    D = C.c_double
    step = R.lib().turtle_stepper_step
    n = position.shape[0]
    out = dict(position=np.empty((n, 3)), index=np.empty((n, 2), dtype=np.int32), depth=np.empty(n),
               distance=np.empty(n), n_steps=np.empty(n, dtype=np.int32), status=np.empty(n, dtype=np.int32))
    p, q = (D * 3)(), (D * 3)()
    alt, ds_ = D(), D()
    idx = (C.c_int * 2)()
    for r in range(n):
        st.reset()
        p[:] = position[r]
        q[:] = direction[r]
        dr = [float(v) for v in direction[r]]
        B = float(budget[r])
        M = float("inf") if distance_max is None else float(distance_max[r])
        assert step(st.h, p, None, None, None, C.byref(alt), None, None, idx) == 0
        X = d = 0.0
        steps = 0
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
            rho = float(density[m])
            x = rho * ds
            spent, far = X + x >= B, d + ds >= M
            if spent or far:
                f, status = ds, SPENT
                if far:
                    f, status = M - d, DISTANCE
                if spent:
                    fs = (B - X) / rho
                    if fs <= f:
                        f, status = fs, SPENT
                if f > ds:
                    f = ds
                for j in range(3):
                    p[j] = p0[j] + dr[j] * f
                if status == SPENT:
                    X, d = B, d + f
                else:
                    X, d = X + rho * f, M
                steps += 1
                idx[0], idx[1] = m, k
                break
            X, d, steps = X + x, d + ds, steps + 1
        out["position"][r] = p[:]
        out["index"][r] = idx[:]
        out["depth"][r], out["distance"][r], out["n_steps"][r], out["status"][r] = X, d, steps, status
    return out


# ---- budgets ------------------------------------------------------------------

def _profile(c, med, T, last, rho):
    """a ray's column depth along its path, piecewise linear: the edges (0, its crossings' distances,
    its end), the density of each piece (the medium a crossing left; after the last one the medium
    it entered, or with no crossing the ray's only medium `last`; 0 outside the data) and the depth
    at each edge"""
    edges = np.concatenate(([0.0], c, [max(T, c[-1]) if c.size else T]))
    m = np.concatenate((med[:, 0], [med[-1, 1] if c.size else last]))
    r = np.where(m >= 0, rho[np.maximum(m, 0)], 0.0)
    return edges, r, np.concatenate(([0.0], np.cumsum(r * np.diff(edges))))


def _candidates(edges, r, depth, D, T, B, M, rho_max):
    """where the budget and the limit would stop the ray, as distances from its origin: (s_b, s_m).
    s_b is past the end (by the budget left over, in the densest medium) where the budget outlasts
    the ray, inf where it is infinite; s_m is M itself"""
    if not np.isfinite(B):
        s_b = np.inf
    elif B < depth[-1]:
        i = int(np.searchsorted(depth, B, side="right")) - 1      # depth[i] <= B < depth[i + 1]
        s_b = edges[i] + (B - depth[i]) / r[i]
    else:
        s_b = max(T, edges[-1]) + (B - min(D, depth[-1])) / rho_max
    return s_b, M


def _margin(edges, T, s_b, s_m):
    """the least distance between a candidate stop and a crossing, the ray's end or the other
    candidate (inf: no finite candidate)"""
    fixed = np.concatenate((edges[1:], [T]))
    gap = np.inf
    for s in (s_b, s_m):
        if np.isfinite(s):
            gap = min(gap, float(np.abs(fixed - s).min()))
    if np.isfinite(s_b) and np.isfinite(s_m):
        gap = min(gap, abs(s_b - s_m))
    return gap


def budgets(rng, length, index, offset, distance, media, density):
    """The recipe: a budget and a distance limit for every ray of a batch whose traverse gave
    `length` [media][n] and `index` [n][2] and whose crossings are the ragged (offset, distance,
    media) of crossings_cases, with the densities `density`.  Per ray, D = sum of density x length
    its full depth and T its total path: budget = u D with u ~ U(0.05, 1.6), infinite with
    probability 0.05; distance_max = v T with v ~ U(0.05, 1.6), infinite with probability 0.6; a ray
    with T = 0 gets budget 1 and no limit.  A ray draws again until its two candidate stops are
    MARGIN x T from every crossing, from its end and from each other (asserted), so that no 1e-6
    of T can swap what stops it.  -> dict(budget, distance_max, stop, depth, status, margin): where
    and why the ray stops by numpy, float64, piecewise linear over its crossings, and the margin
    over T."""
    rho = np.asarray(density, dtype=np.float64)
    n = length.shape[1]
    T_all = length.sum(axis=0)
    D_all = (rho[:, None] * length).sum(axis=0)
    out = dict(budget=np.ones(n), distance_max=np.full(n, np.inf), stop=np.zeros(n), depth=np.zeros(n),
               status=np.empty(n, dtype=np.int32), margin=np.full(n, np.inf))
    for r in range(n):
        T, D = float(T_all[r]), float(D_all[r])
        geometry = LEFT if index[r, 0] < 0 else CEILING
        if T == 0:
            out["status"][r] = geometry
            continue
        rows = slice(int(offset[r]), int(offset[r + 1]))
        edges, dens, depth = _profile(distance[rows], media[rows], T, int(np.argmax(length[:, r])), rho)
        while True:
            u, pu, v, pv = rng.uniform(0.05, 1.6), rng.random(), rng.uniform(0.05, 1.6), rng.random()
            B = np.inf if pu < 0.05 else u * D
            M = np.inf if pv < 0.6 else v * T
            s_b, s_m = _candidates(edges, dens, depth, D, T, B, M, rho.max())
            gap = _margin(edges, T, s_b, s_m)
            if gap >= MARGIN * T:
                break
        assert gap >= MARGIN * T
        end = edges[-1]
        stop = min(s_b, s_m, end)
        status = SPENT if (s_b <= end and s_b < s_m) else DISTANCE if s_m < end else geometry
        out["budget"][r], out["distance_max"][r], out["stop"][r], out["status"][r] = B, M, stop, status
        out["depth"][r] = B if status == SPENT else np.interp(stop, edges, depth)
        out["margin"][r] = gap / T
    return out


def golden_budgets(traverse, crossings):
    """the recipe over the six batches of traverse.npz and crossings.npz, in BATCHES' order with one
    generator: {(case, recipe): budgets(...) plus density}"""
    rng = np.random.default_rng(SEED)
    out = {}
    for case, recipe in BATCHES:
        k = f"{case}_{recipe}_"
        length = traverse[k + "length"]
        density = DENSITY[length.shape[0]]
        out[case, recipe] = budgets(rng, length, traverse[k + "index"], crossings[k + "offset"],
                                    crossings[k + "distance"], crossings[k + "media"], density)
        out[case, recipe]["density"] = density
    return out
