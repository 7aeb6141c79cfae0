"""What the tests of turtle_stepper_advance_exp_n share: the CPU checker (tests/c/advance_exp_loop.c
over the oracle's restatement of turtle_stepper_step), the same loop over the compiled reference,
the densities and scale heights, and the recipe that gives each ray of a batch a depth budget and a
distance limit.  The geometries, rays and crossings are those of traverse_cases / advance_cases; what
changes against advance_cases is the profile a budget is drawn from: the column depth along a ray
is no longer piecewise linear between its crossings, so it comes from an uncut run of the same loop
that records (d, X) after every step.
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
DENSITY = AC.DENSITY          # rock, (water,) air at altitude 0, kg / m^3
# rock (and the layer between) uniform, air falling by e every 8400 m
SCALE_HEIGHT = {2: np.array([INF, 8400.0]), 3: np.array([INF, INF, 8400.0])}
SEED = 0xE8BAD7A
MARGIN = AC.MARGIN
BATCHES = AC.BATCHES

_checker = None


def checker():
    """tests/c/advance_exp_loop.c, compiled against oracle/libturtle_oracle.so"""
    global _checker
    if _checker is None:
        O.lib()  # builds libturtle_oracle.so if needed
        odir = os.path.join(ROOT, "oracle")
        out = tempfile.mkdtemp(prefix="turtle_advance_exp_")
        so = os.path.join(out, "libadvance_exp_loop.so")
        subprocess.check_call(["gcc", "-O2", "-std=gnu99", "-fPIC", "-ffp-contract=off", "-pthread",
                               "-shared", "-I" + odir, "-o", so,
                               os.path.join(ROOT, "tests", "c", "advance_exp_loop.c"),
                               "-L" + odir, "-lturtle_oracle", "-Wl,-rpath," + odir, "-lm"])
        _checker = C.CDLL(so)
    return _checker


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def check(geometry, position, direction, density, scale_height, budget, distance_max=None,
          altitude_max=np.inf, max_steps=1000000, threads=None, slope=0.4, resolution=1e-2):
    """The definition's loop over the CPU restatement -> dict(OUTPUTS)"""
    pos = np.array(position, dtype=np.float64, order="C").reshape(-1, 3)
    d = np.ascontiguousarray(direction, dtype=np.float64).reshape(-1, 3)
    n = pos.shape[0]
    rho = np.ascontiguousarray(density, dtype=np.float64)
    sh = None if scale_height is None else np.ascontiguousarray(scale_height, dtype=np.float64)
    assert rho.shape == (geometry.n_layers + 1,) and (sh is None or sh.shape == rho.shape)
    b = np.ascontiguousarray(budget, dtype=np.float64)
    dm = None if distance_max is None else np.ascontiguousarray(distance_max, dtype=np.float64)
    assert b.shape == (n,) and (dm is None or dm.shape == (n,))
    out = dict(position=pos, index=np.empty((n, 2), dtype=np.int32), depth=np.empty(n), distance=np.empty(n),
               n_steps=np.empty(n, dtype=np.int32), status=np.empty(n, dtype=np.int32))
    threads = threads or min(64, os.cpu_count() or 1)
    checker().advance_exp_loop(geometry.ref, C.c_double(slope), C.c_double(resolution), C.c_long(n), _p(pos), _p(d),
                               _p(rho), _p(sh), _p(b), _p(dm), C.c_double(altitude_max), C.c_int(max_steps),
                               _p(out["index"]), _p(out["depth"]), _p(out["distance"]), _p(out["n_steps"]),
                               _p(out["status"]), C.c_int(threads))
    return out


# ---- the step's law, in Python floats (libm's exp, expm1 and log1p: the C checker's) ----

def law(rho, H, a0, a1, ds):
    """(c, w) of a step of length ds from altitude a0 to a1 in a medium (rho, H)"""
    if H is None or H == INF:
        return rho, 0.0
    return rho * math.exp(-a0 / H), -((a1 - a0) / H) / ds


def S(c, w, f):
    """the depth of the step's first f metres"""
    return c * f if w * f == 0 else c * math.expm1(w * f) / w


def reach(c, w, R):
    """how far into the step the depth R lasts (NaN: never; as the C's log1p gives it)"""
    if w == 0:
        return R / c if c != 0 else (math.nan if R == 0 else math.copysign(INF, R))
    y = R * w / c if c != 0 else math.nan
    if not y > -1:
        return math.nan if y != -1 else -INF / w
    return math.log1p(y) / w


# ---- the same loop over the compiled reference (oracle/_ref) ------------------

reference_stepper = AC.reference_stepper


def reference_loop(st, position, direction, density, scale_height, budget, distance_max, altitude_max,
                   max_steps=1000000, record=None):
    """include/turtle_amd.h's definition of turtle_stepper_advance_exp_n, statement for statement,
    over the reference's own turtle_stepper_step -> dict(OUTPUTS).  record: a list that gets, per
    ray, (d, X, alt, m): path, depth and altitude after every step (and at the origin), and the
    medium each step began in."""
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
        M = INF if distance_max is None else float(distance_max[r])
        assert step(st.h, p, None, None, None, C.byref(alt), None, None, idx) == 0
        X = d = 0.0
        steps = 0
        rec = ([0.0], [0.0], [alt.value], []) if record is not None else None
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
            a0 = alt.value
            assert step(st.h, p, q, None, None, C.byref(alt), None, C.byref(ds_), idx) == 0
            a1 = alt.value
            ds = ds_.value
            c, w = law(float(density[m]), None if scale_height is None else float(scale_height[m]), a0, a1, ds)
            x = S(c, w, ds)
            spent, far = X + x >= B, d + ds >= M
            if spent or far:
                f, status = ds, SPENT
                if far:
                    f, status = M - d, DISTANCE
                if spent:
                    fs = reach(c, w, B - X)
                    if fs <= f:
                        f, status = fs, SPENT
                if f > ds:
                    f = ds
                for j in range(3):
                    p[j] = p0[j] + dr[j] * f
                if status == SPENT:
                    X, d = B, d + f
                else:
                    X, d = X + S(c, w, f), M
                steps += 1
                idx[0], idx[1] = m, k
                break
            X, d, steps = X + x, d + ds, steps + 1
            if rec is not None:
                rec[0].append(d), rec[1].append(X), rec[2].append(a1), rec[3].append(m)
        if record is not None:
            record.append(tuple(np.array(v) for v in rec))
        out["position"][r] = p[:]
        out["index"][r] = idx[:]
        out["depth"][r], out["distance"][r], out["n_steps"][r], out["status"][r] = X, d, steps, status
    return out


# ---- budgets ------------------------------------------------------------------

def _stop_by_budget(profile, density, scale_height, B, rho_max):
    """where along the ray the depth B is reached, by the recorded profile and the step's law; past
    the end (by the budget left over, in the densest medium) where the budget outlasts the ray"""
    d, X, alt, med = profile
    if not np.isfinite(B):
        return INF
    if B < X[-1]:
        i = int(np.searchsorted(X, B, side="right")) - 1          # X[i] <= B < X[i + 1]
        m = int(med[i])
        c, w = law(float(density[m]), float(scale_height[m]), float(alt[i]), float(alt[i + 1]),
                   float(d[i + 1] - d[i]))
        return float(d[i]) + reach(c, w, B - float(X[i]))
    return float(d[-1]) + (B - float(X[-1])) / rho_max


def _depth_at(profile, density, scale_height, s):
    d, X, alt, med = profile
    if s >= d[-1]:
        return float(X[-1])
    i = int(np.searchsorted(d, s, side="right")) - 1
    m = int(med[i])
    c, w = law(float(density[m]), float(scale_height[m]), float(alt[i]), float(alt[i + 1]), float(d[i + 1] - d[i]))
    return float(X[i]) + S(c, w, s - float(d[i]))


def budgets(rng, profiles, index, offset, distance, density, scale_height):
    """advance_cases.budgets' recipe over recorded profiles.  Per ray, D = the depth and T = the path
    at the end of its uncut run: budget = u D with u ~ U(0.05, 1.6), infinite with probability 0.05;
    distance_max = v T with v ~ U(0.05, 1.6), infinite with probability 0.6; a ray with T = 0 gets
    budget 1 and no limit.  A ray draws again until its two candidate stops are MARGIN x T from every
    crossing (the ragged (offset, distance) of crossings_cases), from its end and from each other
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
        edges = np.concatenate(([0.0], distance[int(offset[r]):int(offset[r + 1])], [T]))
        while True:
            u, pu, v, pv = rng.uniform(0.05, 1.6), rng.random(), rng.uniform(0.05, 1.6), rng.random()
            B = INF if pu < 0.05 else u * D
            M = INF if pv < 0.6 else v * T
            s_b = _stop_by_budget(prof, rho, scale_height, B, rho.max())
            gap = AC._margin(edges, T, s_b, M)
            if gap >= MARGIN * T:
                break
        assert gap >= MARGIN * T
        stop = min(s_b, M, T)
        status = SPENT if (s_b <= T and s_b < M) else DISTANCE if M < T else geometry
        out["budget"][r], out["distance_max"][r], out["stop"][r], out["status"][r] = B, M, stop, status
        out["depth"][r] = B if status == SPENT else _depth_at(prof, rho, scale_height, stop)
        if status in (SPENT, DISTANCE):
            out["medium"][r] = int(prof[3][int(np.searchsorted(prof[0], stop, side="right")) - 1])
        out["margin"][r] = gap / T
    return out
