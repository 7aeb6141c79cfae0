"""turtle_stepper_advance_exp_n on the GPU: rays advanced by a column-depth budget and a distance
limit through media whose density falls with altitude, against the reference's loop
(tests/golden/advance_exp.npz), turtle_stepper_advance_n (uniform media: the same bits), closed forms
over flat layers, and the example.

The bar against the reference, in both arithmetics, is test_gpu_advance's: the same status, final
medium and step count, depth within BAR of the ray's full depth, distance and position within BAR
of its total path."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import turtle_amd as TA

import advance_exp_cases as AE
import traverse_cases as TC
from test_gpu_advance import math, off_the_bar, on_the_ray, rays, same_bits, steppers  # noqa: F401
from test_gpu_traverse import BAR, OUTSIDE as TRAVERSE_OUTSIDE

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = AE.OUTPUTS
INF = float("inf")
EPS = 2.0 ** -53


def batch(golden, case, recipe):
    g, a = golden("traverse"), golden("advance_exp")
    k = f"{case}_{recipe}_"
    out = {name: g[k + name] for name in ("position", "direction", "length")}
    out.update(ceiling=float(g[k + "ceiling"]))
    out.update({name: a[k + name] for name in ("budget", "distance_max", "density", "scale_height", "T", "D")})
    out["ref"] = {name: a[k + name] for name in KEYS}
    return out


def raw(st, name, n, pos, d, rho, sh, budget, limit, ceiling, max_steps=1000000):
    """the C call itself over numpy arrays (sh: None for turtle_stepper_advance_n, or an array, or
    "null": turtle_stepper_advance_exp_n with scale_height = NULL); outputs prefilled with garbage"""
    out = dict(position=np.array(pos, dtype=np.float64), index=np.full((n, 2), -9, np.int32),
               depth=np.full(n, np.nan), distance=np.full(n, -7.0), n_steps=np.full(n, -5, np.int32),
               status=np.full(n, -3, np.int32))
    p = {k: v.ctypes.data_as(C.c_void_p) for k, v in out.items()}
    keep = [np.ascontiguousarray(a, dtype=np.float64) for a in (d, rho, budget)]
    D, RHO, B = (a.ctypes.data_as(C.c_void_p) for a in keep)
    lim = None if limit is None else np.ascontiguousarray(limit, dtype=np.float64)
    LIM = None if lim is None else lim.ctypes.data_as(C.c_void_p)
    tail = (B, LIM, C.c_double(ceiling), max_steps, p["index"], p["depth"], p["distance"], p["n_steps"],
            p["status"], TA.HOST)
    if name == "turtle_stepper_advance_n":
        rc = TA.lib().turtle_stepper_advance_n(st.h, C.c_long(n), p["position"], D, RHO, *tail)
    else:
        h = None if sh is None else np.ascontiguousarray(sh, dtype=np.float64)
        H = None if h is None else h.ctypes.data_as(C.c_void_p)
        rc = TA.lib().turtle_stepper_advance_exp_n(st.h, C.c_long(n), p["position"], D, RHO, H, *tail)
    assert rc == 0
    return out


# ---- 1. parity with the reference ---------------------------------------------

@pytest.mark.parametrize("recipe", ["ground", "c2"])
@pytest.mark.parametrize("case", TC.CASES)
def test_advance_exp_matches_the_reference(steppers, golden, math, case, recipe):
    b = batch(golden, case, recipe)
    st = steppers[case]
    assert st.media == b["density"].shape[0]
    t = st.advance(b["position"].copy(), b["direction"], b["density"], b["budget"], b["distance_max"], b["ceiling"],
                   scale_height=b["scale_height"])
    ids = off_the_bar(t, b["ref"], b["D"], b["T"])
    for r in ids:
        print(f"{case} {recipe} {math}: ray {r} status {t['status'][r]} / {b['ref']['status'][r]}, steps "
              f"{t['n_steps'][r]} / {b['ref']['n_steps'][r]}, depth off {abs(t['depth'][r] - b['ref']['depth'][r]):.3e} "
              f"of {b['D'][r]:.3e}, distance off {abs(t['distance'][r] - b['ref']['distance'][r]):.3e} of {b['T'][r]:.3e}")
    ok = np.setdiff1d(np.arange(t["status"].shape[0]), ids)
    print(f"{case} {recipe} {math}: depth off by at most {np.max(np.abs(t['depth'] - b['ref']['depth'])[ok] / np.maximum(b['D'][ok], 1e-300)):.2e} D, "
          f"distance by {np.max(np.abs(t['distance'] - b['ref']['distance'])[ok] / np.maximum(b['T'][ok], 1e-300)):.2e} T")
    # the only rays excused: those that miss traverse's own bar in this batch and arithmetic
    assert set(ids.tolist()) <= set(TRAVERSE_OUTSIDE.get((f"{case}_{recipe}", math), [])), ids.tolist()
    assert len(ids) <= 3
    on_the_ray(t, b["position"], b["direction"], b["T"])
    s = st.trace_stats()
    assert s["rays"] == t["status"].shape[0] and s["steps"] == int(t["n_steps"].sum()) and s["capped"] == 0
    assert st.rounds == 1
    # a ray the budget stopped has spent it to the bit; one the limit stopped stands at the limit
    spent, far = t["status"] == AE.SPENT, t["status"] == AE.DISTANCE
    assert np.array_equal(t["depth"][spent], b["budget"][spent])
    assert np.array_equal(t["distance"][far], b["distance_max"][far])
    # no cut: status, position and step count are traverse's
    uncut = t["status"] >= AE.LEFT
    tr = st.traverse(b["position"].copy(), b["direction"], b["ceiling"])
    for k in ("position", "index", "n_steps"):
        assert np.array_equal(tr[k][uncut], t[k][uncut]), k


# ---- 2. reduction to advance_n ------------------------------------------------

@pytest.mark.parametrize("case", TC.CASES)
def test_uniform_scale_heights_are_advance_n(steppers, golden, math, case):
    st = steppers[case]
    g, a = golden("traverse"), golden("advance")
    for recipe in ("ground", "c2"):
        k = f"{case}_{recipe}_"
        pos, d, ceiling = g[k + "position"], g[k + "direction"], float(g[k + "ceiling"])
        rho, budget, limit = a[k + "density"], a[k + "budget"], a[k + "distance_max"]
        n = pos.shape[0]
        plain = st.advance(pos.copy(), d, rho, budget, limit, ceiling)
        s = st.trace_stats()
        # every scale height HUGE_VAL: the LAW instance, every lane past the law
        t = st.advance(pos.copy(), d, rho, budget, limit, ceiling, scale_height=np.full(st.media, INF))
        assert st.trace_stats() == s and st.rounds == 1
        same_bits(plain, t)
        # scale_height = NULL through the new call: the instance of advance_n
        t = raw(st, "turtle_stepper_advance_exp_n", n, pos, d, rho, None, budget, limit, ceiling)
        assert st.trace_stats() == s
        same_bits(plain, t)
        # air uniform, rock not: no bit changes for a ray that never enters the rock
        sh = np.full(st.media, INF)
        sh[0] = 5000.0
        t = st.advance(pos.copy(), d, rho, budget, limit, ceiling, scale_height=sh)
        no_rock = g[k + "length"][0] == 0
        assert no_rock.sum() >= (150 if recipe == "ground" else 16), (k, int(no_rock.sum()))
        same_bits(rays(plain, no_rock), rays(t, no_rock))
        in_rock = (plain["status"] == AE.SPENT) & (plain["index"][:, 0] == 0)
        assert in_rock.sum() > 15 and (t["distance"][in_rock] != plain["distance"][in_rock]).any()


# ---- 3. closed forms over flat layers ------------------------------------------

# What the altitude of a sample may be off by: the FAST transform is within 3e-9 m of the strict one
# (include/turtle_amd_device.h), which is good to a few ulp of the Earth's radius.
ALT_ERR = 3e-9 + 4 * np.spacing(6.4e6)
LOCATED = 1e-8          # a crossing is located to 1e-8 m: the step that crosses runs that far into the next medium


def depth_tolerance(n_steps, n_cross, rho0, depth, a_over_h):
    """The bound on |depth - closed form| of a vertical ray, from the run's own step count.  The depth
    of a step is rho H (exp(-a0 / H) - exp(-a1 / H)) x ds / (a1 - a0) exactly: the sum telescopes in
    the altitudes the kernel saw, and each step is off by (a) ds / (a1 - a0), which is 1 but for the
    error of the two altitudes, 2 ALT_ERR / ds of a step worth at most rho0 ds; (b) the rounding of
    its arithmetic: 1 / H, the exponent (an error of 1 ulp in a / H is a / H ulp of exp), exp and
    expm1 (1 ulp each), six products and quotients and the sum, at half an ulp each: 6 + a / H ulp,
    taken of the whole depth.  The first and last altitudes are off by ALT_ERR each (and the last
    by the rounding of the reported distance, n ulp of it, below ALT_ERR), and a crossing by
    LOCATED, at a density of at most rho0."""
    ulps = 6.0 + np.ceil(a_over_h)
    return (n_steps * 2 * ALT_ERR * rho0 + n_steps * ulps * 2 * EPS * depth + 2 * ALT_ERR * rho0
            + n_cross * LOCATED * rho0)


def column(rho0, H, a0, a1):
    """rho0 H (exp(-a0 / H) - exp(-a1 / H)), without the cancellation"""
    return -rho0 * H * np.exp(-a0 / H) * np.expm1(-(a1 - a0) / H)


@pytest.fixture(scope="module")
def flats():
    """one flat layer at altitude 0 (rock, air), and two at 0 and 10 000 m (rock and two bands of air)"""
    one, two = TA.Stepper(), TA.Stepper()
    one.add_flat(0.0)
    for off in (0.0, 10000.0):
        two.add_layer()
        two.add_flat(off)
    yield one, two
    one.destroy()
    two.destroy()


def vertical(a0, up, lat0=45.0):
    n = len(a0)
    lat, lon = lat0 + 0.01 * np.arange(n), 3.0 + 0.02 * np.arange(n)
    pos = TA.ecef_from_geodetic(lat, lon, np.asarray(a0, dtype=np.float64))
    d = TA.ecef_from_horizontal(lat, lon, np.zeros(n), np.where(up, 90.0, -90.0))
    return np.ascontiguousarray(pos), np.ascontiguousarray(d)


def test_closed_form_one_medium(flats, math):
    st, _ = flats
    assert st.media == 2
    rho, sh = np.array([2650.0, 1.205]), np.array([INF, 8400.0])
    rho0, H = rho[1], sh[1]
    # ---- up to a ceiling ----
    a0 = np.array([0.5, 3.0, 10.0, 137.0, 1000.0, 2962.0, 5000.0, 8400.0, 15000.0, 29000.0])
    n = a0.shape[0]
    ceiling = 30000.0
    pos, d = vertical(a0, np.ones(n, bool))
    t = st.advance(pos.copy(), d, rho, np.full(n, INF), None, ceiling, scale_height=sh)
    assert (t["status"] == AE.CEILING).all() and (t["index"][:, 0] == 1).all() and (t["n_steps"] > 0).all()
    a1 = a0 + t["distance"]
    assert (a1 >= ceiling - ALT_ERR).all()
    want = column(rho0, H, a0, a1)
    tol = depth_tolerance(t["n_steps"], 0, rho0, want, a1 / H)
    print(f"{math}: up, steps {t['n_steps'].tolist()}, off {(np.abs(t['depth'] - want) / tol).max():.3f} of the bound, "
          f"{(np.abs(t['depth'] - want) / want).max():.2e} of the depth")
    assert (np.abs(t["depth"] - want) <= tol).all()
    # ... which is not what one density gives
    u = st.advance(pos.copy(), d, rho, np.full(n, INF), None, ceiling)
    same_bits(u, t, ("position", "index", "distance", "n_steps", "status"))
    assert (u["depth"] > 1.1 * t["depth"]).all()
    # ---- SPENT, up: the budget a fraction of the depth to the ceiling ----
    for frac in (0.003, 0.5, 0.97):
        B = frac * want
        s = st.advance(pos.copy(), d, rho, B, None, ceiling, scale_height=sh)
        assert (s["status"] == AE.SPENT).all() and np.array_equal(s["depth"], B)
        stop = -H * np.log1p(-B / (rho0 * H * np.exp(-a0 / H)))
        # a depth error dX moves the stop by dX / (the density there); the distance adds n roundings
        there = rho0 * np.exp(-(a0 + stop) / H)
        tol_s = (depth_tolerance(s["n_steps"], 0, rho0, B, (a0 + stop) / H) / there
                 + s["n_steps"] * 2 * EPS * stop + 2 * ALT_ERR)
        print(f"{math}: spent {frac}, off {(np.abs(s['distance'] - stop) / tol_s).max():.3f} of the bound")
        assert (np.abs(s["distance"] - stop) <= tol_s).all()
        on_the_ray(s, pos, d, s["distance"])
    # ---- DISTANCE, up ----
    for frac in (0.01, 0.6):
        M = frac * t["distance"]
        f = st.advance(pos.copy(), d, rho, np.full(n, INF), M, ceiling, scale_height=sh)
        assert (f["status"] == AE.DISTANCE).all() and np.array_equal(f["distance"], M)
        want_m = column(rho0, H, a0, a0 + M)
        tol_m = depth_tolerance(f["n_steps"], 0, rho0, want_m, (a0 + M) / H)
        print(f"{math}: distance {frac}, off {(np.abs(f['depth'] - want_m) / tol_m).max():.3f} of the bound")
        assert (np.abs(f["depth"] - want_m) <= tol_m).all()
    # ---- down, from high up towards the ground: stopped in the air ----
    top = np.array([29000.0, 20000.0, 8400.0, 3000.0, 1200.0, 40.0])
    n = top.shape[0]
    pos, d = vertical(top, np.zeros(n, bool))
    to_ground = column(rho0, H, np.zeros(n), top)             # (the depth from the ground up to the start)
    for frac in (0.02, 0.5, 0.98):
        B = frac * to_ground
        s = st.advance(pos.copy(), d, rho, B, None, INF, scale_height=sh)
        assert (s["status"] == AE.SPENT).all() and (s["index"][:, 0] == 1).all() and np.array_equal(s["depth"], B)
        stop = H * np.log1p(B / (rho0 * H * np.exp(-top / H)))
        there = rho0 * np.exp(-(top - stop) / H)
        tol_s = (depth_tolerance(s["n_steps"], 0, rho0, B, top / H) / there + s["n_steps"] * 2 * EPS * stop
                 + 2 * ALT_ERR)
        print(f"{math}: down, spent {frac}, steps {s['n_steps'].tolist()}, off "
              f"{(np.abs(s['distance'] - stop) / tol_s).max():.3f} of the bound")
        assert (np.abs(s["distance"] - stop) <= tol_s).all()
        M = frac * top
        f = st.advance(pos.copy(), d, rho, np.full(n, INF), M, INF, scale_height=sh)
        assert (f["status"] == AE.DISTANCE).all() and np.array_equal(f["distance"], M)
        want_m = column(rho0, H, top - M, top)
        tol_m = depth_tolerance(f["n_steps"], 0, rho0, want_m, top / H)
        assert (np.abs(f["depth"] - want_m) <= tol_m).all()
    # through the ground into uniform rock: the air's column, then 2650 kg/m^3 to the bit of the budget
    B = to_ground + 2650.0 * 10.0
    s = st.advance(pos.copy(), d, rho, B, None, INF, scale_height=sh)
    assert (s["status"] == AE.SPENT).all() and (s["index"][:, 0] == 0).all() and np.array_equal(s["depth"], B)
    tol_s = (depth_tolerance(s["n_steps"], 1, 2650.0, B, top / H) / 2650.0 + s["n_steps"] * 2 * EPS * (top + 10.0)
             + 2 * ALT_ERR)
    assert (np.abs(s["distance"] - (top + 10.0)) <= tol_s).all()


def test_closed_form_band_pair(flats, math):
    """two bands of air, each with its own density at altitude 0 and its own scale height"""
    _, st = flats
    assert st.media == 3
    rho, sh = np.array([2650.0, 1.205, 0.9]), np.array([INF, 8400.0, 6300.0])
    hb = 10000.0
    a0 = np.array([1.0, 250.0, 4000.0, 9000.0, 9999.0])
    n = a0.shape[0]
    ceiling = 25000.0
    pos, d = vertical(a0, np.ones(n, bool))
    t = st.advance(pos.copy(), d, rho, np.full(n, INF), None, ceiling, scale_height=sh)
    assert (t["status"] == AE.CEILING).all() and (t["index"][:, 0] == 2).all()
    a1 = a0 + t["distance"]
    low, high = column(rho[1], sh[1], a0, hb), column(rho[2], sh[2], hb, a1)
    want = low + high
    tol = depth_tolerance(t["n_steps"], 1, rho[1], want, a1 / sh[2])
    print(f"{math}: bands, steps {t['n_steps'].tolist()}, off {(np.abs(t['depth'] - want) / tol).max():.3f} of the bound")
    assert (np.abs(t["depth"] - want) <= tol).all()
    # SPENT in the upper band: the lower band's column, then the upper band's law
    B = low + 0.5 * high
    s = st.advance(pos.copy(), d, rho, B, None, ceiling, scale_height=sh)
    assert (s["status"] == AE.SPENT).all() and (s["index"][:, 0] == 2).all() and np.array_equal(s["depth"], B)
    stop = (hb - a0) - sh[2] * np.log1p(-(0.5 * high) / (rho[2] * sh[2] * np.exp(-hb / sh[2])))
    there = rho[2] * np.exp(-(a0 + stop) / sh[2])
    tol_s = (depth_tolerance(s["n_steps"], 1, rho[1], B, (a0 + stop) / sh[2]) / there + s["n_steps"] * 2 * EPS * stop
             + 2 * ALT_ERR)
    assert (np.abs(s["distance"] - stop) <= tol_s).all()
    # DISTANCE in the lower band, and down from the upper band into the lower one
    M = 0.5 * (hb - a0)
    f = st.advance(pos.copy(), d, rho, np.full(n, INF), M, ceiling, scale_height=sh)
    assert (f["status"] == AE.DISTANCE).all() and (f["index"][:, 0] == 1).all()
    want_m = column(rho[1], sh[1], a0, a0 + M)
    assert (np.abs(f["depth"] - want_m) <= depth_tolerance(f["n_steps"], 0, rho[1], want_m, hb / sh[1])).all()
    top = np.array([24000.0, 15000.0, 10001.0])
    pos, d = vertical(top, np.zeros(3, bool))
    M = top - 5000.0
    f = st.advance(pos.copy(), d, rho, np.full(3, INF), M, INF, scale_height=sh)
    assert (f["status"] == AE.DISTANCE).all() and (f["index"][:, 0] == 1).all()
    want_m = column(rho[2], sh[2], hb, top) + column(rho[1], sh[1], 5000.0, hb)
    assert (np.abs(f["depth"] - want_m) <= depth_tolerance(f["n_steps"], 1, rho[1], want_m, top / sh[2])).all()


# ---- 4. edges -------------------------------------------------------------------

def test_advance_exp_edges(steppers, golden, math):
    st = steppers["hgt"]
    b = batch(golden, "hgt", "c2")
    pos, d, rho, sh, ceiling = b["position"][:64], b["direction"][:64], b["density"], b["scale_height"], b["ceiling"]
    n = 64
    assert (b["T"][:n] > 0).all()
    # a budget of 0, NaN or negative: spent at the origin; a limit of 0: reached there
    for budget, limit, status in ((0.0, None, AE.SPENT), (np.nan, None, AE.SPENT), (-1.0, None, AE.SPENT),
                                  (INF, 0.0, AE.DISTANCE), (0.0, 0.0, AE.SPENT)):
        t = st.advance(pos.copy(), d, rho, np.full(n, budget), None if limit is None else np.full(n, limit), ceiling,
                       scale_height=sh)
        assert (t["status"] == status).all() and (t["n_steps"] == 0).all()
        assert np.array_equal(t["position"], pos) and (t["depth"] == 0).all() and (t["distance"] == 0).all()
        assert (t["index"][:, 0] == 1).all()                 # (in the air, 500 m above the ground)
    # a start outside the data, and one above the ceiling: rays [-32:-16] and [-16:] of the recipe
    tail = st.advance(b["position"][-32:].copy(), b["direction"][-32:], rho, np.full(32, 1.0), np.full(32, 1.0), ceiling,
                      scale_height=sh)
    assert (tail["status"][:16] == AE.LEFT).all() and (tail["index"][:16, 0] == -1).all()
    assert (tail["status"][16:] == AE.CEILING).all() and (tail["index"][16:, 0] == 1).all()
    assert (tail["n_steps"] == 0).all() and np.array_equal(tail["position"], b["position"][-32:])
    assert (tail["depth"] == 0).all() and (tail["distance"] == 0).all()
    # max_steps
    full = st.advance(pos.copy(), d, rho, np.full(n, INF), None, ceiling, scale_height=sh)
    t = st.advance(pos.copy(), d, rho, np.full(n, INF), None, ceiling, max_steps=5, scale_height=sh)
    capped = t["status"] == AE.MAX_STEPS
    assert np.array_equal(capped, full["n_steps"] > 5) and capped.sum() > n // 2
    assert (t["n_steps"][capped] == 5).all() and st.trace_stats()["capped"] == int(capped.sum())
    same_bits(rays(full, ~capped), rays(t, ~capped))
    assert (t["depth"][capped] < full["depth"][capped]).all() and (t["depth"][capped] > 0).all()
    zero = st.advance(pos.copy(), d, rho, np.full(n, INF), None, ceiling, max_steps=0, scale_height=sh)
    assert (zero["status"] == AE.MAX_STEPS).all() and np.array_equal(zero["position"], pos)
    # the air thins out: less depth than at one density, on the same path
    u = st.advance(pos.copy(), d, rho, np.full(n, INF), None, ceiling)
    same_bits(u, full, ("position", "index", "distance", "n_steps", "status"))
    assert (full["depth"] < u["depth"]).all()
    # density 0 in the exponential medium: nothing is spent there, nothing is divided by it, and a
    # tiny budget lasts down to the rock
    tr = st.traverse(pos.copy(), d, ceiling)
    vac = np.array([2650.0, 0.0])
    t = st.advance(pos.copy(), d, vac, np.full(n, INF), None, ceiling, scale_height=sh)
    same_bits(full, t, ("position", "index", "distance", "n_steps", "status"))
    assert np.isfinite(t["depth"]).all()
    assert (np.abs(t["depth"] - 2650.0 * tr["length"][0]) <= 1e-9 * 2650.0 * tr["length"][0]).all()
    t = st.advance(pos.copy(), d, vac, np.full(n, 1.0), None, ceiling, scale_height=sh)
    rock = tr["length"][0] > 1.0
    assert rock.sum() > n // 2
    assert (t["status"][rock] == AE.SPENT).all() and (t["index"][rock, 0] == 0).all() and (t["depth"][rock] == 1.0).all()
    never = tr["length"][0] == 0
    assert (t["status"][never] != AE.SPENT).all() and (t["depth"][never] == 0).all()
    # an unchecked scale height gives what the arithmetic gives: NaN depth is SPENT after one step
    t = st.advance(pos.copy(), d, rho, np.full(n, INF), None, ceiling, scale_height=np.array([INF, np.nan]))
    assert (t["status"] == AE.SPENT).all() and (t["n_steps"] == 1).all() and np.isnan(t["depth"]).all()


def test_advance_exp_outputs_sizes_and_spaces(steppers, golden, math):
    import torch
    st = steppers["two"]
    parts = [batch(golden, "two", "c2"), batch(golden, "two", "ground")] * 3
    pos, d, budget, limit = (np.concatenate([p[name] for p in parts])
                             for name in ("position", "direction", "budget", "distance_max"))
    rho, sh, ceiling = parts[0]["density"], parts[0]["scale_height"], 2000.0
    n = pos.shape[0]   # 6000
    full = st.advance(pos.copy(), d, rho, budget, limit, ceiling, scale_height=sh)
    assert {AE.SPENT, AE.DISTANCE, AE.CEILING} <= set(full["status"].tolist())
    optional = ("depth", "distance", "n_steps")
    # optional outputs: asking for fewer changes no bit of the rest
    for k in range(len(optional) + 1):
        for want in itertools.combinations(optional, k):
            t = st.advance(pos.copy(), d, rho, budget, limit, ceiling, want=want, scale_height=sh)
            same_bits(full, t)
            for name in optional:
                assert (t[name] is None) == (name not in want)
    # ... and no limit at all is a limit of inf
    same_bits(st.advance(pos.copy(), d, rho, budget, None, ceiling, scale_height=sh),
              st.advance(pos.copy(), d, rho, budget, np.full(n, INF), ceiling, scale_height=sh))
    # batch sizes that are not multiples of 64: the same bits as one batch
    at = 0
    for size in (1, 63, 65, 1000, n - 1129):
        cut = slice(at, at + size)
        t = st.advance(pos[cut].copy(), d[cut], rho, budget[cut], limit[cut], ceiling, scale_height=sh)
        same_bits(t, {k: full[k][cut] for k in KEYS})
        at += size
    assert at == n
    # numpy (HOST) and torch (DEVICE): the same bits
    dev = [torch.tensor(a, device="cuda") for a in (pos, d, rho, budget, limit)]
    t = st.advance(*dev, ceiling, scale_height=torch.tensor(sh, device="cuda"))
    torch.cuda.synchronize()
    same_bits(full, {k: v.cpu().numpy() for k, v in t.items()})
    # the raw call over outputs full of garbage: every element written
    same_bits(full, raw(st, "turtle_stepper_advance_exp_n", n, pos, d, rho, sh, budget, limit, ceiling))


def test_advance_exp_over_stacks(tmp_path):
    """a 2 x 2 stack, every tile loaded: the call made again gives the same bits; a stack without
    room for its tiles is refused, in the name of the call that was made"""
    d = str(tmp_path / "grid")
    for la, lo in ((45, 3), (45, 4), (46, 3), (46, 4)):
        TA.synth.write_hgt(d, la, lo, 1201)
    full, small = TA.Stack(d, 0), TA.Stack(d, 1)
    full.load()
    sf, ss = TA.Stepper(), TA.Stepper()
    sf.add_stack(full, 0.0)
    ss.add_stack(small, 0.0)
    try:
        rng = np.random.default_rng(9)
        n = 3000
        lat, lon = rng.uniform(45.1, 46.9, n), rng.uniform(3.1, 4.9, n)
        az, el = rng.uniform(0, 360, n), rng.uniform(-8.0, 3.0, n)
        p0, _ = sf.position(lat, lon, 300.0)
        dire = TA.ecef_from_horizontal(lat, lon, az, el)
        rho, sh = AE.DENSITY[2], AE.SCALE_HEIGHT[2]
        for math in ("strict", "fast"):
            TA.set_math(math)
            none = np.full(n, INF)
            whole = sf.advance(p0.copy(), dire, rho, none, None, 2000.0, scale_height=sh)
            uniform = sf.advance(p0.copy(), dire, rho, none, None, 2000.0)
            same_bits(uniform, whole, ("position", "index", "distance", "n_steps", "status"))
            moved = whole["distance"] > 0
            assert moved.sum() > n // 2 and (whole["depth"][moved] < uniform["depth"][moved]).all()
            budget = rng.uniform(0.05, 1.6, n) * whole["depth"]
            limit = rng.uniform(0.5, 3.0, n) * whole["distance"]
            t1 = sf.advance(p0.copy(), dire, rho, budget, limit, 2000.0, scale_height=sh)
            assert sf.rounds == 1
            same_bits(t1, sf.advance(p0.copy(), dire, rho, budget, limit, 2000.0, scale_height=sh))
            assert {AE.SPENT, AE.DISTANCE, AE.LEFT} <= set(t1["status"].tolist())
            spent = t1["status"] == AE.SPENT
            assert np.array_equal(t1["depth"][spent], budget[spent])
            same_bits(sf.advance(p0.copy(), dire, rho, budget, limit, 2000.0),
                      sf.advance(p0.copy(), dire, rho, budget, limit, 2000.0, scale_height=np.full(2, INF)))
            with pytest.raises(TA.TurtleError) as err:
                ss.advance(p0.copy(), dire, rho, budget, limit, 2000.0, scale_height=sh)
            assert err.value.name == "DOMAIN_ERROR" and "resident tiles only" in str(err.value)
            assert "turtle_stepper_advance_exp_n" in str(err.value)
    finally:
        TA.set_math("fast")
        for o in (sf, ss, full, small):
            o.destroy()


# ---- 5. the example ---------------------------------------------------------------

def test_slant_depth_example(tmp_path):
    exe = str(tmp_path / "slant_depth")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "slant_depth.c"), "-o", exe,
                           "-L" + os.path.dirname(TA.library_path()), "-lturtle_amd",
                           "-Wl,-rpath," + os.path.dirname(TA.library_path()), "-lm"])
    tile = TC.write_tile(tmp_path, "rough")
    out = subprocess.run([exe, tile], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    lat0, lon0 = (float(v) for v in lines[0].split()[1:3])
    rows = [l.split() for l in lines if l.startswith(("slant", "reach"))]
    assert len(rows) == 34 and rows[16][5] == "ceiling" and all(r[5] == "spent" for r in rows[17:])
    # the same fan through the binding
    TA.set_math("fast")
    m = TA.Map.load(tile)
    st = TA.Stepper()
    st.add_map(m, 0.0)
    try:
        r = np.arange(34)
        el = 10.0 + 5.0 * (r % 17)
        lat, lon = np.full(34, lat0), np.full(34, lon0)
        pos, _ = st.position(lat, lon, np.full(34, 0.5))
        budget = np.where(r < 17, INF, 3000.0)
        t = st.advance(pos, TA.ecef_from_horizontal(lat, lon, np.zeros(34), el), np.array([2650.0, 1.205]), budget,
                       None, 30000.0, scale_height=np.array([INF, 8400.0]))
        names = ("spent", "distance", "left", "ceiling", "max_steps")
        for ray in range(34):
            row = rows[ray]
            assert int(row[1]) == ray and float(row[3]) == el[ray] and row[5] == names[t["status"][ray]]
            assert abs(float(row[7]) - t["distance"][ray]) < 1e-5
            assert abs(float(row[10]) - t["depth"][ray]) <= 1e-6 * t["depth"][ray]
        # the vertical ray is the closed form, as the example's last line says
        last = lines[-1].split()
        assert last[0] == "vertical" and abs(float(last[1]) - float(last[5])) <= 2e-6 * float(last[5])
        assert abs(float(last[1]) - t["depth"][16]) <= 1e-6 * t["depth"][16]
    finally:
        st.destroy()
        m.destroy()
