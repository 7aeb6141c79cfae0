"""turtle_stepper_advance_grid_n on the GPU: rays advanced by a column-depth budget and a distance
limit through rock whose density is a box of voxels, against the reference's loop
(tests/golden/advance_grid.npz), turtle_stepper_advance_n (no grid: the same bits; a uniform grid:
the same to rounding), closed forms over a flat with a small box under it, a kernel of the caller's
own on the device header's walk, and the example.

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

import advance_grid_cases as AG
import traverse_cases as TC
from test_gpu_advance import math, off_the_bar, on_the_ray, rays, same_bits, steppers  # noqa: F401
from test_gpu_traverse import BAR, OUTSIDE as TRAVERSE_OUTSIDE

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = AG.OUTPUTS
INF = float("inf")
ROCK, AIR = 2650.0, 1.205


def fixture_grid(a, density=None, medium=0):
    return TA.Grid(a["origin"], a["axis"], a["size"], AG.voxels() if density is None else density, medium)


def batch(golden, case, recipe):
    g, a = golden("traverse"), golden("advance_grid")
    k = f"{case}_{recipe}_"
    out = {name: g[k + name] for name in ("position", "direction", "length")}
    out.update(ceiling=float(g[k + "ceiling"]))
    out.update({name: a[k + name] for name in ("budget", "distance_max", "density", "T", "D")})
    out["ref"] = {name: a[k + name] for name in KEYS}
    return out


def raw(st, n, pos, d, rho, grid, budget, limit, ceiling, max_steps=1000000):
    """the C call itself over numpy arrays (grid: a TA.Grid over numpy voxels, or None: grid = NULL);
    outputs prefilled with garbage"""
    out = dict(position=np.array(pos, dtype=np.float64), index=np.full((n, 2), -9, np.int32),
               depth=np.full(n, np.nan), distance=np.full(n, -7.0), n_steps=np.full(n, -5, np.int32),
               status=np.full(n, -3, np.int32))
    p = {k: v.ctypes.data_as(C.c_void_p) for k, v in out.items()}
    keep = [np.ascontiguousarray(a, dtype=np.float64) for a in (d, rho, budget)]
    D, RHO, B = (a.ctypes.data_as(C.c_void_p) for a in keep)
    lim = None if limit is None else np.ascontiguousarray(limit, dtype=np.float64)
    LIM = None if lim is None else lim.ctypes.data_as(C.c_void_p)
    vox = None if grid is None else np.ascontiguousarray(grid.density, dtype=np.float64)
    G = None if grid is None else C.byref(grid._struct(vox))
    rc = TA.lib().turtle_stepper_advance_grid_n(st.h, C.c_long(n), p["position"], D, RHO, G, B, LIM, C.c_double(ceiling),
                                                max_steps, p["index"], p["depth"], p["distance"], p["n_steps"],
                                                p["status"], TA.HOST)
    assert rc == 0
    return out


# ---- 1. parity with the reference ---------------------------------------------

@pytest.mark.parametrize("recipe", ["ground", "c2"])
@pytest.mark.parametrize("case", TC.CASES)
def test_advance_grid_matches_the_reference(steppers, golden, math, case, recipe):
    b = batch(golden, case, recipe)
    st = steppers[case]
    assert st.media == b["density"].shape[0]
    grid = fixture_grid(golden("advance_grid"))
    t = st.advance(b["position"].copy(), b["direction"], b["density"], b["budget"], b["distance_max"], b["ceiling"],
                   grid=grid)
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
    spent, far = t["status"] == AG.SPENT, t["status"] == AG.DISTANCE
    assert np.array_equal(t["depth"][spent], b["budget"][spent])
    assert np.array_equal(t["distance"][far], b["distance_max"][far])
    # no cut: status, position and step count are traverse's
    uncut = t["status"] >= AG.LEFT
    tr = st.traverse(b["position"].copy(), b["direction"], b["ceiling"])
    for k in ("position", "index", "n_steps"):
        assert np.array_equal(tr[k][uncut], t[k][uncut]), k
    # the grid is seen: the depths are not those of one density a medium
    u = st.advance(b["position"].copy(), b["direction"], b["density"], np.full(spent.shape[0], INF), None, b["ceiling"])
    g = st.advance(b["position"].copy(), b["direction"], b["density"], np.full(spent.shape[0], INF), None, b["ceiling"],
                   grid=grid)
    same_bits(u, g, ("position", "index", "distance", "n_steps", "status"))
    assert (np.abs(g["depth"] - u["depth"]) > 1e-3 * u["depth"]).sum() > 20


# ---- 2. reductions ---------------------------------------------------------------

def close_to_advance(t, plain, pieces, D, T, rho):
    """a grid that changes no density: advance_n's status, medium and steps, its depth within 1e-12 D
    a piece the ray's walks met (one rounding a piece, with room), its distance and position
    within the same of T + D / (the density where the ray stands)"""
    same_bits(plain, t, ("index", "n_steps", "status"))
    count = np.maximum(pieces, 1)
    assert (np.abs(t["depth"] - plain["depth"]) <= 1e-12 * D * count).all()
    here = rho[np.maximum(plain["index"][:, 0], 0)]
    span = 1e-12 * count * (T + D / here)
    assert (np.abs(t["distance"] - plain["distance"]) <= span).all()
    assert (np.linalg.norm(t["position"] - plain["position"], axis=1) <= span + 4 * np.spacing(6.4e6)).all()


@pytest.mark.parametrize("case", TC.CASES)
def test_grids_that_change_nothing(steppers, golden, math, case):
    st = steppers[case]
    g, a, ag = golden("traverse"), golden("advance"), golden("advance_grid")
    geo = TC.oracle_geometry(case)
    for recipe in ("ground", "c2"):
        k = f"{case}_{recipe}_"
        pos, d, ceiling = g[k + "position"], g[k + "direction"], float(g[k + "ceiling"])
        rho, budget, limit = a[k + "density"], a[k + "budget"], a[k + "distance_max"]
        n = pos.shape[0]
        T = g[k + "length"].sum(axis=0)
        D = (rho[:, None] * g[k + "length"]).sum(axis=0)
        plain = st.advance(pos.copy(), d, rho, budget, limit, ceiling)
        s = st.trace_stats()
        # grid = NULL through the new call: the instance, and the bits, of advance_n
        t = raw(st, n, pos, d, rho, None, budget, limit, ceiling)
        assert st.trace_stats() == s and st.rounds == 1
        same_bits(plain, t)
        # every voxel at density[0]: advance_n to rounding; the pieces counted by the CPU checker
        uniform = np.full(AG.N[::-1], rho[0])
        pieces = AG.check(geo, pos, d, rho, AG.Box(ag["origin"], ag["axis"], ag["size"], uniform), budget, limit,
                          ceiling, tally=True)["tally"][:, 3]
        t = st.advance(pos.copy(), d, rho, budget, limit, ceiling, grid=fixture_grid(ag, uniform))
        assert st.trace_stats() == s
        close_to_advance(t, plain, pieces, D, T, rho)
        spent = t["status"] == AG.SPENT
        assert np.array_equal(t["depth"][spent], budget[spent])
        # the fixture's voxels given to the air, the box 2600 m lower, under every ground: no ray's air
        # enters it (a lane in the air tests the box at every step, and walks one piece)
        under = TA.Grid.enu(AG.LATITUDE, AG.LONGITUDE, AG.HEIGHT, AG.SIZE, AG.voxels(),
                            offset=(AG.OFFSET[0], AG.OFFSET[1], AG.OFFSET[2] - 2600.0), medium=st.media - 1)
        t = st.advance(pos.copy(), d, rho, budget, limit, ceiling, grid=under)
        assert st.trace_stats() == s
        close_to_advance(t, plain, plain["n_steps"] + 1, D, T, rho)


# ---- 3. closed forms: a flat at altitude 0, a 4 x 3 x 2 box under it ----------------

LAT, LON = 45.0, 3.0
SMALL_N, SMALL_SIZE, SMALL_OFFSET = (4, 3, 2), (10.0, 10.0, 10.0), (-15.0, -12.0, -30.0)


def small_voxels(void=False):
    """[2][3][4]: 2000 + 100 i0 + 10 i1 + 300 i2 (void: voxels (1, 1, 1) and (2, 1, 1) hold nothing)"""
    i2, i1, i0 = np.meshgrid(np.arange(2), np.arange(3), np.arange(4), indexing="ij")
    v = 2000.0 + 100.0 * i0 + 10.0 * i1 + 300.0 * i2
    if void:
        v[1, 1, 1:3] = 0.0
    return v


@pytest.fixture(scope="module")
def flats():
    """one flat layer at altitude 0 (rock under it, air over it)"""
    st = TA.Stepper()
    st.add_flat(0.0)
    yield st
    st.destroy()


def small_grid(density=None, lower=0.0):
    """the box: 4 x 3 x 2 voxels of 10 m, east-north-up at (45N, 3E), its top 10 m (and `lower`) under
    the flat; the point (45N, 3E, 0) stands over the voxels (1, 1, .), 15 m east and 12 m north of the
    box's corner"""
    offset = (SMALL_OFFSET[0], SMALL_OFFSET[1], SMALL_OFFSET[2] - lower)
    return TA.Grid.enu(LAT, LON, 0.0, SMALL_SIZE, small_voxels() if density is None else density, offset=offset)


def at(grid, s):
    """ECEF of the point s = (east, north, up) metres from the box's corner"""
    return grid.origin + np.asarray(s, dtype=np.float64) @ grid.axis


def along(grid, u):
    d = np.asarray(u, dtype=np.float64) @ grid.axis
    return d / np.linalg.norm(d)


# the segments: (start s, direction in the box's frame, length, the pieces (metres, density) in order)
def segments(v):
    r3 = np.sqrt(3.0)
    return [
        # vertical, down through both layers over (1, 1, .): 8 m of rock, the two voxels, 10 m of rock
        ((15.0, 12.0, 28.0), (0, 0, -1), 38.0, [(8.0, ROCK), (10.0, v[1, 1, 1]), (10.0, v[0, 1, 1]), (10.0, ROCK)]),
        # along axis 0 through four voxels, from inside the first to inside the last
        ((1.0, 12.0, 15.0), (1, 0, 0), 38.0, [(9.0, v[1, 1, 0]), (10.0, v[1, 1, 1]), (10.0, v[1, 1, 2]), (9.0, v[1, 1, 3])]),
        # down a voxel diagonal: (0, 0, 0) and (1, 1, 1) through their common corner (the ties)
        ((-2.0, -2.0, -2.0), (1, 1, 1), 26.0 * r3, [(2 * r3, ROCK), (10 * r3, v[0, 0, 0]), (10 * r3, v[1, 1, 1]), (4 * r3, ROCK)]),
        # in through a side face, out through the other: the outside density before and after
        ((-5.0, 12.0, 5.0), (1, 0, 0), 50.0, [(5.0, ROCK)] + [(10.0, v[0, 1, i]) for i in range(4)] + [(5.0, ROCK)]),
        # the same line in the upper layer (with `void`: nothing across (1, 1, 1) and (2, 1, 1))
        ((-5.0, 12.0, 15.0), (1, 0, 0), 50.0, [(5.0, ROCK)] + [(10.0, v[1, 1, i]) for i in range(4)] + [(5.0, ROCK)]),
    ]


def run_segments(st, grid, segs, budget=None):
    pos = np.array([at(grid, s[0]) for s in segs])
    d = np.array([along(grid, s[1]) for s in segs])
    limit = np.array([s[2] for s in segs])
    n = len(segs)
    b = np.full(n, INF) if budget is None else budget
    t = st.advance(pos.copy(), d, np.array([ROCK, AIR]), b, limit, INF, grid=grid)
    return pos, d, limit, t


@pytest.mark.parametrize("void", [False, True])
def test_closed_forms(flats, math, void):
    st = flats
    v = small_voxels(void)
    grid = small_grid(v)
    segs = segments(v)
    pos, d, limit, t = run_segments(st, grid, segs)
    want = np.array([sum(length * rho for length, rho in s[3]) for s in segs])
    print(f"{math} void={void}: steps {t['n_steps'].tolist()}, depth off {(np.abs(t['depth'] - want) / want).max():.2e} D")
    assert (t["status"] == AG.DISTANCE).all() and np.array_equal(t["distance"], limit) and (t["index"][:, 0] == 0).all()
    assert (np.abs(t["depth"] - want) <= 1e-9 * want).all()
    on_the_ray(t, pos, d, limit)
    if void:
        # the depth does not grow across the void: the limit at its near face and at its far face
        near = run_segments(st, grid, [(segs[4][0], segs[4][1], 15.0, None)])[3]
        far = run_segments(st, grid, [(segs[4][0], segs[4][1], 35.0, None)])[3]
        assert abs(near["depth"][0] - (5 * ROCK + 10 * v[1, 1, 0])) <= 1e-9 * near["depth"][0]
        assert abs(far["depth"][0] - near["depth"][0]) <= 1e-9 * near["depth"][0]
        # a budget reached 1 m past the void stops 1 m past it
        B = 5 * ROCK + 10 * v[1, 1, 0] + 1.0 * v[1, 1, 3]
        s = run_segments(st, grid, [segs[4]], np.array([B]))[3]
        assert s["status"][0] == AG.SPENT and s["depth"][0] == B and abs(s["distance"][0] - 36.0) <= 1e-7
    # every segment, its pieces' ends in the middle of each piece: a budget put there stops there
    for j, seg in enumerate(segs):
        start = depth = 0.0
        for length, rho in seg[3]:
            if rho > 0:
                B = depth + 0.5 * length * rho
                s = run_segments(st, grid, [seg], np.array([B]))[3]
                # (the ECEF coordinates are good to 1e-9 m; a voxel's face moved by that is 1e-6 kg/m^2)
                assert s["status"][0] == AG.SPENT and s["depth"][0] == B, (j, start)
                assert abs(s["distance"][0] - (start + 0.5 * length)) <= 1e-7, (j, start, s["distance"][0])
                assert np.linalg.norm(s["position"][0] - (pos[j] + d[j] * s["distance"][0])) <= 1e-7
            start, depth = start + length, depth + length * rho


def test_stops_inside_a_voxel_are_additive(steppers, golden, math):
    """advance by b1, then from where that ended by b2 (fresh samples): the depths and distances add
    up to those of one advance by b1 + b2, as test_gpu_advance has it for advance_n"""
    st = steppers["rough"]
    b = batch(golden, "rough", "ground")
    grid = fixture_grid(golden("advance_grid"))
    b1 = b2 = 0.5 * b["budget"]          # (b1 + b2 is the budget to the bit)
    args = (b["direction"], b["density"])
    one = st.advance(b["position"].copy(), *args, b["budget"], None, b["ceiling"], grid=grid)
    first = st.advance(b["position"].copy(), *args, b1, None, b["ceiling"], grid=grid)
    second = st.advance(first["position"].copy(), *args, b2, None, b["ceiling"], grid=grid)
    on = (first["status"] == AG.SPENT) & (first["index"][:, 0] == 0)
    box = AG.golden_box(grid.origin, grid.axis)
    inside = np.array([AG.inside(box, p) for p in first["position"]])
    assert (on & inside).sum() > 150
    on_the_ray(first, b["position"], b["direction"], b["T"])
    tol = BAR * b["T"][on]
    assert (np.abs(first["depth"] + second["depth"] - one["depth"])[on] <= BAR * b["D"][on]).all()
    assert (np.abs(first["distance"] + second["distance"] - one["distance"])[on] <= tol).all()
    assert (np.linalg.norm(second["position"] - one["position"], axis=1)[on] <= tol).all()


# ---- 4. edges -------------------------------------------------------------------

def test_advance_grid_edges(steppers, flats, golden, math):
    st = steppers["hgt"]
    b = batch(golden, "hgt", "c2")
    grid = fixture_grid(golden("advance_grid"))
    pos, d, rho, ceiling = b["position"][:64], b["direction"][:64], b["density"], b["ceiling"]
    n = 64
    assert (b["T"][:n] > 0).all()
    # a budget of 0, NaN or negative: spent at the origin; a limit of 0: reached there
    for budget, limit, status in ((0.0, None, AG.SPENT), (np.nan, None, AG.SPENT), (-1.0, None, AG.SPENT),
                                  (INF, 0.0, AG.DISTANCE), (0.0, 0.0, AG.SPENT)):
        t = st.advance(pos.copy(), d, rho, np.full(n, budget), None if limit is None else np.full(n, limit), ceiling,
                       grid=grid)
        assert (t["status"] == status).all() and (t["n_steps"] == 0).all()
        assert np.array_equal(t["position"], pos) and (t["depth"] == 0).all() and (t["distance"] == 0).all()
        assert (t["index"][:, 0] == 1).all()                 # (in the air, 500 m above the ground)
    # a start outside the data, and one above the ceiling: rays [-32:-16] and [-16:] of the recipe
    tail = st.advance(b["position"][-32:].copy(), b["direction"][-32:], rho, np.full(32, 1.0), np.full(32, 1.0), ceiling,
                      grid=grid)
    assert (tail["status"][:16] == AG.LEFT).all() and (tail["index"][:16, 0] == -1).all()
    assert (tail["status"][16:] == AG.CEILING).all() and (tail["index"][16:, 0] == 1).all()
    assert (tail["n_steps"] == 0).all() and np.array_equal(tail["position"], b["position"][-32:])
    assert (tail["depth"] == 0).all() and (tail["distance"] == 0).all()
    # max_steps
    full = st.advance(pos.copy(), d, rho, np.full(n, INF), None, ceiling, grid=grid)
    t = st.advance(pos.copy(), d, rho, np.full(n, INF), None, ceiling, max_steps=5, grid=grid)
    capped = t["status"] == AG.MAX_STEPS
    assert np.array_equal(capped, full["n_steps"] > 5) and capped.sum() > n // 2
    assert (t["n_steps"][capped] == 5).all() and st.trace_stats()["capped"] == int(capped.sum())
    same_bits(rays(full, ~capped), rays(t, ~capped))
    assert (t["depth"][capped] < full["depth"][capped]).all() and (t["depth"][capped] > 0).all()
    zero = st.advance(pos.copy(), d, rho, np.full(n, INF), None, ceiling, max_steps=0, grid=grid)
    assert (zero["status"] == AG.MAX_STEPS).all() and np.array_equal(zero["position"], pos)
    # a start inside the box, in the rock: 100 m under the ellipsoid near the middle of the tile, heading east and down
    box = AG.golden_box(grid.origin, grid.axis)
    # (330 m north and 160 m east of the middle itself, which lies on a voxel's edge)
    here = (np.array([AG.LATITUDE + 0.003]), np.array([AG.LONGITUDE + 0.002]))
    p0 = TA.ecef_from_geodetic(*here, np.array([-100.0]))
    assert AG.inside(box, p0[0])
    d0 = TA.ecef_from_horizontal(*here, np.array([90.0]), np.array([-2.0]))
    t = st.advance(p0.copy(), d0, rho, np.array([INF]), np.array([5000.0]), ceiling, grid=grid)
    assert t["status"][0] == AG.DISTANCE and t["index"][0, 0] == 0 and t["distance"][0] == 5000.0
    want, _, _ = AG.grid_depth(box, rho[0], 0, p0[0].tolist(), d0[0].tolist(), 5000.0, INF)
    assert abs(t["depth"][0] - want) <= BAR * want and abs(want - rho[0] * 5000.0) > 1e-3 * want
    # a 1 x 1 x 1 grid: one voxel of 1000 kg/m^3, 20 m thick, 10 m under the flat
    one = TA.Grid.enu(LAT, LON, 0.0, (40.0, 40.0, 20.0), np.full((1, 1, 1), 1000.0), offset=(-20.0, -20.0, -30.0))
    p1 = TA.ecef_from_geodetic(np.array([LAT]), np.array([LON]), np.array([-2.0]))
    d1 = TA.ecef_from_horizontal(np.array([LAT]), np.array([LON]), np.array([0.0]), np.array([-90.0]))
    t = flats.advance(p1.copy(), d1, np.array([ROCK, AIR]), np.array([INF]), np.array([38.0]), INF, grid=one)
    assert t["status"][0] == AG.DISTANCE and abs(t["depth"][0] - (8 * ROCK + 20 * 1000.0 + 10 * ROCK)) <= 1e-9 * t["depth"][0]


def test_advance_grid_outputs_sizes_and_spaces(steppers, golden, math):
    import torch
    st = steppers["two"]
    parts = [batch(golden, "two", "c2"), batch(golden, "two", "ground")]
    pos, d, budget, limit = (np.concatenate([p[name] for p in parts])
                             for name in ("position", "direction", "budget", "distance_max"))
    rho, ceiling = parts[0]["density"], 2000.0
    grid = fixture_grid(golden("advance_grid"))
    n = pos.shape[0]   # 2000
    full = st.advance(pos.copy(), d, rho, budget, limit, ceiling, grid=grid)
    assert {AG.SPENT, AG.DISTANCE, AG.CEILING} <= set(full["status"].tolist())
    optional = ("depth", "distance", "n_steps")
    # optional outputs: asking for fewer changes no bit of the rest
    for k in range(len(optional) + 1):
        for want in itertools.combinations(optional, k):
            t = st.advance(pos.copy(), d, rho, budget, limit, ceiling, want=want, grid=grid)
            same_bits(full, t)
            for name in optional:
                assert (t[name] is None) == (name not in want)
    # ... and no limit at all is a limit of inf
    same_bits(st.advance(pos.copy(), d, rho, budget, None, ceiling, grid=grid),
              st.advance(pos.copy(), d, rho, budget, np.full(n, INF), ceiling, grid=grid))
    # batch sizes that are not multiples of 64: the same bits as one batch
    at_ = 0
    for size in (1, 63, 65, 1000, n - 1129):
        cut = slice(at_, at_ + size)
        t = st.advance(pos[cut].copy(), d[cut], rho, budget[cut], limit[cut], ceiling, grid=grid)
        same_bits(t, {k: full[k][cut] for k in KEYS})
        at_ += size
    assert at_ == n
    # numpy (HOST) and torch (DEVICE), the voxels a tensor on the GPU: the same bits
    dev = [torch.tensor(a, device="cuda") for a in (pos, d, rho, budget, limit)]
    on_gpu = TA.Grid(grid.origin, grid.axis, grid.size, torch.tensor(grid.density, device="cuda"))
    t = st.advance(*dev, ceiling, grid=on_gpu)
    torch.cuda.synchronize()
    same_bits(full, {k: v.cpu().numpy() for k, v in t.items()})
    # the raw call over outputs full of garbage: every element written
    same_bits(full, raw(st, n, pos, d, rho, grid, budget, limit, ceiling))


def test_advance_grid_over_stacks(tmp_path):
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
        rho = AG.DENSITY[2]
        # a box over the stack's middle, 100 km wide: 50 x 50 x 8 voxels of 2 km x 2 km x 300 m
        i2, i1, i0 = np.meshgrid(np.arange(8), np.arange(50), np.arange(50), indexing="ij")
        grid = TA.Grid.enu(46.0, 4.0, 0.0, (2000.0, 2000.0, 300.0), 2000.0 + 20.0 * i0 + 10.0 * i1 + 50.0 * i2,
                           offset=(-50000.0, -50000.0, -1400.0))
        for math in ("strict", "fast"):
            TA.set_math(math)
            none = np.full(n, INF)
            whole = sf.advance(p0.copy(), dire, rho, none, None, 2000.0, grid=grid)
            uniform = sf.advance(p0.copy(), dire, rho, none, None, 2000.0)
            same_bits(uniform, whole, ("position", "index", "distance", "n_steps", "status"))
            assert (np.abs(whole["depth"] - uniform["depth"]) > 1e-3 * uniform["depth"]).sum() > n // 4
            budget = rng.uniform(0.05, 1.6, n) * whole["depth"]
            limit = rng.uniform(0.5, 3.0, n) * whole["distance"]
            t1 = sf.advance(p0.copy(), dire, rho, budget, limit, 2000.0, grid=grid)
            assert sf.rounds == 1
            same_bits(t1, sf.advance(p0.copy(), dire, rho, budget, limit, 2000.0, grid=grid))
            assert {AG.SPENT, AG.DISTANCE, AG.LEFT} <= set(t1["status"].tolist())
            spent = t1["status"] == AG.SPENT
            assert np.array_equal(t1["depth"][spent], budget[spent])
            with pytest.raises(TA.TurtleError) as err:
                ss.advance(p0.copy(), dire, rho, budget, limit, 2000.0, grid=grid)
            assert err.value.name == "DOMAIN_ERROR" and "resident tiles only" in str(err.value)
            assert "turtle_stepper_advance_grid_n" in str(err.value)
    finally:
        TA.set_math("fast")
        for o in (sf, ss, full, small):
            o.destroy()


# ---- 5. the walk in a kernel of the caller's own ---------------------------------

@pytest.fixture(scope="module")
def grid_walk(tmp_path_factory):
    """tests/c/grid_walk.hip, built as tests/device_loops.py builds its kernels"""
    import device_loops as DL
    so = os.path.join(str(tmp_path_factory.mktemp("grid_walk")), "libgrid_walk.so")
    made = subprocess.run([DL.HIPCC] + DL.FLAGS + ["-fPIC", "-shared", os.path.join(ROOT, "tests", "c", "grid_walk.hip"),
                           "-o", so], capture_output=True, text=True)
    assert made.returncode == 0, made.stderr[-4000:]
    lib = C.CDLL(so)
    lib.grid_walk_view_size.restype = C.c_long
    return lib


def test_the_device_function_gives_the_bits_of_the_call(flats, grid_walk, math):
    """One step of the library's call is one walk: from the origin, over the step's length, with the
    whole budget.  The closed-form segments, each begun with a step that ends at max_steps (its
    length: the reported distance) and again with a budget of half that step's depth (SPENT inside
    it): the header's walk, in a kernel built apart from the library, returns the depth and the
    stop of the library's call to the bit."""
    import torch
    from turtle_amd.binding import _Grid
    assert grid_walk.grid_walk_view_size() == C.sizeof(_Grid)
    st = flats
    v = small_voxels()
    # the box 270 m lower: a step there is longer than the box is wide, and one walk crosses it all
    grid = small_grid(v, lower=270.0)
    segs = segments(v)
    # the segments' starts, and the same lines begun 3 m later
    pos = np.array([at(grid, s[0]) for s in segs] + [at(grid, np.array(s[0]) + 3.0 * np.array(s[1]) / np.linalg.norm(s[1]))
                                                     for s in segs])
    d = np.array([along(grid, s[1]) for s in segs] * 2)
    n = pos.shape[0]
    rho = np.array([ROCK, AIR])
    step = st.advance(pos.copy(), d, rho, np.full(n, INF), None, INF, max_steps=1, grid=grid)
    assert (step["status"] == AG.MAX_STEPS).all() and (step["n_steps"] == 1).all() and (step["index"][:, 0] == 0).all()
    # (the steps do cross the box: most of them meet more than one density)
    assert (np.abs(step["depth"] - ROCK * step["distance"]) > 1e-3 * step["depth"]).sum() >= 8
    half = 0.5 * step["depth"]
    cut = st.advance(pos.copy(), d, rho, half, None, INF, max_steps=1, grid=grid)
    assert (cut["status"] == AG.SPENT).all() and np.array_equal(cut["depth"], half)
    vox = torch.tensor(v, device="cuda")
    view = grid._struct(vox)
    L = np.concatenate([step["distance"], step["distance"]])
    R = np.concatenate([np.full(n, INF), half])
    dev = {k: torch.tensor(a, device="cuda") for k, a in dict(
        rho=np.full(2 * n, ROCK), m=np.zeros(2 * n, dtype=np.int32), p0=np.concatenate([pos, pos]),
        d=np.concatenate([d, d]), L=L, R=R).items()}
    x, f = torch.zeros(2 * n, dtype=torch.float64, device="cuda"), torch.zeros(2 * n, dtype=torch.float64, device="cuda")
    stopped = torch.zeros(2 * n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rc = grid_walk.grid_walk(C.byref(view), C.c_long(2 * n), p(dev["rho"]), p(dev["m"]), p(dev["p0"]), p(dev["d"]),
                             p(dev["L"]), p(dev["R"]), p(x), p(f), p(stopped))
    assert rc == 0
    x, f, stopped = x.cpu().numpy(), f.cpu().numpy(), stopped.cpu().numpy()
    assert not stopped[:n].any() and stopped[n:].all()
    assert np.array_equal(x[:n], step["depth"]) and np.array_equal(f[:n], step["distance"])
    assert np.array_equal(f[n:], cut["distance"])
    # ... and the C checker's walk agrees with both to rounding
    cx, cf, cs = AG.walk_c(AG.Box(grid.origin, grid.axis, grid.size, v), ROCK, 0, np.concatenate([pos, pos]),
                           np.concatenate([d, d]), L, R)
    assert np.array_equal(cs, stopped)
    assert (np.abs(cx[:n] - x[:n]) <= 1e-12 * x[:n]).all() and (np.abs(cf - f) <= 1e-12 * np.maximum(f, 1.0)).all()


# ---- 6. the example ---------------------------------------------------------------

def test_density_grid_example(tmp_path):
    exe = str(tmp_path / "density_grid")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "density_grid.c"), "-o", exe,
                           "-L" + os.path.dirname(TA.library_path()), "-lturtle_amd",
                           "-Wl,-rpath," + os.path.dirname(TA.library_path()), "-lm"])
    tile = TC.write_tile(tmp_path, "rough")
    out = subprocess.run([exe, tile], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    lat0, lon0, z0 = (float(lines[0].split()[i]) for i in (1, 2, 4))
    rows = [l.split() for l in lines if l.startswith("line")]
    assert len(rows) == 16
    # the same fan through the binding
    TA.set_math("fast")
    m = TA.Map.load(tile)
    st = TA.Stepper()
    st.add_map(m, 0.0)
    try:
        el = 2.0 + 2.0 * np.arange(16)
        lat, lon = np.full(16, lat0), np.full(16, lon0)
        pos, _ = st.position(lat, lon, np.full(16, 0.5))
        d = TA.ecef_from_horizontal(lat, lon, np.zeros(16), el)
        body = np.full((8, 16, 16), 2650.0)
        plain = body.copy()
        body[1:5, 4:8, 6:10] = 1800.0
        depth = []
        for voxels in (body, plain):
            grid = TA.Grid.enu(lat0, lon0, z0, (500.0, 500.0, 250.0), voxels, offset=(-4000.0, 0.0, -250.0))
            t = st.advance(pos.copy(), d, np.array([2650.0, 1.205]), np.full(16, INF), None, 5000.0, grid=grid)
            depth.append(t["depth"])
        for ray in range(16):
            row = rows[ray]
            assert int(row[1]) == ray and float(row[3]) == el[ray]
            assert abs(float(row[5]) - t["distance"][ray]) < 1e-5
            assert abs(float(row[8]) - depth[0][ray]) <= 1e-6 * depth[0][ray]
            assert abs(float(row[11]) - depth[1][ray]) <= 1e-6 * depth[1][ray]
        # the body is seen: some line's opacity is lower with it, none higher
        assert (depth[0] < 0.98 * depth[1]).any() and (depth[0] <= depth[1] * (1 + 1e-12)).all()
    finally:
        st.destroy()
        m.destroy()
