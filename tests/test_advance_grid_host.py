"""turtle_stepper_advance_grid_n without a GPU: the C ABI declares, exports, names and checks the
call; the CPU checker (tests/c/advance_grid_loop.c over the oracle's restatement) and, where it is
built, the compiled reference reproduce tests/golden/advance_grid.npz bit for bit; without a grid
the checker gives advance.npz; the walk in Python and in C agree on random segments and on segments
whose sums have closed forms; and the fixture holds what the GPU tests lean on."""
import ctypes as C
import os

import numpy as np
import pytest

import turtle_amd as TA
from oracle import ref_ffi as R

import advance_grid_cases as AG
import traverse_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


def fixture_box(a):
    return AG.golden_box(a["origin"], a["axis"])


def test_advance_grid_declared_exported_named_and_bound():
    text = open(os.path.join(ROOT, "include", "turtle_amd.h")).read()
    assert "TURTLE_API enum turtle_return turtle_stepper_advance_grid_n(" in text
    assert "struct turtle_amd_grid {" in text and "TURTLE_API void turtle_amd_grid_enu(" in text
    assert "advance_exp_n or advance_grid_n call on this stepper" in text      # (the comment on trace_stats)
    exported = C.CDLL(TA.library_path())
    assert hasattr(exported, "turtle_stepper_advance_grid_n") and hasattr(exported, "turtle_amd_grid_enu")
    L = TA.lib()
    f = L.turtle_error_function
    f.restype = C.c_char_p
    f.argtypes = [C.c_void_p]
    assert f(C.cast(L.turtle_stepper_advance_grid_n, C.c_void_p).value) == b"turtle_stepper_advance_grid_n"
    assert f(C.cast(L.turtle_stepper_advance_n, C.c_void_p).value) == b"turtle_stepper_advance_n"
    import inspect
    assert inspect.signature(TA.Stepper.advance).parameters["grid"].default is None
    assert inspect.signature(TA.Grid.__init__).parameters["medium"].default == 0
    assert list(inspect.signature(TA.Grid.enu).parameters)[:5] == ["latitude", "longitude", "height", "size", "density"]
    device = open(os.path.join(ROOT, "include", "turtle_amd_device.h")).read()
    assert "struct turtle_amd_grid_view {" in device
    assert "GridDepth grid_depth(const turtle_amd_grid_view & G, double rho_out, int m," in device


def test_grid_enu_is_the_horizontal_frame(golden):
    """host arithmetic: east, north, up at the point, orthonormal; the fixture's frame to rounding"""
    a = golden("advance_grid")
    g = TA.Grid.enu(AG.LATITUDE, AG.LONGITUDE, AG.HEIGHT, AG.SIZE, np.zeros(AG.N[::-1]), offset=AG.OFFSET)
    assert g.n == AG.N and g.medium == 0
    assert np.abs(g.axis @ g.axis.T - np.eye(3)).max() < 1e-15
    assert np.abs(g.axis - a["axis"]).max() < 1e-15 and np.abs(g.origin - a["origin"]).max() < 1e-8
    origin, axis = AG.enu_frame(AG.LATITUDE, AG.LONGITUDE, AG.HEIGHT, AG.OFFSET)
    assert np.abs(axis - a["axis"]).max() < 1e-15 and np.abs(origin - a["origin"]).max() < 1e-8
    assert np.allclose(np.cross(g.axis[0], g.axis[1]), g.axis[2], atol=1e-15)       # right-handed
    with pytest.raises(ValueError):
        TA.Grid(np.zeros(3), np.eye(3), np.ones(3), np.zeros((4, 4)))                 # [n2][n1][n0]


def test_advance_grid_argument_errors():
    """checked before anything touches a device; the outputs stay as they were"""
    st = TA.Stepper()
    st.add_flat(0.0)
    L = TA.lib()
    pos, d, rho, b, dm = np.ones((4, 3)), np.ones((4, 3)), np.ones(2), np.ones(4), np.ones(4)
    idx, nst, sta = (np.full(s, -3, dtype=np.int32) for s in ((4, 2), 4, 4))
    dep, dis = np.full(4, -7.0), np.full(4, -8.0)
    POS, D, RHO, B, DM, IDX, NST, STA, DEP, DIS = (a.ctypes.data_as(C.c_void_p)
                                                   for a in (pos, d, rho, b, dm, idx, nst, sta, dep, dis))
    vox = np.ones((2, 3, 4))

    def grid(n=(4, 3, 2), size=(1.0, 1.0, 1.0), medium=0, density=vox):
        g = TA.Grid(np.zeros(3), np.eye(3), size, vox, medium)
        g.n = n
        return C.byref(g._struct(density))

    def call(stepper=st.h, n=4, position=POS, direction=D, density=RHO, grid=grid(), budget=B, distance_max=DM,
             max_steps=10, index=IDX, depth=DEP, distance=DIS, n_steps=NST, status=STA, space=TA.HOST):
        rc = L.turtle_stepper_advance_grid_n(stepper, C.c_long(n), position, direction, density, grid, budget,
                                             distance_max, C.c_double(np.inf), max_steps, index, depth, distance,
                                             n_steps, status, space)
        TA.binding._pending.clear()
        return TA.binding.RETURN_NAMES[rc]

    try:
        assert [call(stepper=None), call(position=None), call(direction=None), call(density=None),
                call(budget=None), call(index=None), call(status=None), call(grid=grid(density=None))] == ["BAD_ADDRESS"] * 8
        assert [call(max_steps=-1), call(space=2), call(space=-1)] == ["DOMAIN_ERROR"] * 3
        bad = [grid(n=(0, 3, 2)), grid(n=(4, -1, 2)), grid(n=(4, 3, 0)), grid(size=(0.0, 1.0, 1.0)),
               grid(size=(1.0, -2.0, 1.0)), grid(size=(1.0, 1.0, np.nan)), grid(size=(np.inf, 1.0, 1.0)),
               grid(n=(2048, 2048, 512)), grid(medium=-1), grid(medium=2)]
        assert [call(grid=g) for g in bad] == ["DOMAIN_ERROR"] * len(bad)
        assert [call(grid=g, n=0) for g in bad] == ["DOMAIN_ERROR"] * len(bad)   # (before n is looked at)
        # no grid is no error: with a bad argument beside it, that argument's error
        assert call(grid=None, max_steps=-1) == "DOMAIN_ERROR"
        assert call(grid=None, budget=None) == "BAD_ADDRESS"
        assert call(n=0) == call(n=-3) == call(n=0, distance_max=None, depth=None) == "SUCCESS"
        assert call(n=0, grid=None) == "SUCCESS"
        assert (pos == 1).all() and (idx == -3).all() and (nst == -3).all() and (sta == -3).all()
        assert (dep == -7).all() and (dis == -8).all()
        # the messages carry the name of the call that was made
        rc = L.turtle_stepper_advance_grid_n(st.h, C.c_long(4), POS, D, RHO, None, B, DM, C.c_double(np.inf), -1, IDX,
                                             DEP, DIS, NST, STA, TA.HOST)
        assert rc != 0 and "turtle_stepper_advance_grid_n" in TA.binding._pending[-1][1]
        TA.binding._pending.clear()
        rc = L.turtle_stepper_advance_grid_n(st.h, C.c_long(4), POS, D, RHO, grid(medium=5), B, DM, C.c_double(np.inf),
                                             3, IDX, DEP, DIS, NST, STA, TA.HOST)
        assert rc != 0 and "turtle_stepper_advance_grid_n" in TA.binding._pending[-1][1]
        TA.binding._pending.clear()
        g = TA.Grid(np.zeros(3), np.eye(3), np.ones(3), vox)
        with pytest.raises(TA.TurtleError) as err:                     # and through the binding
            st.advance(pos, d, rho, b, max_steps=-1, grid=g)
        assert err.value.name == "DOMAIN_ERROR" and "turtle_stepper_advance_grid_n" in str(err.value)
        with pytest.raises(ValueError):
            st.advance(pos, d, rho, b, grid=g, scale_height=np.full(2, INF))   # not together
    finally:
        st.destroy()


@pytest.mark.parametrize("case", TC.CASES)
def test_checker_reproduces_the_fixture(golden, case):
    g, a = golden("traverse"), golden("advance_grid")
    geo = TC.oracle_geometry(case)
    box = fixture_box(a)
    for recipe in ("ground", "c2"):
        k = f"{case}_{recipe}_"
        out = AG.check(geo, g[k + "position"], g[k + "direction"], a[k + "density"], box, a[k + "budget"],
                       a[k + "distance_max"], float(g[k + "ceiling"]))
        for name in AG.OUTPUTS:
            assert np.array_equal(out[name], a[k + name]), (case, recipe, name)
        # uncut: the D and T the fixture's budgets were drawn from
        n = out["status"].shape[0]
        full = AG.check(geo, g[k + "position"], g[k + "direction"], a[k + "density"], box, np.full(n, np.inf), None,
                        float(g[k + "ceiling"]))
        assert np.array_equal(full["depth"], a[k + "D"]) and np.array_equal(full["distance"], a[k + "T"])


@pytest.mark.skipif(not R.available(), reason="oracle/_ref is not built (no reference sources here)")
@pytest.mark.parametrize("case", TC.CASES)
def test_the_reference_reproduces_the_fixture(golden, tmp_path, case):
    g, a = golden("traverse"), golden("advance_grid")
    m = R.RefMap.load(TC.write_tile(tmp_path, case))
    st = AG.reference_stepper(case, m)
    box = fixture_box(a)
    try:
        for recipe in ("ground", "c2"):
            k = f"{case}_{recipe}_"
            out = AG.reference_loop(st, g[k + "position"], g[k + "direction"], a[k + "density"], box,
                                    a[k + "budget"], a[k + "distance_max"], float(g[k + "ceiling"]))
            for name in AG.OUTPUTS:
                assert np.array_equal(out[name], a[k + name]), (case, recipe, name)
    finally:
        st.destroy()
        m.destroy()
    R.errors()


@pytest.mark.parametrize("case", TC.CASES)
def test_no_grid_is_advance(golden, case):
    """grid = NULL: advance.npz's status, index and n_steps, its depth and distance to rounding (the
    walk's one piece computes the cut as a + (R - acc) / rho and the depth as rho * (b - a))"""
    g, a = golden("traverse"), golden("advance")
    geo = TC.oracle_geometry(case)
    for recipe in ("ground", "c2"):
        k = f"{case}_{recipe}_"
        out = AG.check(geo, g[k + "position"], g[k + "direction"], a[k + "density"], None, a[k + "budget"],
                       a[k + "distance_max"], float(g[k + "ceiling"]))
        for name in ("status", "index", "n_steps"):
            assert np.array_equal(out[name], a[k + name]), (case, recipe, name)
        steps = np.maximum(a[k + "n_steps"], 1)
        for name in ("depth", "distance"):
            assert (np.abs(out[name] - a[k + name]) <= 4 * 2.0 ** -53 * steps * np.abs(a[k + name])).all(), (k, name)
        assert np.abs(out["position"] - a[k + "position"]).max() <= 1e-8


# ---- the walk alone ---------------------------------------------------------------

def small_box():
    """7 x 5 x 4 voxels of 10 x 20 x 5 m along x, y, z from the origin; rho = 1 + i0 + 10 i1 + 100 i2"""
    i2, i1, i0 = np.meshgrid(np.arange(4), np.arange(5), np.arange(7), indexing="ij")
    return AG.Box(np.zeros(3), np.eye(3), (10.0, 20.0, 5.0), 1.0 + i0 + 10.0 * i1 + 100.0 * i2)


def both(box, rho_out, m, p0, dr, L, R=INF):
    """the walk in Python and in C on one segment, asserted to agree -> (x, f, stopped)"""
    x, f, stopped = AG.grid_depth(box, rho_out, m, [float(v) for v in p0], [float(v) for v in dr], L, R)
    cx, cf, cs = AG.walk_c(box, rho_out, m, p0, dr, L, R)
    assert bool(cs[0]) == stopped
    assert abs(cx[0] - x) <= 1e-12 * max(abs(x), 1.0) and abs(cf[0] - f) <= 1e-12 * max(abs(f), 1.0)
    return x, f, stopped


def test_the_walks_agree_on_random_segments():
    box = small_box()
    rng = np.random.default_rng(5)
    n = 300
    p0 = rng.uniform((-30, -40, -10), (100, 140, 30), (n, 3))
    dr = rng.normal(size=(n, 3))
    dr[::7, 0] = 0.0
    dr[3::11, 2] = 0.0
    dr[5::13, 1:] = 0.0
    dr[5::13, 0] = 1.0
    dr /= np.linalg.norm(dr, axis=1)[:, None]
    L = rng.uniform(1.0, 200.0, n)
    cx, cf, cs = AG.walk_c(box, 7.0, 0, p0, dr, L, INF)
    stops = 0
    for r in range(n):
        pieces = []
        x, f, stopped = AG.grid_depth(box, 7.0, 0, p0[r].tolist(), dr[r].tolist(), float(L[r]), INF, pieces)
        assert not stopped and f == L[r] and not cs[r] and cf[r] == L[r]
        assert abs(cx[r] - x) <= 1e-12 * x
        # the pieces tile [0, L] in order, none negative
        assert pieces[0][0] == 0 and pieces[-1][1] == L[r]
        assert all(q[0] == p[1] for p, q in zip(pieces, pieces[1:])) and all(p[1] >= p[0] for p in pieces)
        # the sum against the density sampled along the segment (a midpoint rule, 20 000 points)
        fm = (np.arange(20000) + 0.5) * (L[r] / 20000)
        s = p0[r] + fm[:, None] * dr[r]
        i = np.floor(s / box.size).astype(int)
        within = ((i >= 0) & (i < np.array(box.n))).all(axis=1)
        i = np.clip(i, 0, np.array(box.n) - 1)
        rho = np.where(within, box.density[i[:, 2], i[:, 1], i[:, 0]], 7.0)
        assert abs(rho.mean() * L[r] - x) <= 500.0 * 40 * L[r] / 20000 + 1e-9   # (<= 40 faces, jumps <= 500)
        # stopped at a part of the sum and walked again to there: that part
        R = float(rng.uniform(0.05, 1.2)) * x
        x2, f2, st2 = both(box, 7.0, 0, p0[r], dr[r], float(L[r]), R)
        assert st2 == (R <= x) or abs(R - x) < 1e-9 * x
        if st2:
            stops += 1
            x3, _, st3 = both(box, 7.0, 0, p0[r], dr[r], f2, INF)
            assert not st3 and abs(x3 - R) <= 1e-9 * R
        # another medium: one piece at its density
        assert both(box, 3.0, 1, p0[r], dr[r], float(L[r])) == (3.0 * L[r], L[r], False)
    assert stops > 150


def test_segments_with_closed_forms():
    box = small_box()
    out = 7.0
    e = 1e-11
    # a zero direction component, the segment lying exactly on the face between i1 = 0 and 1: the
    # voxels (i0, 1, 0) of the upper side, 10 m each, and 5 m outside at either end
    x, f, _ = both(box, out, 0, (-5.0, 20.0, 2.5), (1.0, 0.0, 0.0), 80.0)
    assert x == 5 * out + 10.0 * sum(1 + i0 + 10 for i0 in range(7)) + 5 * out and f == 80.0
    # through voxel edges (two axes tie): the diagonal of the plane z = 2.5 meets (i, i, 0), i = 0 .. 4
    u = np.array([10.0, 20.0, 0.0]) / np.sqrt(500.0)
    x, _, _ = both(box, out, 0, -np.sqrt(500.0) * u + (0, 0, 2.5), u, 7 * np.sqrt(500.0))
    want = np.sqrt(500.0) * (out + sum(1 + 11 * i for i in range(5)) + out)
    assert abs(x - want) <= e * want
    # through voxel corners (three axes tie): the voxels' diagonal meets (i, i, i), i = 0 .. 3
    u = np.array([10.0, 20.0, 5.0]) / np.sqrt(525.0)
    x, _, _ = both(box, out, 0, -np.sqrt(525.0) * u, u, 6 * np.sqrt(525.0))
    want = np.sqrt(525.0) * (out + sum(1 + 111 * i for i in range(4)) + out)
    assert abs(x - want) <= e * want
    # ... and backwards
    x, _, _ = both(box, out, 0, 5 * np.sqrt(525.0) * u, -u, 6 * np.sqrt(525.0))
    assert abs(x - want) <= e * want
    # a start inside the box: 5 m of (3, 2, 1), 10 m of (4, 2, 1), 5 m of (5, 2, 1)
    x, _, _ = both(box, out, 0, (35.0, 50.0, 7.5), (1.0, 0.0, 0.0), 20.0)
    assert x == 5 * 124.0 + 10 * 125.0 + 5 * 126.0
    # a miss: the outside density all the way
    assert both(box, out, 0, (-5.0, -5.0, -5.0), (0.0, 1.0, 0.0), 50.0) == (50 * out, 50.0, False)
    assert both(box, out, 0, (-5.0, 10.0, 2.5), (-1.0, 0.0, 0.0), 50.0) == (50 * out, 50.0, False)
    # an end inside the box: 5 m outside, (0, 0, 0) and (1, 0, 0) whole, 5 m of (2, 0, 0)
    x, _, _ = both(box, out, 0, (-5.0, 10.0, 2.5), (1.0, 0.0, 0.0), 30.0)
    assert x == 5 * out + 10 * 1.0 + 10 * 2.0 + 5 * 3.0
    # stopped in the middle of (1, 0, 0): 5 m of 7, 10 m of 1, 5 m of 2
    assert both(box, out, 0, (-5.0, 10.0, 2.5), (1.0, 0.0, 0.0), 30.0, 35.0 + 10.0 + 10.0) == (45.0, 20.0, True)
    # a void: it spends nothing, stops nothing, divides nothing; a budget reached past it stops past it
    hollow = small_box()
    hollow.density[0, 0, 1] = 0.0
    hollow = AG.Box(hollow.origin, hollow.axis, hollow.size, hollow.density)
    assert both(hollow, out, 0, (-5.0, 10.0, 2.5), (1.0, 0.0, 0.0), 30.0) == (35.0 + 10.0 + 0.0 + 15.0, 30.0, False)
    # (a budget that ends with (0, 0, 0) stops at its far face, before the void; 3 kg/m^2 more, 1 m past it)
    assert both(hollow, out, 0, (-5.0, 10.0, 2.5), (1.0, 0.0, 0.0), 30.0, 45.0)[1:] == (15.0, True)
    assert both(hollow, out, 0, (-5.0, 10.0, 2.5), (1.0, 0.0, 0.0), 30.0, 45.0 + 3.0)[1:] == (26.0, True)
    # a 1 x 1 x 1 grid
    one = AG.Box(np.zeros(3), np.eye(3), (10.0, 20.0, 5.0), np.full((1, 1, 1), 4.0))
    assert both(one, out, 0, (-5.0, 10.0, 2.5), (1.0, 0.0, 0.0), 30.0) == (5 * out + 40.0 + 15 * out, 30.0, False)


# ---- the fixture ------------------------------------------------------------------

def test_the_fixture_holds_what_it_is_meant_to(golden):
    g, a = golden("traverse"), golden("advance_grid")
    box = fixture_box(a)
    assert tuple(a["n"]) == AG.N and tuple(a["size"]) == AG.SIZE and int(a["medium"]) == AG.MEDIUM
    assert np.array_equal(a["block"], np.array(AG.BLOCK))
    assert all(np.size(a[name]) <= 3000 for name in a)               # (no voxels in the file: they are a formula)
    rho = box.density
    (a0, b0), (a1, b1), (a2, b2) = AG.BLOCK
    assert (rho[a2:b2, a1:b1, a0:b0] == AG.BLOCK_DENSITY).all() and (rho > 0).all()
    smooth = AG.voxels(block=None)
    assert 1800.0 <= smooth.min() < 1900.0 and 3100.0 < smooth.max() <= 3200.0
    rock_steps = voxel_steps = face_rays = spent_inside = far_inside = 0
    for case, recipe in AG.BATCHES:
        k = f"{case}_{recipe}_"
        media = g[k + "length"].shape[0]
        assert np.array_equal(a[k + "density"], AG.DENSITY[media])
        status, index = a[k + "status"], a[k + "index"]
        T = a[k + "T"]
        moving = T > 0
        assert (np.abs(T - g[k + "length"].sum(axis=0)) <= 1e-9 * np.maximum(T, 1.0)).all(), k
        assert np.array_equal(a[k + "budget"][~moving], np.ones((~moving).sum()))
        assert np.isinf(a[k + "distance_max"][~moving]).all()
        spent, far = status == AG.SPENT, status == AG.DISTANCE
        counts = np.bincount(status, minlength=5)
        assert counts[AG.SPENT] > 0 and counts[AG.DISTANCE] > 0 and counts[AG.MAX_STEPS] == 0, k
        uncut = status >= AG.LEFT
        assert np.array_equal(index[uncut], g[k + "index"][uncut]), k
        assert np.array_equal(a[k + "n_steps"][uncut], g[k + "n_steps"][uncut]), k
        assert np.array_equal(a[k + "depth"][uncut], a[k + "D"][uncut]), k
        assert (index[~uncut, 0] >= 0).all() and (a[k + "n_steps"][~uncut] <= g[k + "n_steps"][~uncut]).all(), k
        assert np.array_equal(a[k + "depth"][spent], a[k + "budget"][spent]), k
        assert np.array_equal(a[k + "distance"][far], a[k + "distance_max"][far]), k
        # what the uncut run met, by the checker (which reproduces the reference's run, above)
        n = status.shape[0]
        full = AG.check(TC.oracle_geometry(case), g[k + "position"], g[k + "direction"], a[k + "density"], box,
                        np.full(n, np.inf), None, float(g[k + "ceiling"]), tally=True)
        assert np.array_equal(full["n_steps"], g[k + "n_steps"])
        tally = full["tally"].astype(np.int64)
        rock_steps += int(tally[:, 0].sum())
        voxel_steps += int(tally[:, 1].sum())
        face_rays += int((tally[:, 2] > 0).sum())
        rock = index[:, 0] == AG.MEDIUM
        within = np.array([AG.inside(box, p) for p in a[k + "position"]])
        spent_inside += int((spent & rock & within).sum())
        far_inside += int((far & rock & within).sum())
        print(f"{k}: status {counts.tolist()}, rock steps {int(tally[:, 0].sum())}, met a voxel "
              f"{int(tally[:, 1].sum())}, in the box: SPENT {int((spent & rock & within).sum())}, DISTANCE "
              f"{int((far & rock & within).sum())}")
    assert voxel_steps >= 0.3 * rock_steps, (voxel_steps, rock_steps)
    assert face_rays >= 100 and spent_inside >= 200 and far_inside >= 50, (face_rays, spent_inside, far_inside)
    # the rough tile's ground rises past the box's top
    top = TA.synth.rough_nodes(TC.N, TC.ROUGH_SEED, TC.ROUGH_AMPLITUDE).max()
    assert top > AG.OFFSET[2] + AG.N[2] * AG.SIZE[2] + 200.0
