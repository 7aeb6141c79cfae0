"""The recipes of tests/composite_cases.py do what tests/test_gpu_composite.py relies on, from the
CPU restatement alone (itself pinned on them to the reference: test_oracle_golden.py, g14)."""
import numpy as np
import pytest

import composite_cases as CO
import crossings_cases as CC


@pytest.fixture(scope="module", params=CO.CASES)
def made(request):
    return request.param, CO.oracle_geometry(request.param)


def test_graze_rays_are_long_and_start_where_layers_end(made):
    case, geo = made
    pos, d, has = CO.graze(case, geo)
    t = geo.trace(pos, d, max_steps=CO.GRAZE_MAX_STEPS, threads=8)
    assert (t["n_steps"] > 512).sum() >= 300 and (t["n_steps"] < CO.GRAZE_MAX_STEPS).all()
    assert np.isfinite(t["length"]).all() and (t["index"][:, 0] >= 0).all()
    if case in ("layers", "overlap"):
        assert (~has).sum() >= 100           # the layer below the lid has no data there
    if case != "overlap":
        assert np.unique(t["index"][t["index"][:, 0] == CO.COMPOSITE_LAYER[case], 1]).size >= 2
    # the golden rays are the head of these
    head = CO.graze(case, geo, CO.GOLDEN_RAYS)
    assert np.array_equal(head[0], pos[:CO.GOLDEN_RAYS]) and np.array_equal(head[1], d[:CO.GOLDEN_RAYS])


def test_rays_under_the_composite_layer_change_data_on_their_way(made):
    case, geo = made
    pos, d, _ = CO.under(case, geo)
    assert CO.data_switches(geo, pos, d) >= 50
    t = geo.trace(pos, d, max_steps=CO.GRAZE_MAX_STEPS, threads=8)
    assert (t["n_steps"] > 512).sum() >= 200 and (t["n_steps"] < CO.GRAZE_MAX_STEPS).all()


def test_sight_lines_cross_often_and_seldom_reach_the_cap(made):
    case, geo = made
    pos, d = CO.sight(case)
    ref = CC.check(geo, pos, d, CO.CEILING, max_steps=CO.SIGHT_MAX_STEPS, threads=8)
    assert (ref["n_crossings"] > 1).sum() > CO.SIGHT // 2
    assert (ref["n_steps"] >= CO.SIGHT_MAX_STEPS).sum() < CO.SIGHT // 100
    assert CO.on_a_rim(case, ref["point"]).sum() >= 10      # crossings located on a rim: a cliff face


def test_rim_points_hug_every_rim(made):
    case, _ = made
    lat, lon, eps = CO.rim_points(case)
    assert 0.8 * CO.RIM_POINTS <= lat.size <= CO.RIM_POINTS and set(eps) == set(CO.IC.EPS)
    from oracle import ffi as O
    assert CO.on_a_rim(case, O.ecef_from_geodetic(lat, lon, np.zeros(lat.size)), within=1.01e-4).all()
    assert CO.on_a_rim(case, O.ecef_from_geodetic(lat, lon, np.zeros(lat.size))).sum() < 0.5 * lat.size


def test_the_open_world_overflows_the_same_way_around_its_cap():
    """without a lid a flat never ends: rays run to the cap, and some overflow to NaN.  Which do
    does not depend on where the cap falls, 2800 .. 3200, but for OPEN_LEFT_OUT"""
    geo = CO.oracle_geometry("example_open")
    pos, d, _ = CO.graze("example_open", geo, CO.OPEN_RAYS)
    finite = [np.isfinite(geo.trace(pos, d, max_steps=cap, threads=4)["length"]) for cap in (2800, CO.OPEN_MAX_STEPS, 3200)]
    keep = np.setdiff1d(np.arange(CO.OPEN_RAYS), CO.OPEN_LEFT_OUT)
    assert np.array_equal(finite[0][keep], finite[1][keep]) and np.array_equal(finite[1][keep], finite[2][keep])
    assert sorted(np.flatnonzero(finite[0] != finite[2])) == sorted(CO.OPEN_LEFT_OUT)
    assert 20 < (~finite[1]).sum() < 100
