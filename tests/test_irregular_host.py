"""Pin the CPU restatement on irregular tile stacks (tests/irregular_cases.py) against the
reference's own outputs (tests/golden/irregular.npz, written by generate_irregular.py): traces
at both local ranges, elevations and gradients, bit for bit.  What the GPU tests compare with."""
import numpy as np
import pytest

import irregular_cases as IC


@pytest.fixture(scope="module", params=IC.CASES)
def pinned(request, golden):
    case = request.param
    return case, golden("irregular"), IC.oracle_geometry(case)


def test_inputs_are_the_generators(pinned):
    case, g, _ = pinned
    nodes = IC.tile_nodes(case)
    assert IC.sha(np.concatenate([nodes[k].ravel() for k in sorted(nodes)])) == str(g[f"{case}_nodes_sha"])
    pos, d = IC.rays(case, IC.GOLDEN_RAYS)
    assert IC.sha(pos) == str(g[f"{case}_origin_sha"]) and IC.sha(d) == str(g[f"{case}_direction_sha"])
    # the rays of the GPU tests begin with these
    pos2, d2 = IC.rays(case)
    assert np.array_equal(pos2[:IC.GOLDEN_RAYS], pos) and np.array_equal(d2[:IC.GOLDEN_RAYS], d)
    lat, lon = IC.lookup_points(case)
    assert IC.sha(np.stack([lat, lon])) == str(g[f"{case}_points_sha"])


@pytest.mark.parametrize("tag, local_range", [("r1", 1.0), ("r0", 0.0)])
def test_traces_bit_for_bit(pinned, tag, local_range):
    case, g, geo = pinned
    pos, d = IC.rays(case, IC.GOLDEN_RAYS)
    t = geo.trace(pos, d, max_steps=IC.MAX_STEPS, local_range=local_range, threads=4)
    k = f"{case}_{tag}_"
    assert np.array_equal(t["index"], g[k + "index"].astype(np.int32))
    assert np.array_equal(t["length"], g[k + "length"])
    assert np.array_equal(t["n_steps"], g[k + "n_steps"])
    assert IC.sha(t["position"]) == str(g[k + "position_sha"])
    if tag == "r1":
        assert np.array_equal(t["position"], g[k + "position"])
    assert (t["n_steps"] < IC.MAX_STEPS).all()


def test_elevation_and_gradient_bit_for_bit(pinned):
    case, g, geo = pinned
    lat, lon = IC.lookup_points(case)
    z, inside = geo.stack_elevation(0, lat, lon)
    assert np.array_equal(inside, g[f"{case}_inside"].astype(np.int32))
    assert np.array_equal(z, g[f"{case}_z"])
    glat, glon, gin = IC.stack_gradient(geo, case, lat, lon)
    assert np.array_equal(gin, inside)
    assert np.array_equal(glat, g[f"{case}_glat"]) and np.array_equal(glon, g[f"{case}_glon"])
    # the points do hug the edges: both answers, and every resident tile
    assert 0.5 * lat.size < inside.sum() < 0.95 * lat.size
    slots = np.unique(IC.slot_of(case, lat, lon)[inside == 1])
    assert slots.size > 0.8 * len(IC.DIRECTORIES[case][3])


def test_asc_range_is_the_readers_scan():
    """a tile whose first node read (north-west) is its highest: the scan's zmax is the second
    highest [ref asc.c:87-111], and the highest node's code wraps"""
    z = np.array([[3.0, 5.0], [9.0, 1.0]])          # rows south -> north: 9 is read first
    z0, dz = IC.asc_range(z)
    assert (z0, dz) == (1.0, 4.0 / 65535)
    z0, dz = IC.asc_range(z[::-1])
    assert (z0, dz) == (1.0, 8.0 / 65535)
    # some tile of the cases is of that kind: the trap is exercised
    trapped = [k for case in IC.CASES for k, t in IC.tile_nodes(case).items()
               if IC.asc_range(t)[1] != (t.max() - t.min()) / 65535]
    assert trapped
