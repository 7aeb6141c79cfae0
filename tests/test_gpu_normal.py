"""turtle_stepper_normal_n on the GPU: the unit normal of a layer's top surface, against the call's
definition evaluated over the compiled reference (tests/golden/normal.npz, made by
tests/golden/generate_normal.py), against closed forms, and at the crossings that
turtle_stepper_crossings_n records.

The bar.  The kernel evaluates the definition's expressions in its operand order in IEEE doubles;
what can differ from the fixture is the last ulp of OCML's asin / acos / atan2 / sin / cos / tan /
atanh against glibc's, carried through the cell fraction into the gradient.  WORST is the largest
component difference measured on the MI355X over every case of the fixture; the bar is ten times
that.  (A difference above 1e-7 would be a bug, not a tolerance: one ulp of latitude moves a slope
on 200 m of node noise by under 1e-9.)"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import turtle_amd as TA

import normal_cases as NC
from sight_cases import geometries  # noqa: F401 (the fixture, for pytest to find)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# measured on the MI355X, the largest |component - expected| of each case: map 1.2e-16, stack 1.3e-15,
# layers 1.4e-15, layers_geoid 1.5e-15, utm 1.74e-11, lambert 2.17e-11 (the projected maps: the last
# ulp of the projection's functions on x, y of 10^6 m, over the 200 m the central difference spans)
WORST = 2.17e-11
BAR = 10 * WORST
SENTINEL = -7.0
ULP = 2.0 ** -52


def run(st, position, layer):
    out = np.full((np.asarray(position).reshape(-1, 3).shape[0], 3), SENTINEL)
    return st.normal(position, layer, out=out)


def check_against(g, case, normal, data_index):
    want_n, want_i = g[case + "_normal"], g[case + "_data_index"]
    assert np.array_equal(data_index, want_i), case
    none = want_i < 0
    assert np.array_equal(normal[none], np.full((int(none.sum()), 3), SENTINEL)), case   # untouched, to the bit
    length = np.linalg.norm(normal[~none], axis=1)
    worst = np.abs(normal[~none] - want_n[~none]).max()
    print(f"{case}: {int((~none).sum())} normals, worst component difference {worst:.3e}, "
          f"worst | |n| - 1 | {np.abs(length - 1).max():.2e}")
    assert np.abs(length - 1).max() <= 4 * ULP, case
    assert worst <= BAR, (case, worst)
    return worst


@pytest.mark.parametrize("case", NC.CASES)
def test_against_the_reference(golden, geometries, case):
    g = golden("normal")
    normal, data_index = run(geometries(case)["stepper"], g[case + "_position"], g[case + "_layer"])
    check_against(g, case, normal, data_index)
    if case.startswith("layers"):
        assert {0, 1} <= set(data_index[g[case + "_layer"] == 1])   # the map, and the stack where it ends


def test_paged_stack_runs_in_rounds_and_gives_the_resident_bits(golden, geometries):
    g = golden("normal")
    pos, layer = g["stack_position"], g["stack_layer"]
    full, paged = geometries("stack")["stepper"], geometries("stack", 1)["stepper"]
    normal, data_index = run(full, pos, layer)
    assert full.rounds == 1
    p_normal, p_index = run(paged, pos, layer)
    print("rounds over a stack of 3 tiles that keeps 1:", paged.rounds)
    assert paged.rounds > 1
    assert np.array_equal(p_normal, normal) and np.array_equal(p_index, data_index)
    check_against(g, "stack", p_normal, p_index)


@pytest.mark.parametrize("case", ["map", "stack", "lambert", "layers_geoid"])
def test_spaces_and_arithmetics_give_the_same_bits(golden, geometries, case):
    import torch
    g = golden("normal")
    st = geometries(case)["stepper"]
    pos, layer = g[case + "_position"], g[case + "_layer"]
    normal, data_index = run(st, pos, layer)
    d_out = torch.full((pos.shape[0], 3), SENTINEL, dtype=torch.float64, device="cuda")
    d_normal, d_index = st.normal(torch.as_tensor(pos, device="cuda"), torch.as_tensor(layer, device="cuda"),
                                  out=d_out)
    TA.synchronize()
    assert np.array_equal(d_normal.cpu().numpy(), normal) and np.array_equal(d_index.cpu().numpy(), data_index)
    try:
        TA.set_math("strict")
        s_normal, s_index = run(st, pos, layer)
    finally:
        TA.set_math("fast")
    assert np.array_equal(s_normal, normal) and np.array_equal(s_index, data_index)


def test_one_point_and_a_ragged_batch(golden, geometries):
    """n = 1, and n = 257: neither a multiple of a wave nor of a block (the map case has 257 points)"""
    g = golden("normal")
    st = geometries("map")["stepper"]
    pos, layer = g["map_position"], g["map_layer"]
    assert pos.shape[0] == 257
    normal, data_index = run(st, pos, layer)
    for r in (0, 16, 256):
        one_n, one_i = run(st, pos[r:r + 1], layer[r:r + 1])
        assert np.array_equal(one_n[0], normal[r]) and one_i[0] == data_index[r]
    scalar_n, scalar_i = st.normal(pos[:5], 0)        # one layer for all
    assert np.array_equal(scalar_n, normal[:5]) and np.array_equal(scalar_i, data_index[:5])


def _geodetic(position):
    """the kernels' own (strict) latitude and longitude of the positions"""
    try:
        TA.set_math("strict")
        lat, lon, _ = TA.ecef_to_geodetic(position)
    finally:
        TA.set_math("fast")
    return lat, lon


def _frame(lat, lon):
    lam, phi = np.radians(lon), np.radians(lat)
    sl, cl, sp, cp = np.sin(lam), np.cos(lam), np.sin(phi), np.cos(phi)
    zero = np.zeros_like(sl)
    return (np.stack([-sl, cl, zero], 1), np.stack([-cl * sp, -sl * sp, cp], 1),
            np.stack([cl * cp, sl * cp, sp], 1))


def test_a_flat_layer_gives_the_vertical():
    rng = np.random.Generator(np.random.Philox(77))
    lat, lon = rng.uniform(-89.0, 89.0, 300), rng.uniform(-180.0, 180.0, 300)
    pos = TA.ecef_from_geodetic(lat, lon, rng.uniform(-500.0, 5000.0, 300))
    pos[0] = (0.0, 0.0, 6.4e6)                          # the pole: x == 0 && y == 0
    st = TA.Stepper()
    st.add_flat(100.0)
    try:
        normal, data_index = run(st, pos, np.zeros(300, dtype=np.int32))
    finally:
        st.destroy()
    assert (data_index == 0).all()
    la, lo = _geodetic(pos)
    up = _frame(la, lo)[2]
    print("flat: worst |normal - U|", np.abs(normal - up).max())
    assert np.abs(normal - up).max() <= 1e-15


def test_a_plane_in_longitude_gives_the_analytic_tilt():
    """nodes z = 16 ix over z = (0, 65535): the 16-bit codes hold them exactly, the gradient is
    128 m a degree of longitude and none in latitude (away from the first half-row, where the
    reference's slip puts the latitude's 0 into gx)"""
    ix = np.arange(17, dtype=np.float64)
    m = TA.Map.create(np.broadcast_to(16.0 * ix, (17, 17)).copy(), (20.0, 22.0), (-1.0, 1.0), (0.0, 65535.0))
    st = TA.Stepper()
    st.add_map(m, 0.0)
    rng = np.random.Generator(np.random.Philox(78))
    lat, lon = rng.uniform(-0.9, 0.95, 300), rng.uniform(20.05, 21.95, 300)
    pos = TA.ecef_from_geodetic(lat, lon, rng.uniform(0.0, 3000.0, 300))
    try:
        normal, data_index = run(st, pos, np.zeros(300, dtype=np.int32))
    finally:
        st.destroy()
        m.destroy()
    assert (data_index == 0).all()
    la, lo = _geodetic(pos)
    east, _, up = _frame(la, lo)
    s = np.sin(np.radians(la))
    rn = NC.A / np.sqrt(1.0 - NC.E * NC.E * s * s)
    metres_per_degree = (rn + 128.0 * (lo - 20.0)) * np.cos(np.radians(la)) * np.pi / 180.0
    w = up - (128.0 / metres_per_degree)[:, None] * east
    w /= np.linalg.norm(w, axis=1)[:, None]
    print("plane: worst |normal - analytic|", np.abs(normal - w).max())
    assert np.abs(normal - w).max() <= BAR


def _rays(case, n=300):
    """steep rays over ground with no walls: half come down from above every surface, half come up
    from below them all.  (Where a layer's data ends -- the rim of a map, a missing tile, a map laid
    over a stack -- a ray changes medium through a vertical wall, which is no layer's top.)"""
    rng = np.random.Generator(np.random.Philox(79))
    if case == "map":
        boxes = [((-0.9, 0.9), (-0.9, 0.9))]
    else:   # under the map on top; over the stack alone; where the middle layer has no data
        boxes = [((0.35, 1.15), (10.6, 11.4)), ((0.1, 0.9), (10.05, 10.4)), ((1.35, 1.9), (11.55, 11.95))]
    which = rng.integers(0, len(boxes), n)
    lat = np.array([rng.uniform(*boxes[k][0]) for k in which])
    lon = np.array([rng.uniform(*boxes[k][1]) for k in which])
    down = np.arange(n) % 2 == 0
    el = np.where(down, -1.0, 1.0) * rng.uniform(60.0, 85.0, n)
    pos = TA.ecef_from_geodetic(lat, lon, np.where(down, 3500.0, -500.0))
    return pos, TA.ecef_from_horizontal(lat, lon, rng.uniform(0.0, 360.0, n), el)


@pytest.mark.parametrize("case", ["layers", "map"])
def test_a_crossing_lies_on_the_top_of_layer_min(geometries, case):
    st = geometries(case)["stepper"]
    pos, direction = _rays(case)
    n = pos.shape[0]
    try:
        TA.set_math("strict")
        t = st.crossings(pos.copy(), direction, altitude_max=3600.0, max_steps=200, capacity=8)
        point, media = t["point"], t["media"]
        slot = np.arange(8)[:, None] < np.minimum(t["n_crossings"], 8)[None, :]
        assert t["n_crossings"].max() <= 8
        real = slot & (media[..., 1] >= 0)                 # {m, -1}: left the data, no surface
        layer = np.minimum(media[..., 0], media[..., 1])
        lat, lon, _ = TA.ecef_to_geodetic(point.reshape(-1, 3))
    finally:
        TA.set_math("fast")
    assert real.sum() >= n                                 # every ray crossed something
    if case == "layers":
        assert {(3, 2), (2, 1), (1, 0), (2, 0), (0, 1), (1, 2), (2, 3), (0, 2)} <= \
            {tuple(p) for p in media[real]}
    worst = 0.0
    for k in np.unique(layer[real]):
        pick = np.flatnonzero((real & (layer == k)).reshape(-1))
        on, di = st.position(lat[pick], lon[pick], 0.0, int(k))
        assert (di >= 0).all()
        worst = max(worst, np.linalg.norm(on - point.reshape(-1, 3)[pick], axis=1).max())
    print(f"{case}: {int(real.sum())} crossings, the farthest {worst:.2e} m from the top of layer min(a, b)")
    assert worst <= 1e-6

    normal, data_index = st.normal_at_crossings(point, media)
    assert normal.shape == point.shape and data_index.shape == media.shape[:2]
    assert (data_index[real] >= 0).all()
    assert (data_index[slot & ~real] == -1).all()          # left the data: no layer, reported
    along = np.einsum("cnk,nk->cn", normal, direction)
    going_down = media[..., 0] > media[..., 1]             # into min(a, b) = b
    assert (along[real & going_down] < 0).all() and (along[real & ~going_down] > 0).all()
    assert (real & going_down).any() and (real & ~going_down).any()


@pytest.fixture(scope="module")
def normal_loop(tmp_path_factory):
    """tests/c/normal_loop.hip, built as tests/device_loops.py builds its kernels"""
    import device_loops as DL
    so = os.path.join(str(tmp_path_factory.mktemp("normal_loop")), "libnormal_loop.so")
    made = subprocess.run([DL.HIPCC] + DL.FLAGS + ["-fPIC", "-shared", os.path.join(ROOT, "tests", "c", "normal_loop.hip"),
                                                   "-o", so], capture_output=True, text=True)
    assert made.returncode == 0, made.stderr[-4000:]
    return C.CDLL(so)


@pytest.mark.parametrize("math", ["fast", "strict"])
def test_the_device_function_gives_the_bits_of_the_call(golden, geometries, normal_loop, math):
    import torch
    g = golden("normal")
    st = geometries("map")["stepper"]
    pos, layer = g["map_position"], g["map_layer"]
    normal, data_index = run(st, pos, layer)
    d_pos, d_layer = torch.as_tensor(pos, device="cuda"), torch.as_tensor(layer, device="cuda")
    d_out = torch.full((pos.shape[0], 3), SENTINEL, dtype=torch.float64, device="cuda")
    d_index = torch.full((pos.shape[0],), -9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with st.view() as view:
        rc = normal_loop.normal_loop(view, {"fast": 0, "strict": 1}[math], 2, None, C.c_long(pos.shape[0]),
                                     C.c_void_p(d_pos.data_ptr()), C.c_void_p(d_layer.data_ptr()),
                                     C.c_void_p(d_out.data_ptr()), C.c_void_p(d_index.data_ptr()))
    assert rc == 0
    assert np.array_equal(d_out.cpu().numpy(), normal) and np.array_equal(d_index.cpu().numpy(), data_index)
