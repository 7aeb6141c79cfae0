"""turtle_map_fill_n / turtle_map_node_n on the GPU: against what the reference's turtle_map_fill
stores (tests/golden/fill.npz), against the scalar loops over twin maps, all or nothing, and seen
by every reader afterwards.

Every comparison of codes and node values is exact equality.  The one check with a bar is the
trace of a stepper after a fill, against the CPU checker in oracle/: identical medium and 1e-6
on the path length, the bar of tests/test_gpu_parity.py (libm against OCML)."""
import ctypes as C

import numpy as np
import pytest

import turtle_amd as TA
from oracle import ffi as O
from turtle_amd import synth

import fill_cases as FC
import resample_cases as RC
import terrains as T

pytestmark = pytest.mark.gpu

HOST, DEVICE = 0, 1
SENTINEL = -777.25
D = C.c_double


def decoded(codes, span):
    """turtle_map_node's value of default-encoding codes [ref map.c:41-44]"""
    return span[0] + codes.astype(np.float64) * FC.dz_of(span)


def raw_fill_n(m, ix0, iy0, z, flags=0, clamped=None):
    """the C call on a numpy array -> (code name, text)"""
    rc = TA.lib().turtle_map_fill_n(m.h, ix0, iy0, z.shape[1], z.shape[0], z.ctypes.data_as(C.c_void_p),
                                    C.c_long(z.strides[0] // 8), flags,
                                    C.byref(clamped) if clamped is not None else None, HOST)
    pend = list(TA.binding._pending)
    TA.binding._pending.clear()
    return TA.binding.RETURN_NAMES[rc], (pend[-1][1].split("} ", 1)[-1] if pend else "")


# ---- the reference's codes -------------------------------------------------------------

@pytest.mark.parametrize("name", list(FC.SPANS))
def test_reference_golden(golden, name):
    g = golden("fill")
    span = FC.SPANS[name]
    v, refused, codes = g[f"{name}_values"], g[f"{name}_refused"], g[f"{name}_codes"]

    def window(values, want_codes):
        ny, nx = FC.window_shape(len(values))
        z = np.full(ny * nx, span[0])
        z[:len(values)] = values
        c = np.zeros(ny * nx, dtype=np.uint16)
        c[:len(values)] = want_codes
        return z.reshape(ny, nx), c.reshape(ny, nx)

    ny, nx = FC.window_shape(len(v))
    m = TA.Map.create(shape=(ny + 3, nx + 4), x=(0, 1), y=(0, 1), z=span)
    try:
        zero = decoded(np.zeros((ny + 3, nx + 4), dtype=np.uint16), span)
        assert np.array_equal(m.nodes(), zero)
        # what the reference accepted: its codes
        z, want = window(v[~refused], codes[~refused])
        assert m.fill_array(z, 2, 1) == 0
        after = zero.copy()
        after[1:1 + z.shape[0], 2:2 + nx] = decoded(want, span)
        assert np.array_equal(m.nodes(), after)
        assert np.array_equal(FC.scalar_nodes(TA.lib(), m.h, nx + 4, ny + 3), after)
        # with what it refused among them: nothing changes
        z, _ = window(v, codes)
        with pytest.raises(TA.TurtleError) as e:
            m.fill_array(z, 2, 1)
        assert e.value.name == "DOMAIN_ERROR" and "elevation is outside of map span" in str(e.value)
        assert np.array_equal(m.nodes(), after)
        assert np.array_equal(FC.scalar_nodes(TA.lib(), m.h, nx + 4, ny + 3), after)
        # clamped: the nearest end of the span
        top = span[0] + 65535 * FC.dz_of(span)
        _, want = window(v, np.where(refused, np.where(v < span[0], 0, 65535), codes).astype(np.uint16))
        assert m.fill_array(z, 2, 1, clamp=True) == int(refused.sum())
        after[1:1 + z.shape[0], 2:2 + nx] = decoded(want, span)
        assert np.array_equal(m.nodes(), after)
        assert np.array_equal(FC.scalar_nodes(TA.lib(), m.h, nx + 4, ny + 3), after)
        assert after.max() == top and after.min() == span[0]
    finally:
        m.destroy()


# ---- the scalar loop -------------------------------------------------------------------

@pytest.mark.parametrize("shape", FC.SHAPES)
def test_twin_maps_against_the_scalar_loop(tmp_path, shape):
    nx, ny = shape
    span = (-100.0, 3000.0)
    L = TA.lib()
    one = TA.Map.create(shape=(ny, nx), x=(0, 1), y=(0, 1), z=span)
    two = TA.Map.create(shape=(ny, nx), x=(0, 1), y=(0, 1), z=span)
    rng = np.random.default_rng(nx * 100 + ny)
    try:
        # the whole map first (no HBM copy yet) and last (over a current one)
        for k, (ix0, iy0, wx, wy, pad) in enumerate(FC.windows(nx, ny) + [(0, 0, nx, ny, 0)]):
            wide = np.full((wy, wx + pad), np.nan)  # (what lies between the rows is not read)
            wide[:, :wx] = span[0] + (span[1] - span[0]) * rng.random((wy, wx))
            z = wide[:, :wx]
            FC.scalar_fill(L, one.h, ix0, iy0, z)
            assert two.fill_array(z, ix0, iy0) == 0
            want = FC.scalar_nodes(L, one.h, nx, ny)
            assert np.array_equal(want[iy0:iy0 + wy, ix0:ix0 + wx], decoded(RC.quantise(z, span[0], FC.dz_of(span))[0], span))
            # 1. turtle_map_node loops
            assert np.array_equal(FC.scalar_nodes(L, two.h, nx, ny), want), k
            # 2. turtle_map_node_n of the whole map, and into rows with padding
            assert np.array_equal(two.nodes(), want), k
            assert np.array_equal(one.nodes(), want), k
            out = np.full((ny, nx + 5), SENTINEL)
            assert two.nodes(out=out[:, 2:2 + nx]) is not None
            assert np.array_equal(out[:, 2:2 + nx], want)
            assert (out[:, :2] == SENTINEL).all() and (out[:, 2 + nx:] == SENTINEL).all()
            sub = two.nodes(ix0, iy0, wx, wy)
            assert np.array_equal(sub, want[iy0:iy0 + wy, ix0:ix0 + wx])
            # 3. turtle_map_dump: the same file
            one.dump(str(tmp_path / "one.png"))
            two.dump(str(tmp_path / "two.png"))
            assert open(tmp_path / "one.png", "rb").read() == open(tmp_path / "two.png", "rb").read(), k
    finally:
        one.destroy()
        two.destroy()


def test_signed_map(tmp_path):
    """an hgt tile stores (int16)z: truncation toward zero"""
    n = 1201
    path = synth.write_hgt(str(tmp_path), 45, 2, n)
    one, two = TA.Map.load(path), TA.Map.load(path)
    L = TA.lib()
    try:
        base = synth.srtm_like_nodes(45, 2, n).astype(np.float64)
        assert np.array_equal(two.nodes(), base)
        z = np.tile(np.array([12.7, -12.7, -0.4, 0.4, -1.0, 32767.9, -32766.5, 99.999]), 50).reshape(20, 20)
        FC.scalar_fill(L, one.h, 5, 3, z)  # columns 5 .. 24, rows 3 .. 22: across block corners
        assert two.fill_array(z, 5, 3) == 0
        got = two.nodes()
        assert np.array_equal(got, one.nodes())
        assert np.array_equal(got[3:23, 5:25], z.astype(np.int16).astype(np.float64))
        assert got[3, 5] == 12.0 and got[3, 6] == -12.0 and got[3, 7] == 0.0
        base[3:23, 5:25] = np.trunc(z)
        assert np.array_equal(got, base)
        assert np.array_equal(FC.scalar_nodes(L, two.h, 30, 30), FC.scalar_nodes(L, one.h, 30, 30))
        # the whole tile, more nodes than one pass of the kernels' grids takes
        z = base * 0.5 - 0.25
        assert two.fill_array(z) == 0
        assert np.array_equal(two.nodes(), np.trunc(z))
        node, zz = L.turtle_map_node, D()
        for ix, iy in np.random.default_rng(5).integers(0, n, (300, 2)):
            assert node(two.h, int(ix), int(iy), None, None, C.byref(zz)) == 0
            assert zz.value == np.trunc(z[iy, ix])
        # below the span of an hgt tile
        bad = z.copy()
        bad[-1, -1] = -32768.0
        with pytest.raises(TA.TurtleError) as e:
            two.fill_array(bad)
        assert e.value.name == "DOMAIN_ERROR"
        assert np.array_equal(two.nodes(), np.trunc(z))
    finally:
        one.destroy()
        two.destroy()


# ---- all or nothing --------------------------------------------------------------------

def test_all_or_nothing():
    nx, ny = 19, 13
    span = (-100.0, 3000.0)
    m = TA.Map.create(shape=(ny, nx), x=(0.0, 1.8), y=(0.0, 1.2), z=span)
    L = TA.lib()
    try:
        rng = np.random.default_rng(11)
        assert m.fill_array(2900.0 * rng.random((ny, nx))) == 0
        before = m.nodes()
        x = np.tile(np.arange(nx) * (1.8 / (nx - 1)), ny)
        y = np.repeat(np.arange(ny) * (1.2 / (ny - 1)), nx)
        z_before, in_before = m.elevation(x, y)
        assert in_before.sum() >= (nx - 1) * (ny - 1)
        rows_before = FC.scalar_nodes(L, m.h, nx, ny)
        assert np.array_equal(rows_before, before)
        clamped = C.c_long(-5)
        for value, flags in ((np.nan, 0), (3000.5, 0), (-100.5, 0), (np.nan, 1), (np.inf, 0)):
            z = 1000.0 * rng.random((5, 6))
            z[-1, -1] = value  # (every other element would be stored)
            assert raw_fill_n(m, 5, 4, z, flags, clamped) == ("DOMAIN_ERROR", "elevation is outside of map span")
            assert clamped.value == -5
            assert np.array_equal(m.nodes(), before)
            z_after, in_after = m.elevation(x, y)
            assert np.array_equal(z_after, z_before) and np.array_equal(in_after, in_before)
            assert np.array_equal(FC.scalar_nodes(L, m.h, nx, ny), rows_before)
        # the same rows clamped: stored, and counted
        z[-1, -1], z[0, 0] = 3000.5, -1e300
        assert raw_fill_n(m, 5, 4, z, 1, clamped) == ("SUCCESS", "") and clamped.value == 2
        got = m.nodes()
        assert got[4 + 4, 5 + 5] == span[0] + 65535 * FC.dz_of(span) and got[4, 5] == span[0]
        assert not np.array_equal(got, before)
    finally:
        m.destroy()


def test_a_descending_span_takes_nothing():
    """dz < 0 [ref map.c:195-201]: z != z0 is "inconsistent", and z0 itself lies above z0 + 65535 dz.
    The scalar call's messages, a NaN apart; clamped, everything is stored as z0."""
    m = TA.Map.create(shape=(4, 9), x=(0, 1), y=(0, 1), z=(10.0, 0.0))
    try:
        for value, text in ((5.0, "inconsistent elevation value"), (10.0, "elevation is outside of map span")):
            with pytest.raises(TA.TurtleError) as e:
                m.fill(1, 1, value)
            assert text in str(e.value)
        z = np.full((3, 4), 10.0)
        assert raw_fill_n(m, 2, 1, z) == ("DOMAIN_ERROR", "elevation is outside of map span")
        z[1, 2] = np.nan
        assert raw_fill_n(m, 2, 1, z) == ("DOMAIN_ERROR", "elevation is outside of map span")
        assert raw_fill_n(m, 2, 1, z, 1) == ("DOMAIN_ERROR", "elevation is outside of map span")
        z[1, 2] = 5.0
        assert raw_fill_n(m, 2, 1, z) == ("DOMAIN_ERROR", "inconsistent elevation value")
        assert (m.nodes() == 10.0).all()
        assert m.fill_array(z, 2, 1, clamp=True) == 12
        assert (m.nodes() == 10.0).all()
    finally:
        m.destroy()


# ---- readers ---------------------------------------------------------------------------

def check_trace(t, ref):
    assert np.array_equal(t["index"][:, 0], ref["index"][:, 0])
    rel = np.abs(t["length"] - ref["length"]) / np.maximum(np.abs(ref["length"]), 1e-300)
    rel[ref["length"] == 0] = np.abs(t["length"][ref["length"] == 0])
    assert rel.max() <= 1e-6, rel.max()


def test_readers_see_the_change():
    nx, ny = 67, 45
    nodes = synth.c1_gradient_nodes(nx, ny)
    m = TA.Map.create(shape=(ny, nx), x=T.C1_X, y=T.C1_Y, z=T.C1_Z)
    st = TA.Stepper()
    st.add_map(m, 0.0)
    try:
        assert m.fill_array(nodes) == 0
        geo = O.OracleGeometry(grids=[O.default_grid(nodes, T.C1_X, T.C1_Y, T.C1_Z)], layers=[[(O.MAP, 0, 0.0)]])
        lat, lon, az, el = synth.uniform_rays(2000, T.C1_Y, T.C1_X, seed=9)
        pos0, _ = geo.position(lat, lon, 500.0)
        d = O.ecef_from_horizontal(lat, lon, az, el)
        ref0 = geo.trace(pos0, d)
        t0 = st.trace(pos0.copy(), d)  # the stepper's tables hold the map now
        check_trace(t0, ref0)
        x = np.tile(T.C1_X[0] + np.arange(nx) * ((T.C1_X[1] - T.C1_X[0]) / (nx - 1)), ny)
        y = np.repeat(T.C1_Y[0] + np.arange(ny) * ((T.C1_Y[1] - T.C1_Y[0]) / (ny - 1)), nx)
        z_old, _ = m.elevation(x, y)
        # a wall across the rays' path
        wall = np.full((ny, 3), 1990.0)
        assert m.fill_array(wall, 30, 0) == 0
        nodes[:, 30:33] = wall
        geo = O.OracleGeometry(grids=[O.default_grid(nodes, T.C1_X, T.C1_Y, T.C1_Z)], layers=[[(O.MAP, 0, 0.0)]])
        ref1 = geo.trace(pos0, d)
        t1 = st.trace(pos0.copy(), d)
        check_trace(t1, ref1)
        changed = ref1["length"] != ref0["length"]
        assert changed.sum() > 200 and not np.array_equal(t1["length"], t0["length"])
        assert np.array_equal(t1["length"][~changed], t0["length"][~changed])
        # the batch lookup at the nodes, and the scalar one on the host
        want = m.nodes()
        assert np.array_equal(want, decoded(O.default_grid_raw(nodes, *T.C1_Z), T.C1_Z))
        z, inside = m.elevation(x, y)
        zo, io = geo.grid_elevation(0, x, y)
        assert np.array_equal(inside, io) and np.array_equal(z[io != 0], zo[io != 0])
        moved = (z != z_old).reshape(ny, nx)
        assert moved[:, 30:33].all() and not moved[:, :29].any() and not moved[:, 34:-1].any()
        rng = np.random.default_rng(3)
        xs = T.C1_X[0] + rng.random(300) * (T.C1_X[1] - T.C1_X[0])
        ys = T.C1_Y[0] + rng.random(300) * (T.C1_Y[1] - T.C1_Y[0])
        zo, _ = geo.grid_elevation(0, xs, ys)
        TA.set_scalar("host")
        try:
            zs = np.array([m.elevation_scalar(xs[k], ys[k])[0] for k in range(300)])
        finally:
            TA.set_scalar("device")
        assert np.array_equal(zs, zo)
    finally:
        st.destroy()
        m.destroy()


# ---- spaces ----------------------------------------------------------------------------

def test_device_space_gives_the_host_bits():
    import torch
    nx, ny = 65, 9
    span = (-100.0, 3000.0)
    one = TA.Map.create(shape=(ny, nx), x=(0, 1), y=(0, 1), z=span)
    two = TA.Map.create(shape=(ny, nx), x=(0, 1), y=(0, 1), z=span)
    try:
        rng = np.random.default_rng(21)
        z = span[0] + 3100.0 * rng.random((ny, nx))
        z[2, 3] = 3000.5
        wide = torch.full((ny + 2, nx + 7), float("nan"), dtype=torch.float64, device="cuda")
        wide[1:1 + ny, 3:3 + nx] = torch.as_tensor(z, device="cuda")
        piece = wide[1:1 + ny, 3:3 + nx]  # not contiguous: ld = nx + 7
        torch.cuda.synchronize()  # (torch's stream is not the library's)
        assert not piece.is_contiguous() and TA.binding._rows(piece, DEVICE)[0].data_ptr() == piece.data_ptr()
        with pytest.raises(TA.TurtleError) as e:
            two.fill_array(piece)
        assert e.value.name == "DOMAIN_ERROR"
        assert one.fill_array(z, clamp=True) == 1 and two.fill_array(piece, clamp=True) == 1
        want = one.nodes()
        assert np.array_equal(two.nodes(), want)
        # a window, from the device and from the host, over the other's nodes
        assert one.fill_array(piece[2:5, 10:31], 7, 4) == 0
        assert two.fill_array(np.ascontiguousarray(z[2:5, 10:31]), 7, 4) == 0
        want = one.nodes()
        assert np.array_equal(two.nodes(), want) and np.array_equal(want[4:7, 7:28], one.nodes(7, 4, 21, 3))
        # reads into device memory: a tensor of its own, and a slice that keeps its padding
        got = two.nodes(device=True)
        TA.synchronize()  # device arrays: the call returns once its launch is queued
        assert got.is_cuda and got.dtype == torch.float64 and np.array_equal(got.cpu().numpy(), want)
        out = torch.full((ny + 2, nx + 7), SENTINEL, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        two.nodes(out=out[1:1 + ny, 3:3 + nx])
        TA.synchronize()
        host = out.cpu().numpy()
        assert np.array_equal(host[1:1 + ny, 3:3 + nx], want)
        host[1:1 + ny, 3:3 + nx] = SENTINEL
        assert (host == SENTINEL).all()
        part = two.nodes(60, 5, device=True)  # to the map's corner
        TA.synchronize()
        assert tuple(part.shape) == (4, 5) and np.array_equal(part.cpu().numpy(), want[5:, 60:])
    finally:
        one.destroy()
        two.destroy()


# ---- beside the other calls ------------------------------------------------------------

def test_nodes_after_a_resample(tmp_path, golden):
    g = golden("resample")
    nx, ny, x, y, z, proj, _ = RC.CASES["a"]
    m = TA.Map.create(shape=(ny, nx), x=x, y=y, z=z, projection=proj)
    stack = TA.Stack(RC.tile_dir(tmp_path, "ground"), 0)
    try:
        assert m.fill_array(decoded(RC.sentinel(nx, ny), z)) == 0
        assert np.array_equal(m.nodes(), decoded(RC.sentinel(nx, ny), z))
        outside, clamped = m.resample(stack=stack)
        assert outside == int(g["a_outside"].sum()) and clamped == 0
        assert np.array_equal(m.nodes(), decoded(g["a_codes"], z))
        on_device = m.nodes(device=True)
        TA.synchronize()
        assert np.array_equal(on_device.cpu().numpy(), decoded(g["a_codes"], z))
    finally:
        m.destroy()
        stack.destroy()


def test_view_guard():
    m = TA.Map.create(shape=(9, 12), x=T.C1_X, y=T.C1_Y, z=T.C1_Z)
    st = TA.Stepper()
    st.add_map(m, 0.0)
    try:
        z = np.full((4, 5), 700.0)
        assert m.fill_array(z, 1, 1) == 0
        before = m.nodes()
        with st.view():
            with pytest.raises(TA.TurtleError) as e:
                m.fill_array(z + 1.0, 1, 1)
            assert e.value.name == "DOMAIN_ERROR" and "holds a device view" in str(e.value)
            assert np.array_equal(m.nodes(), before)
        assert m.fill_array(z + 1.0, 1, 1) == 0
        assert not np.array_equal(m.nodes(), before)
    finally:
        st.destroy()
        m.destroy()
