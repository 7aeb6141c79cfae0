"""turtle_map_fill_n / turtle_map_node_n without a GPU: the C ABI declares, exports and names the
two calls, every argument error is raised before a device is touched and changes nothing, and
the golden fixture (tests/golden/fill.npz) covers what it is meant to."""
import ctypes as C
import os

import numpy as np
import pytest

import turtle_amd as TA

import fill_cases as FC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST, DEVICE = 0, 1
NX, NY = 5, 4


def test_declared_exported_and_named():
    text = open(os.path.join(ROOT, "include", "turtle_amd.h")).read()
    assert "TURTLE_API enum turtle_return turtle_map_fill_n(" in text
    assert "TURTLE_API enum turtle_return turtle_map_node_n(" in text
    assert "TURTLE_AMD_FILL_CLAMP = 1" in text
    raw = C.CDLL(TA.library_path())
    assert hasattr(raw, "turtle_map_fill_n") and hasattr(raw, "turtle_map_node_n")
    L = TA.lib()
    f = L.turtle_error_function
    f.restype = C.c_char_p
    f.argtypes = [C.c_void_p]
    for name in ("turtle_map_fill_n", "turtle_map_node_n"):
        assert f(C.cast(getattr(L, name), C.c_void_p).value) == name.encode()


@pytest.fixture()
def small():
    z = np.arange(NX * NY, dtype=np.float64).reshape(NY, NX) * 0.5
    m = TA.Map.create(nodes_s2n=z, x=(0, 1), y=(0, 1), z=(0, 65535))
    yield m, FC.scalar_nodes(TA.lib(), m.h, NX, NY)
    m.destroy()


def raised(rc):
    """-> (code name, text of the message the handler got)"""
    pend = list(TA.binding._pending)
    TA.binding._pending.clear()
    text = pend[-1][1].split("} ", 1)[-1] if pend else ""
    return TA.binding.RETURN_NAMES[rc], text


def fill_n(h, ix0, iy0, nx, ny, z, ld, flags=0, space=HOST, clamped=None):
    ptr = z.ctypes.data_as(C.c_void_p) if z is not None else None
    return raised(TA.lib().turtle_map_fill_n(h, ix0, iy0, nx, ny, ptr, C.c_long(ld), flags,
                                             C.byref(clamped) if clamped is not None else None, space))


def node_n(h, ix0, iy0, nx, ny, z, ld, space=HOST):
    ptr = z.ctypes.data_as(C.c_void_p) if z is not None else None
    return raised(TA.lib().turtle_map_node_n(h, ix0, iy0, nx, ny, ptr, C.c_long(ld), space))


def test_fill_n_argument_errors_change_nothing(small):
    m, before = small
    z = np.full((NY, NX), 7.0)
    clamped = C.c_long(-5)
    assert fill_n(None, 0, 0, NX, NY, z, NX)[0] == "BAD_ADDRESS"
    assert fill_n(m.h, 0, 0, NX, NY, None, NX)[0] == "BAD_ADDRESS"
    for window in ((-1, 0, 2, 2), (0, -1, 2, 2), (NX - 1, 0, 2, 1), (0, NY - 1, 1, 2), (0, 0, NX + 1, NY),
                   (NX, 0, 1, 1), (2 ** 31 - 1, 0, 2, 1)):
        assert fill_n(m.h, *window, z, NX + 1, clamped=clamped) == ("DOMAIN_ERROR", "point is outside of map"), window
    code, text = fill_n(m.h, 0, 0, NX, NY, z, NX - 1)
    assert code == "DOMAIN_ERROR" and "leading dimension" in text
    for flags in (2, 3, -1):
        code, text = fill_n(m.h, 0, 0, NX, NY, z, NX, flags=flags)
        assert code == "DOMAIN_ERROR" and "flags" in text
    for space in (2, -1):
        code, text = fill_n(m.h, 0, 0, NX, NY, z, NX, space=space)
        assert code == "DOMAIN_ERROR" and "space" in text
    assert clamped.value == -5
    assert np.array_equal(FC.scalar_nodes(TA.lib(), m.h, NX, NY), before)


def test_node_n_argument_errors(small):
    m, before = small
    z = np.full((NY, NX + 1), -3.0)
    assert node_n(None, 0, 0, NX, NY, z, NX + 1)[0] == "BAD_ADDRESS"
    assert node_n(m.h, 0, 0, NX, NY, None, NX)[0] == "BAD_ADDRESS"
    for window in ((-1, 0, 2, 2), (0, -1, 2, 2), (NX - 1, 0, 2, 1), (0, NY - 1, 1, 2), (0, 0, NX, NY + 1)):
        assert node_n(m.h, *window, z, NX + 1) == ("DOMAIN_ERROR", "point is outside of map"), window
    code, text = node_n(m.h, 0, 0, NX, NY, z, NX - 1)
    assert code == "DOMAIN_ERROR" and "leading dimension" in text
    code, text = node_n(m.h, 0, 0, NX, NY, z, NX + 1, space=7)
    assert code == "DOMAIN_ERROR" and "space" in text
    assert (z == -3.0).all()
    assert np.array_equal(FC.scalar_nodes(TA.lib(), m.h, NX, NY), before)


def test_empty_windows_succeed(small):
    m, before = small
    z = np.full((NY, NX), 9.0)
    clamped = C.c_long(-5)
    for nx, ny in ((0, 3), (3, 0), (0, 0), (-2, 2), (2, -2)):
        # (wherever the corner is, whatever ld says)
        assert fill_n(m.h, 40, -3, nx, ny, z, 0, clamped=clamped)[0] == "SUCCESS"
        assert node_n(m.h, 40, -3, nx, ny, z, 0)[0] == "SUCCESS"
    assert (z == 9.0).all()
    assert np.array_equal(FC.scalar_nodes(TA.lib(), m.h, NX, NY), before)


@pytest.mark.skipif(TA.device_count() > 0, reason="a GPU is present")
def test_no_device_is_a_library_error(small):
    m, before = small
    z = np.full((NY, NX), 7.0)
    for space in (HOST, DEVICE):
        assert fill_n(m.h, 0, 0, NX, NY, z, NX, space=space)[0] == "LIBRARY_ERROR"
        assert fill_n(m.h, 1, 1, 2, 2, z, NX, flags=1, space=space)[0] == "LIBRARY_ERROR"
        assert node_n(m.h, 0, 0, NX, NY, z, NX, space=space)[0] == "LIBRARY_ERROR"
    assert (z == 7.0).all()
    with pytest.raises(TA.TurtleError) as e:
        m.fill_array(z)
    assert e.value.name == "LIBRARY_ERROR" and "no CPU path" in str(e.value)
    with pytest.raises(TA.TurtleError) as e:
        m.nodes()
    assert e.value.name == "LIBRARY_ERROR"
    assert np.array_equal(FC.scalar_nodes(TA.lib(), m.h, NX, NY), before)


def test_binding_row_strides():
    B = TA.binding
    wide = np.zeros((6, 10))
    assert B._row_stride(wide) == 10 and B._row_stride(wide[1:4, 2:7]) == 10
    assert B._row_stride(wide[:, ::2]) == 0 and B._row_stride(wide[::-1]) == 0
    assert B._row_stride(wide.astype(np.float32)) == 0
    assert B._row_stride(wide[2:3, 1:4]) == 3  # (one row: any distance does)
    z, ld = B._rows(wide[:, ::2], HOST)
    assert ld == 5 and z.flags.c_contiguous
    z, ld = B._rows(wide[1:4, 2:7], HOST)
    assert ld == 10 and np.shares_memory(z, wide)
    with pytest.raises(ValueError):
        B._rows(np.zeros(4), HOST)


def test_the_fixture_covers_what_it_is_meant_to(golden):
    g = golden("fill")
    for name, (z0, z1) in FC.SPANS.items():
        v, refused, codes = g[f"{name}_values"], g[f"{name}_refused"], g[f"{name}_codes"]
        assert np.array_equal(v.view(np.uint64), FC.values(name).view(np.uint64))  # (the sign of -0.0 too)
        dz = FC.dz_of((z0, z1))
        top = z0 + 65535 * dz
        # the reference refuses exactly what is off the span [ref map.c:195-201]
        assert np.array_equal(refused, (v < z0) | (v > top))
        assert 100 < refused.sum() < len(v) // 2
        assert refused[3] and refused[4] and not refused[:3].any()  # the next doubles outside; the ends
        assert codes[0] == 0 and codes[1] == 65535
        # exact half-integers round away from zero, their neighbours to either side
        if name in ("unit", "quarter"):
            for n, k in enumerate(FC.HALF_K):
                assert v[9 + 3 * n] == z0 + (k + 0.5) * dz and codes[9 + 3 * n] == k + 1, (name, k)
                # (z0 = 0: z - z0 is exact, a neighbour of the half-integer stays one)
                assert name != "unit" or list(codes[9 + 3 * n:12 + 3 * n]) == [k + 1, k, k + 1], k
        # every code is round((z - z0) / dz), halves away from zero [ref map.c:47-51]
        q = (v[~refused] - z0) / dz
        low = np.floor(q)
        assert np.array_equal(codes[~refused], (low + (q - low >= 0.5)).astype(np.uint16))
        assert len(v) >= 9 + 3 * len(FC.HALF_K) + FC.N_RANDOM
    assert np.signbit(g["unit_values"][7]) and g["unit_codes"][7] == 0 and not g["unit_refused"][7]
    assert g["negative_refused"][7] is not None and g["negative_codes"][7] == round(100 / FC.dz_of((-100.0, 3000.0)))
