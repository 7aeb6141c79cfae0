"""turtle_stepper_normal_n without a GPU: the C ABI declares, exports, names and checks the call;
the definition restated over the compiled reference (tests/normal_cases.py) reproduces
tests/golden/normal.npz bit for bit; and the binding turns crossings into layers as documented."""
import ctypes as C
import os

import numpy as np
import pytest

import turtle_amd as TA
from oracle import ref_ffi as R

import normal_cases as NC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_normal_declared_exported_and_named():
    text = open(os.path.join(ROOT, "include", "turtle_amd.h")).read()
    assert "TURTLE_API enum turtle_return turtle_stepper_normal_n(" in text
    assert hasattr(C.CDLL(TA.library_path()), "turtle_stepper_normal_n")
    L = TA.lib()
    f = L.turtle_error_function
    f.restype = C.c_char_p
    f.argtypes = [C.c_void_p]
    assert f(C.cast(L.turtle_stepper_normal_n, C.c_void_p).value) == b"turtle_stepper_normal_n"
    device = open(os.path.join(ROOT, "include", "turtle_amd_device.h")).read()
    assert "int normal(const Geometry<MODE, MATH> & g" in device


def test_normal_argument_errors():
    """checked before anything touches a device"""
    st = TA.Stepper()
    st.add_flat(0.0)
    L = TA.lib()
    p = np.zeros((4, 3))
    lay = np.zeros(4, dtype=np.int32)
    di = np.zeros(4, dtype=np.int32)
    ptr, lptr, dptr = (a.ctypes.data_as(C.c_void_p) for a in (p, lay, di))

    def call(stepper, n, position, layer, normal, data_index):
        rc = L.turtle_stepper_normal_n(stepper, C.c_long(n), position, layer, normal, data_index, TA.HOST)
        TA.binding._pending.clear()
        return TA.binding.RETURN_NAMES[rc]

    try:
        assert [call(None, 4, ptr, lptr, ptr, dptr), call(st.h, 4, None, lptr, ptr, dptr),
                call(st.h, 4, ptr, None, ptr, dptr), call(st.h, 4, ptr, lptr, None, dptr),
                call(st.h, 4, ptr, lptr, ptr, None)] == ["BAD_ADDRESS"] * 5
        assert call(st.h, 0, ptr, lptr, ptr, dptr) == call(st.h, -3, ptr, lptr, ptr, dptr) == "SUCCESS"
        assert not p.any() and not di.any()
    finally:
        st.destroy()


@pytest.mark.skipif(not R.available(), reason="oracle/_ref is not built (no reference sources here)")
@pytest.mark.parametrize("case", NC.CASES)
def test_the_restatement_reproduces_the_fixture(golden, tmp_path, case):
    g = golden("normal")
    geo = NC.reference_geometry(case, str(tmp_path))
    try:
        position, layer = NC.positions(case)
        assert np.array_equal(position, g[case + "_position"]) and np.array_equal(layer, g[case + "_layer"])
        out = NC.restate(geo, position, layer)
    finally:
        NC.destroy(geo)
    for name, value in out.items():
        assert np.array_equal(value, g[f"{case}_{name}"]), (case, name)
    R.errors()


def test_the_fixture_holds_what_it_is_meant_to(golden):
    g = golden("normal")
    found = g["map_data_index"] >= 0
    # (a): the half-cell quadrants of an interior cell, the rims, the first half-row, a node, outside
    assert found[:15].all() and not found[15:17].any() and g["map_position"].shape[0] == 257
    assert g["map_latitude"][14] == 0.0 and g["map_longitude"][14] == 0.0            # on node (8, 8)
    assert g["map_glat"][9] == 0.0 and g["map_glat"][8] != 0.0                       # the slip: gy untouched
    assert not (g["map_data_index"][-3:] >= 0).any()                                 # no such layer
    # (b): tile interiors, both sides of the seams, the missing tile
    assert found.sum() > 200 and (g["stack_data_index"][:3] == 0).all() and (g["stack_data_index"][3:5] == -1).all()
    # (d): both data of the middle layer answer, every layer index occurs
    for case in ("layers", "layers_geoid"):
        middle = g[case + "_layer"] == 1
        assert {-1, 0, 1} <= set(g[case + "_data_index"][middle])
        assert set(g[case + "_layer"]) == {-1, 0, 1, 2, 3}
    flat = g["layers_layer"] == 0
    assert not g["layers_glon"][flat].any() and g["layers_geoid_glon"][g["layers_geoid_layer"] == 0].any()
    for case in NC.CASES:
        n = g[case + "_normal"][g[case + "_data_index"] >= 0]
        assert np.abs(np.linalg.norm(n, axis=1) - 1).max() <= 2.0 ** -51


def test_crossing_layers_are_the_minimum_of_the_pair():
    media = np.array([[[1, 0], [2, 3], [1, -1]],
                      [[0, 1], [0, 0], [0, 0]]], dtype=np.int32)     # [capacity 2][n 3][2]
    layer = TA.Stepper.crossing_layers(media)
    # slot-major; {m, -1} (left the data) -> -1: no layer; an EMPTY slot {0, 0} -> layer 0: callers
    # mask the slots by n_crossings
    assert layer.dtype == np.int32 and layer.tolist() == [0, 2, -1, 0, 0, 0]
