"""turtle_stepper_traverse_n without a GPU: the CPU checker (tests/c/traverse_loop.c over the
oracle's restatement) reproduces the reference's lines of sight (tests/golden/traverse.npz) bit
for bit, the rough test tile is pinned, and the C ABI declares, exports and checks the call."""
import ctypes as C
import hashlib
import os

import numpy as np

import turtle_amd as TA
from turtle_amd import synth

import traverse_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_checker_reproduces_the_reference(golden):
    g = golden("traverse")
    for case in TC.CASES:
        geo = TC.oracle_geometry(case)
        for recipe in ("ground", "c2"):
            k = f"{case}_{recipe}_"
            out = TC.check(geo, g[k + "position"], g[k + "direction"], float(g[k + "ceiling"]))
            for name in ("index", "length", "n_steps", "n_crossings"):
                assert np.array_equal(out[name], g[k + name]), (case, recipe, name)
    # the fixture holds what it is meant to: many crossings on the rough tile, all three media of
    # the two-layer one, rays that end outside the data, rays that start above the ceiling
    assert g["rough_c2_n_crossings"].max() > 50
    assert (g["two_c2_length"] > 0).any(axis=1).all()
    assert (g["hgt_c2_index"][:, 0] == -1).sum() > 100
    assert (g["hgt_c2_n_steps"][-16:] == 0).all() and (g["hgt_c2_n_steps"][:-32] > 0).all()


def test_rough_tile_is_pinned(golden):
    z = synth.rough_nodes(TC.N, TC.ROUGH_SEED, TC.ROUGH_AMPLITUDE)
    assert hashlib.sha256(z.tobytes()).hexdigest() == str(golden("traverse")["rough_nodes_sha"])
    assert z.dtype == np.int16 and z.shape == (TC.N, TC.N)
    assert 0 < np.abs(np.diff(z.astype(int), axis=1)).mean() < 400 and z.max() - z.min() > 1500
    assert not np.array_equal(synth.rough_nodes(65, 1), synth.rough_nodes(65, 2))


def test_traverse_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "turtle_amd.h")).read()
    for name in ("turtle_stepper_traverse_n", "turtle_amd_stepper_media"):
        assert f"TURTLE_API" in text and f"{name}(" in text
        assert hasattr(C.CDLL(TA.library_path()), name)
    L = TA.lib()
    f = L.turtle_error_function
    f.restype = C.c_char_p
    f.argtypes = [C.c_void_p]
    assert f(C.cast(L.turtle_stepper_traverse_n, C.c_void_p).value) == b"turtle_stepper_traverse_n"


def test_traverse_argument_errors():
    """checked before anything touches a device"""
    st = TA.Stepper()
    L = TA.lib()
    p = np.zeros((4, 3))
    idx = np.zeros((4, 2), dtype=np.int32)
    ptr, iptr = p.ctypes.data_as(C.c_void_p), idx.ctypes.data_as(C.c_void_p)

    def call(n, pos, d, max_steps, index):
        rc = L.turtle_stepper_traverse_n(st.h, C.c_long(n), pos, d, C.c_double(np.inf), max_steps,
                                         index, None, None, None, TA.HOST)
        TA.binding._pending.clear()
        return TA.binding.RETURN_NAMES[rc]

    try:
        assert [call(4, None, ptr, 10, iptr), call(4, ptr, None, 10, iptr), call(4, ptr, ptr, 10, None)] \
            == ["BAD_ADDRESS"] * 3
        assert call(4, ptr, ptr, -1, iptr) == "DOMAIN_ERROR"
        assert call(0, ptr, ptr, 10, iptr) == call(-3, ptr, ptr, 10, iptr) == "SUCCESS"
        assert L.turtle_amd_stepper_media(st.h) == 1
        st.add_layer()
        assert L.turtle_amd_stepper_media(st.h) == 2
    finally:
        st.destroy()
