"""turtle_stepper_crossings_n without a GPU: the CPU checker (tests/c/crossings_loop.c over the
oracle's restatement) reproduces every crossing of the reference's lines of sight
(tests/golden/crossings.npz) bit for bit, and the C ABI declares, exports and checks the call."""
import ctypes as C
import os

import numpy as np

import turtle_amd as TA

import crossings_cases as CC
import traverse_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_checker_reproduces_the_reference(golden):
    g, x = golden("traverse"), golden("crossings")
    for case in TC.CASES:
        geo = TC.oracle_geometry(case)
        for recipe in ("ground", "c2"):
            k = f"{case}_{recipe}_"
            out = CC.check(geo, g[k + "position"], g[k + "direction"], float(g[k + "ceiling"]))
            for name in ("index", "length", "n_steps", "n_crossings"):
                assert np.array_equal(out[name], g[k + name]), (case, recipe, name)
            for name in ("offset", "point", "distance", "media"):
                assert np.array_equal(out[name], x[k + name]), (case, recipe, name)
    # the fixture holds what it is meant to: rays with more than 50 crossings, every pair of the
    # two-layer tile's neighbouring media, rays that leave the data (entered -1)
    assert np.diff(x["rough_c2_offset"]).max() > 50
    pairs = {tuple(p) for p in x["two_ground_media"]} | {tuple(p) for p in x["two_c2_media"]}
    assert {(0, 1), (1, 0), (1, 2), (2, 1)} <= pairs
    assert (x["hgt_c2_media"][:, 1] == -1).sum() > 100


def test_crossings_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "turtle_amd.h")).read()
    assert "TURTLE_API enum turtle_return turtle_stepper_crossings_n(" in text
    assert hasattr(C.CDLL(TA.library_path()), "turtle_stepper_crossings_n")
    L = TA.lib()
    f = L.turtle_error_function
    f.restype = C.c_char_p
    f.argtypes = [C.c_void_p]
    assert f(C.cast(L.turtle_stepper_crossings_n, C.c_void_p).value) == b"turtle_stepper_crossings_n"


def test_crossings_argument_errors():
    """checked before anything touches a device"""
    st = TA.Stepper()
    L = TA.lib()
    p = np.zeros((4, 3))
    idx = np.zeros((4, 2), dtype=np.int32)
    cnt = np.zeros(4, dtype=np.int32)
    ptr, iptr, cptr = (a.ctypes.data_as(C.c_void_p) for a in (p, idx, cnt))

    def call(n, pos, d, max_steps, index, n_crossings, capacity):
        rc = L.turtle_stepper_crossings_n(st.h, C.c_long(n), pos, d, C.c_double(np.inf), max_steps,
                                          index, None, None, n_crossings, capacity, None, None, None,
                                          TA.HOST)
        TA.binding._pending.clear()
        return TA.binding.RETURN_NAMES[rc]

    try:
        assert [call(4, None, ptr, 10, iptr, cptr, 2), call(4, ptr, None, 10, iptr, cptr, 2),
                call(4, ptr, ptr, 10, None, cptr, 2), call(4, ptr, ptr, 10, iptr, None, 2)] \
            == ["BAD_ADDRESS"] * 4
        assert call(4, ptr, ptr, -1, iptr, cptr, 2) == call(4, ptr, ptr, 10, iptr, cptr, -1) \
            == "DOMAIN_ERROR"
        assert call(0, ptr, ptr, 10, iptr, cptr, 2) == call(-3, ptr, ptr, 10, iptr, cptr, 0) == "SUCCESS"
    finally:
        st.destroy()
