"""turtle_map_resample without a GPU: the CPU checker (tests/resample_cases.py over the oracle's
restatement) reproduces the reference's maps (tests/golden/resample.npz) bit for bit, and the C ABI
declares, exports and checks the call."""
import ctypes as C
import os

import numpy as np
import pytest

import turtle_amd as TA

import resample_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def checker_codes(g, case, clamp=False):
    m = RC.meta(case)
    src = m["source"]
    if src == "stack":
        z, inside = RC.check(m, stack=RC.ground_oracle())
    elif src == "void":
        z, inside = RC.check(m, stack=RC.void_oracle())
    else:
        sm = RC.meta(src)
        z, inside = RC.check(m, source=RC.map_oracle(sm, g[f"{src}_codes"]), source_meta=sm)
    return RC.expected(m, z, inside, RC.sentinel(m["nx"], m["ny"]), clamp=clamp), inside


@pytest.mark.parametrize("case", list(RC.CASES))
def test_checker_reproduces_the_reference(golden, case):
    g = golden("resample")
    (codes, ok, half), inside = checker_codes(g, case)
    assert np.array_equal(~inside, g[f"{case}_outside"])
    assert np.array_equal(~ok, g[f"{case}_refused"])
    # the reference leaves a node it refused as it was
    assert np.array_equal(np.where(ok, codes, RC.sentinel(RC.meta(case)["nx"], RC.meta(case)["ny"])),
                          g[f"{case}_codes"])
    if f"{case}_clamped_codes" in g:
        (clamped, _, _), _ = checker_codes(g, case, clamp=True)
        assert np.array_equal(clamped, g[f"{case}_clamped_codes"])


def test_the_fixture_covers_what_it_is_meant_to(golden):
    g = golden("resample")
    for case in "abce":  # the missing tile, the edge of map a
        assert 0.02 < g[f"{case}_outside"].mean() < 0.5, case
    assert g["d_outside"].any() and not g["d_outside"].all()
    assert g["f_refused"].any() and not g["f_outside"].any()
    # voids reach the span check: some refused nodes are far below the ground
    (z, inside) = RC.check(RC.meta("f"), stack=RC.void_oracle())
    assert (z[g["f_refused"]] < -1000).sum() > 100
    assert g["a_codes"].shape == (203, 201)


def test_resample_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "turtle_amd.h")).read()
    assert "TURTLE_API enum turtle_return turtle_map_resample(" in text
    assert "TURTLE_AMD_RESAMPLE_CLAMP = 1" in text
    assert hasattr(C.CDLL(TA.library_path()), "turtle_map_resample")
    L = TA.lib()
    f = L.turtle_error_function
    f.restype = C.c_char_p
    f.argtypes = [C.c_void_p]
    assert f(C.cast(L.turtle_map_resample, C.c_void_p).value) == b"turtle_map_resample"


def test_resample_argument_errors_and_no_device():
    """checked before anything touches a device; without one, LIBRARY_ERROR"""
    L = TA.lib()
    m = TA.Map.create(shape=(3, 4), x=(0, 1), y=(0, 1), z=(0, 1))
    src = TA.Map.create(shape=(3, 4), x=(0, 1), y=(0, 1), z=(0, 1))

    def call(target, stack, source, flags=0):
        rc = L.turtle_map_resample(target, stack, source, flags, None, None)
        TA.binding._pending.clear()
        return TA.binding.RETURN_NAMES[rc]

    try:
        assert call(None, None, src.h) == "BAD_ADDRESS"
        assert call(m.h, None, None) == "BAD_ADDRESS"
        assert call(m.h, src.h, src.h) == "DOMAIN_ERROR"  # (any non-NULL stack pointer)
        assert call(m.h, None, m.h) == "DOMAIN_ERROR"
        assert call(m.h, None, src.h, flags=2) == "DOMAIN_ERROR"
        if TA.device_count() == 0:
            assert call(m.h, None, src.h) == "LIBRARY_ERROR"
            with pytest.raises(TA.TurtleError) as e:
                m.resample(source=src)
            assert e.value.name == "LIBRARY_ERROR"
        assert m.node(1, 1)[2] == 0.0
    finally:
        m.destroy()
        src.destroy()
