"""turtle_stepper_clearance_n without a GPU: the C ABI declares, exports, names and checks the call;
the definition restated over the compiled reference (tests/clearance_cases.py) reproduces
tests/golden/clearance.npz bit for bit; and the fixture holds what the GPU tests lean on."""
import ctypes as C
import os

import numpy as np
import pytest

import turtle_amd as TA
from oracle import ref_ffi as R

import clearance_cases as CC
import horizon_cases as HC
import normal_cases as NC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STORED = CC.OUTPUTS + ("profile", "data_index")


def test_clearance_declared_exported_and_named():
    text = open(os.path.join(ROOT, "include", "turtle_amd.h")).read()
    assert "TURTLE_API enum turtle_return turtle_stepper_clearance_n(" in text
    assert "TURTLE_AMD_CLEARANCE_PAIRED = 1" in text and TA.CLEARANCE_PAIRED == 1
    assert hasattr(C.CDLL(TA.library_path()), "turtle_stepper_clearance_n")
    L = TA.lib()
    f = L.turtle_error_function
    f.restype = C.c_char_p
    f.argtypes = [C.c_void_p]
    assert f(C.cast(L.turtle_stepper_clearance_n, C.c_void_p).value) == b"turtle_stepper_clearance_n"
    assert callable(TA.Stepper.clearance)


def test_clearance_argument_errors():
    """checked before anything touches a device; the outputs stay as they were"""
    st = TA.Stepper()
    st.add_flat(0.0)
    L = TA.lib()
    o, t, fr = np.ones((4, 3)), np.ones((5, 3)), np.full(7, 0.5)
    cl = np.full((4, 5), CC.SENTINEL)
    smp, nd = np.full((4, 5), -3, dtype=np.int32), np.full((4, 5), -4, dtype=np.int32)
    O, T, FR, CL, SMP, ND = (a.ctypes.data_as(C.c_void_p) for a in (o, t, fr, cl, smp, nd))
    PAIRED = TA.CLEARANCE_PAIRED

    def call(stepper=st.h, n=4, observer=O, m=5, target=T, n_f=7, fraction=FR, layer=0, flags=0, clearance=CL,
             sample=SMP, n_data=ND, space=TA.HOST):
        rc = L.turtle_stepper_clearance_n(stepper, C.c_long(n), observer, C.c_long(m), target, n_f, fraction,
                                          layer, flags, clearance, sample, n_data, space)
        TA.binding._pending.clear()
        return TA.binding.RETURN_NAMES[rc]

    try:
        assert [call(stepper=None), call(observer=None), call(target=None), call(fraction=None),
                call(clearance=None), call(sample=None)] == ["BAD_ADDRESS"] * 6
        assert [call(layer=-1), call(layer=1), call(space=2), call(space=-1)] == ["DOMAIN_ERROR"] * 4
        assert [call(flags=2), call(flags=3), call(flags=-1), call(flags=1 << 20)] == ["DOMAIN_ERROR"] * 4
        assert call(flags=PAIRED) == call(flags=PAIRED, n=5, m=4) == "DOMAIN_ERROR"       # m != n
        # the number of lines does not fit an int: the kernel's item numbers are ints
        assert call(n=2 ** 31, m=1) == call(n=2 ** 30, m=2) == call(n=2 ** 40, m=5) == call(n=3, m=2 ** 40) \
            == call(n=2 ** 31, m=2 ** 31, flags=PAIRED) == "DOMAIN_ERROR"
        assert call(n=0) == call(n=-3) == call(m=0) == call(m=-1) == call(n_f=0) == call(n_f=-2) \
            == call(n=0, m=0, flags=PAIRED) == "SUCCESS"
        assert (cl == CC.SENTINEL).all() and (smp == -3).all() and (nd == -4).all()
        # the messages: turtle_stepper_position_n's for a layer, the call's own name in the others
        rc = L.turtle_stepper_clearance_n(st.h, C.c_long(4), O, C.c_long(5), T, 7, FR, 3, 0, CL, SMP, ND, TA.HOST)
        assert rc != 0 and TA.binding._pending[-1][1].endswith("no valid data")
        TA.binding._pending.clear()
        rc = L.turtle_stepper_clearance_n(st.h, C.c_long(4), O, C.c_long(5), T, 7, FR, 0, PAIRED, CL, SMP, ND, TA.HOST)
        assert rc != 0 and "turtle_stepper_clearance_n" in TA.binding._pending[-1][1]
        TA.binding._pending.clear()
        with pytest.raises(TA.TurtleError) as err:                     # and through the binding
            st.clearance(o, t, fr, paired=True)
        assert err.value.name == "DOMAIN_ERROR"
    finally:
        st.destroy()


@pytest.mark.skipif(not R.available(), reason="oracle/_ref is not built (no reference sources here)")
@pytest.mark.parametrize("case", CC.CASES)
def test_the_restatement_reproduces_the_fixture(golden, tmp_path, case):
    g = golden("clearance")
    geo = NC.reference_geometry(case, str(tmp_path))
    stepper = HC.reference_stepper(geo)
    try:
        observer, target, fraction = HC.observers(case, stepper), CC.targets(case, stepper), CC.fractions()
        assert np.array_equal(observer, g[case + "_observer"]) and np.array_equal(target, g[case + "_target"])
        assert np.array_equal(fraction, g[case + "_fraction"]) and int(g[case + "_layer"]) == CC.LAYER[case]
        out = CC.restate(stepper, observer, target, fraction, CC.LAYER[case])
        # n_data is compared exactly on the GPU: no sample's data index may hang on an ulp
        assert CC.data_is_robust(stepper, out["latitude"], out["longitude"], out["data_index"], CC.LAYER[case]) == 0
        diagonal = CC.restate(stepper, observer, target[:4], fraction, CC.LAYER[case], paired=True)
    finally:
        stepper.destroy()
        NC.destroy(geo)
    for name in STORED:
        assert np.array_equal(out[name], g[f"{case}_{name}"], equal_nan=True), (case, name)
        assert np.array_equal(diagonal[name], g[f"{case}_{name}"][np.arange(4), np.arange(4)], equal_nan=True), name
    R.errors()


def test_the_fixture_holds_what_it_is_meant_to(golden):
    g = golden("clearance")
    for case in CC.CASES:
        profile, di, fraction = g[case + "_profile"], g[case + "_data_index"], g[case + "_fraction"]
        clearance, sample, n_data = (g[f"{case}_{name}"] for name in CC.OUTPUTS)
        assert profile.shape == (4, 6, 130) and g[case + "_observer"].shape == (4, 3) and g[case + "_target"].shape == (6, 3)
        assert np.array_equal(fraction, (2.0 * np.arange(130) + 1.0) / 260.0)
        assert (fraction > 0).all() and (fraction < 1).all()
        assert np.array_equal(np.isnan(profile), di < 0)
        # the expected outputs are the profile's minimum, the first of equals, and the data's count
        for name, value in CC.expected(profile, di).items():
            assert np.array_equal(value, g[f"{case}_{name}"]), (case, name)
        assert (sample > 0).all()
        gap = CC.gaps(profile).min()
        print(f"{case}: blocked {int((clearance < -1).sum())}, open {int((clearance > 1).sum())}, lines with skipped "
              f"samples {int((n_data < 130).sum())}, winners k + 1 = {sorted(set(sample.ravel().tolist()))}, "
              f"smallest lowest-to-second gap {gap:.3e} m")
        assert (clearance < -1.0).sum() >= 3, case                # clearly blocked lines
        assert (clearance > 1.0).sum() >= 3, case                 # clearly open ones
        assert (n_data < 130).any() and (n_data[:, 5] < 130).all() and (n_data[:, 5] > 0).all(), case
        assert (n_data[:, :2] == 130).all(), case                 # and lines that keep every sample
        assert gap > 1e-5, (case, gap)       # ten times the cap on the GPU test's bar: the sample is pinned
    for case in ("map", "stack", "layers_geoid"):      # (the Lambert map is 3.2 km a side)
        sample = g[case + "_sample"]
        assert (sample <= 64).any() and (sample > 64).any(), case            # both sides of lane 0's second turn
    assert {0, 1} <= set(g["layers_geoid_data_index"].ravel().tolist())       # the map, and the stack where it ends
    assert (g["stack_n_data"][:, :5] < 130).any()                             # a line ACROSS the hole, not only into it
