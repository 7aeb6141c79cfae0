"""turtle_stepper_horizon_n without a GPU: the C ABI declares, exports, names and checks the call;
the definition restated over the compiled reference (tests/horizon_cases.py) reproduces
tests/golden/horizon.npz bit for bit; and the fixture holds what the GPU tests lean on."""
import ctypes as C
import os

import numpy as np
import pytest

import turtle_amd as TA
from oracle import ref_ffi as R

import horizon_cases as HC
import normal_cases as NC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_horizon_declared_exported_and_named():
    text = open(os.path.join(ROOT, "include", "turtle_amd.h")).read()
    assert "TURTLE_API enum turtle_return turtle_stepper_horizon_n(" in text
    assert hasattr(C.CDLL(TA.library_path()), "turtle_stepper_horizon_n")
    L = TA.lib()
    f = L.turtle_error_function
    f.restype = C.c_char_p
    f.argtypes = [C.c_void_p]
    assert f(C.cast(L.turtle_stepper_horizon_n, C.c_void_p).value) == b"turtle_stepper_horizon_n"
    assert callable(TA.Stepper.horizon)


def test_horizon_argument_errors():
    """checked before anything touches a device; the outputs stay as they were"""
    st = TA.Stepper()
    st.add_flat(0.0)
    L = TA.lib()
    p = np.ones((4, 3))
    az, ds = np.zeros(5), np.ones(7)
    el, rg = np.full((4, 5), HC.SENTINEL), np.full((4, 5), HC.SENTINEL)
    smp = np.full((4, 5), -3, dtype=np.int32)
    P, AZ, DS, EL, RG, SMP = (a.ctypes.data_as(C.c_void_p) for a in (p, az, ds, el, rg, smp))

    def call(stepper=st.h, n=4, position=P, n_az=5, azimuth=AZ, n_d=7, distance=DS, layer=0, elevation=EL,
             sample=SMP, range_=RG, space=TA.HOST):
        rc = L.turtle_stepper_horizon_n(stepper, C.c_long(n), position, n_az, azimuth, n_d, distance, layer,
                                        elevation, sample, range_, space)
        TA.binding._pending.clear()
        return TA.binding.RETURN_NAMES[rc]

    try:
        assert [call(stepper=None), call(position=None), call(azimuth=None), call(distance=None),
                call(elevation=None), call(sample=None)] == ["BAD_ADDRESS"] * 6
        assert [call(layer=-1), call(layer=1), call(space=2), call(space=-1)] == ["DOMAIN_ERROR"] * 4
        # n * n_azimuths does not fit an int: the kernel's item numbers are ints
        assert call(n=2 ** 31, n_az=1) == call(n=2 ** 30, n_az=2) == call(n=2 ** 40, n_az=5) == "DOMAIN_ERROR"
        assert call(n=0) == call(n=-3) == call(n_az=0) == call(n_az=-1) == call(n_d=0) == call(n_d=-2) == "SUCCESS"
        assert (el == HC.SENTINEL).all() and (rg == HC.SENTINEL).all() and (smp == -3).all()
        # the messages: turtle_stepper_position_n's for a layer, the call's own name in the others
        rc = L.turtle_stepper_horizon_n(st.h, C.c_long(4), P, 5, AZ, 7, DS, 3, EL, SMP, RG, TA.HOST)
        assert rc != 0 and TA.binding._pending[-1][1].endswith("no valid data")
        TA.binding._pending.clear()
    finally:
        st.destroy()


@pytest.mark.skipif(not R.available(), reason="oracle/_ref is not built (no reference sources here)")
@pytest.mark.parametrize("case", HC.CASES)
def test_the_restatement_reproduces_the_fixture(golden, tmp_path, case):
    g = golden("horizon")
    geo = NC.reference_geometry(case, str(tmp_path))
    stepper = HC.reference_stepper(geo)
    try:
        position, azimuth, distance = HC.observers(case, stepper), HC.azimuths(), HC.distances()
        assert np.array_equal(position, g[case + "_position"]) and np.array_equal(azimuth, g[case + "_azimuth"])
        assert np.array_equal(distance, g[case + "_distance"]) and int(g[case + "_layer"]) == HC.LAYER[case]
        out = HC.restate(stepper, position, azimuth, distance, HC.LAYER[case])
    finally:
        stepper.destroy()
        NC.destroy(geo)
    for name, value in out.items():
        assert np.array_equal(value, g[f"{case}_{name}"], equal_nan=True), (case, name)
    R.errors()


def test_the_fixture_holds_what_it_is_meant_to(golden):
    g = golden("horizon")
    for case in HC.CASES:
        sine, sample, distance = g[case + "_sine"], g[case + "_sample"], g[case + "_distance"]
        assert sine.shape == (4, 5, 130) and distance.shape == (130,) and distance[0] == 0.0
        assert (np.diff(distance) > 0).all() and distance[1] == 500.0 and distance[-1] == 150e3
        # the expected outputs are the profile's maximum, the first of equals
        filled = np.where(np.isnan(sine), -np.inf, sine)
        assert np.array_equal(sample, np.where(np.isinf(filled.max(-1)), 0, filled.argmax(-1) + 1))
        assert (sample > 0).all()
        # lines with samples outside the data, beyond the sample at the observer's foot
        assert np.isnan(sine[:, :, 1:]).any(), case
        # the observer at height 0: its own foot (distance 0) is skipped, the next sample is not;
        # from 2 m up the foot is a sample, straight down
        assert np.isnan(sine[0, :, 0]).all() and np.isfinite(sine[0, :, 1]).all(), case
        assert (g[case + "_data_index"][0, :, 0] == -1).all()
        assert np.abs(sine[1:, :, 0] + 1.0).max() < 1e-12, case
        gap = HC.gaps(sine).min()
        print(f"{case}: winners k + 1 = {sorted(set(sample.ravel().tolist()))}, smallest best-to-second gap {gap:.3e}")
        assert gap > 1e-8, (case, gap)       # ten times the GPU test's cap on its bar
    for case in ("map", "stack", "layers_geoid"):      # (the Lambert map is 3.2 km a side: its winners are near)
        sample = g[case + "_sample"]
        assert (sample <= 64).any() and (sample > 64).any(), case            # both sides of lane 64's turn
        assert sample.min() >= 2 and sample.max() <= 130
    assert {0, 1} <= set(g["layers_geoid_data_index"].ravel().tolist())       # the map, and the stack where it ends
    assert (g["stack_data_index"] == -1)[:, :, 1:].any()                      # the missing tile, the rims
