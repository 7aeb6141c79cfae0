"""turtle_stepper_viewshed_n without a GPU: the C ABI declares, exports, names and checks the call;
the definition restated over the compiled reference (tests/viewshed_cases.py) reproduces
tests/golden/viewshed.npz bit for bit; and the fixture holds what the GPU tests lean on -- above
all that no flag of it hangs on the last digits of a sine."""
import ctypes as C
import os

import numpy as np
import pytest

import turtle_amd as TA
from oracle import ref_ffi as R

import horizon_cases as HC
import normal_cases as NC
import viewshed_cases as VC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 1e-8          # ten times the cap on the GPU test's bar (tests/test_gpu_horizon.py: CAP_SINE)


def test_viewshed_declared_exported_and_named():
    text = open(os.path.join(ROOT, "include", "turtle_amd.h")).read()
    assert "TURTLE_API enum turtle_return turtle_stepper_viewshed_n(" in text
    assert hasattr(C.CDLL(TA.library_path()), "turtle_stepper_viewshed_n")
    L = TA.lib()
    f = L.turtle_error_function
    f.restype = C.c_char_p
    f.argtypes = [C.c_void_p]
    assert f(C.cast(L.turtle_stepper_viewshed_n, C.c_void_p).value) == b"turtle_stepper_viewshed_n"
    assert callable(TA.Stepper.viewshed)


def test_viewshed_argument_errors():
    """checked before anything touches a device; the outputs stay as they were"""
    st = TA.Stepper()
    st.add_flat(0.0)
    L = TA.lib()
    p = np.ones((4, 3))
    az, ds = np.zeros(5), np.ones(7)
    vis = np.full((4, 5, 7), -5, dtype=np.int8)
    sn, hz = np.full((4, 5, 7), HC.SENTINEL), np.full((4, 5, 7), HC.SENTINEL)
    nv = np.full((4, 5), -3, dtype=np.int32)
    P, AZ, DS, VIS, SN, HZ, NV = (a.ctypes.data_as(C.c_void_p) for a in (p, az, ds, vis, sn, hz, nv))

    def call(stepper=st.h, n=4, position=P, n_az=5, azimuth=AZ, n_d=7, distance=DS, layer=0, height=0.0,
             visible=VIS, sine=SN, horizon=HZ, n_visible=NV, space=TA.HOST):
        rc = L.turtle_stepper_viewshed_n(stepper, C.c_long(n), position, n_az, azimuth, n_d, distance, layer,
                                         C.c_double(height), visible, sine, horizon, n_visible, space)
        TA.binding._pending.clear()
        return TA.binding.RETURN_NAMES[rc]

    try:
        assert [call(stepper=None), call(position=None), call(azimuth=None), call(distance=None),
                call(visible=None)] == ["BAD_ADDRESS"] * 5
        assert [call(layer=-1), call(layer=1), call(space=2), call(space=-1)] == ["DOMAIN_ERROR"] * 4
        # n * n_azimuths does not fit an int: the kernel's item numbers are ints
        assert call(n=2 ** 31, n_az=1) == call(n=2 ** 30, n_az=2) == call(n=2 ** 40, n_az=5) == "DOMAIN_ERROR"
        assert call(n=0) == call(n=-3) == call(n_az=0) == call(n_az=-1) == call(n_d=0) == call(n_d=-2) == "SUCCESS"
        assert call(n=0, height=10.0) == "SUCCESS"
        assert (vis == -5).all() and (sn == HC.SENTINEL).all() and (hz == HC.SENTINEL).all() and (nv == -3).all()
        # the messages: turtle_stepper_position_n's for a layer, the call's own name in front
        rc = L.turtle_stepper_viewshed_n(st.h, C.c_long(4), P, 5, AZ, 7, DS, 3, C.c_double(0.0), VIS, SN, HZ, NV,
                                         TA.HOST)
        assert rc != 0 and TA.binding._pending[-1][1].endswith("no valid data")
        assert "turtle_stepper_viewshed_n" in TA.binding._pending[-1][1]
        TA.binding._pending.clear()
    finally:
        st.destroy()


@pytest.mark.skipif(not R.available(), reason="oracle/_ref is not built (no reference sources here)")
@pytest.mark.parametrize("case", VC.CASES)
def test_the_restatement_reproduces_the_fixture(golden, tmp_path, case):
    g, inputs = golden("viewshed"), golden("horizon")
    geo = NC.reference_geometry(case, str(tmp_path))
    stepper = HC.reference_stepper(geo)
    try:
        position, azimuth, distance = HC.observers(case, stepper), HC.azimuths(), HC.distances()
        assert np.array_equal(position, inputs[case + "_position"])          # (the fixture stores no inputs
        assert np.array_equal(azimuth, inputs[case + "_azimuth"])            # of its own: horizon.npz's)
        assert np.array_equal(distance, inputs[case + "_distance"])
        outs = {h: VC.restate(stepper, position, azimuth, distance, VC.LAYER[case], h) for h in VC.TARGET_HEIGHTS}
    finally:
        stepper.destroy()
        NC.destroy(geo)
    for height, out in outs.items():
        assert float(g[f"{case}_{VC.tag(height)}_target_height"]) == height
        for name in VC.OUTPUTS:
            want = g[f"{case}_{VC.tag(height)}_{name}"]
            assert out[name].dtype == want.dtype, (case, height, name)
            assert np.array_equal(out[name], want, equal_nan=(name != "visible")), (case, height, name)
    R.errors()


def test_the_fixture_holds_what_it_is_meant_to(golden):
    g, hg = golden("viewshed"), golden("horizon")
    assert VC.TARGET_HEIGHTS[0] == 0.0 and len(VC.TARGET_HEIGHTS) == 2
    for case in VC.CASES:
        profile = hg[case + "_sine"]
        running = VC.running_maximum(profile)
        for height in VC.TARGET_HEIGHTS:
            key = f"{case}_{VC.tag(height)}"
            visible, sine, horizon, n_visible = (g[f"{key}_{name}"] for name in VC.OUTPUTS)
            assert visible.shape == sine.shape == horizon.shape == (4, 5, 130) and n_visible.shape == (4, 5)
            assert visible.dtype == np.int8 and n_visible.dtype == np.int32
            # the ground's sines do not depend on the target: the horizon is the exclusive running
            # maximum of horizon.npz's profile at either height, and the same samples are skipped
            assert np.array_equal(horizon, running), key
            assert np.array_equal(visible < 0, np.isnan(profile)) and np.array_equal(np.isnan(sine), np.isnan(profile))
            assert set(np.unique(visible).tolist()) == {-1, 0, 1}, key
            want_visible, want_count = VC.follows(sine, horizon, np.isnan(profile))
            assert np.array_equal(visible, want_visible) and np.array_equal(n_visible, want_count), key
            if height == 0.0:
                assert np.array_equal(sine, profile, equal_nan=True), key        # bit for bit
            else:   # a target above the ground stands higher against the sky, except straight below
                both = ~np.isnan(profile)
                both[:, :, 0] = False
                assert (sine[both] > profile[both]).all(), key
                assert (visible >= g[f"{case}_h0_visible"]).all() and (visible > g[f"{case}_h0_visible"]).any()
            # the first sample with data of every line is visible, behind a horizon of -inf
            first = (visible >= 0).argmax(-1)
            assert (np.take_along_axis(visible, first[..., None], -1) == 1).all()
            assert np.isneginf(np.take_along_axis(horizon, first[..., None], -1)).all() and np.isneginf(horizon[..., 0]).all()
            # the observer at height 0: its own foot is skipped; from 2 m up it is a sample
            assert (visible[0, :, 0] == -1).all() and (visible[1:, :, 0] == 1).all(), key
            assert (visible[:, :, 1:] == -1).any(), key                          # rims, the missing tile
            margin = VC.margins(sine, horizon, visible).min()
            print(f"{key}: {int((visible >= 0).sum())} samples with data, {int((visible == 1).sum())} visible, "
                  f"smallest |sine - horizon| {margin:.3e}")
            assert margin > MARGIN, (key, margin)      # a condition: every flag of the fixture is pinned
            if case != "lambert":                      # (3.2 km a side: its data ends before sample 64)
                for half in (visible[:, :, :64], visible[:, :, 64:]):            # both sides of the chunk's end
                    assert (half == 1).any() and (half == 0).any(), key
    assert (g["stack_h0_visible"][:, :, 1:] == -1).any()
    counts = [int((g[f"{case}_h0_visible"] >= 0).sum()) for case in VC.CASES]
    seen = [int((g[f"{case}_h0_visible"] == 1).sum()) for case in VC.CASES]
    assert counts == [2276, 2272, 427, 2151] and seen == [1237, 1297, 133, 1262]
