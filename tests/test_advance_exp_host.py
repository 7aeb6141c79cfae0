"""turtle_stepper_advance_exp_n without a GPU: the C ABI declares, exports, names and checks the call;
the CPU checker (tests/c/advance_exp_loop.c over the oracle's restatement) and, where it is built,
the compiled reference reproduce tests/golden/advance_exp.npz bit for bit; the fixture holds what the
GPU tests lean on; and with every scale height HUGE_VAL the checker gives advance.npz."""
import ctypes as C
import os

import numpy as np
import pytest

import turtle_amd as TA
from oracle import ref_ffi as R

import advance_exp_cases as AE
import traverse_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_advance_exp_declared_exported_named_and_bound():
    text = open(os.path.join(ROOT, "include", "turtle_amd.h")).read()
    assert "TURTLE_API enum turtle_return turtle_stepper_advance_exp_n(" in text
    assert hasattr(C.CDLL(TA.library_path()), "turtle_stepper_advance_exp_n")
    L = TA.lib()
    f = L.turtle_error_function
    f.restype = C.c_char_p
    f.argtypes = [C.c_void_p]
    assert f(C.cast(L.turtle_stepper_advance_exp_n, C.c_void_p).value) == b"turtle_stepper_advance_exp_n"
    assert f(C.cast(L.turtle_stepper_advance_n, C.c_void_p).value) == b"turtle_stepper_advance_n"
    import inspect
    assert inspect.signature(TA.Stepper.advance).parameters["scale_height"].default is None
    device = open(os.path.join(ROOT, "include", "turtle_amd_device.h")).read()
    assert "double column_depth(double c, double w, double f)" in device
    assert "double column_reach(double c, double w, double R)" in device


def test_advance_exp_argument_errors():
    """checked before anything touches a device; the outputs stay as they were"""
    st = TA.Stepper()
    st.add_flat(0.0)
    L = TA.lib()
    pos, d, rho, sh, b, dm = np.ones((4, 3)), np.ones((4, 3)), np.ones(2), np.ones(2), np.ones(4), np.ones(4)
    idx, nst, sta = (np.full(s, -3, dtype=np.int32) for s in ((4, 2), 4, 4))
    dep, dis = np.full(4, -7.0), np.full(4, -8.0)
    POS, D, RHO, SH, B, DM, IDX, NST, STA, DEP, DIS = (a.ctypes.data_as(C.c_void_p)
                                                       for a in (pos, d, rho, sh, b, dm, idx, nst, sta, dep, dis))

    def call(stepper=st.h, n=4, position=POS, direction=D, density=RHO, scale_height=SH, budget=B,
             distance_max=DM, max_steps=10, index=IDX, depth=DEP, distance=DIS, n_steps=NST, status=STA,
             space=TA.HOST):
        rc = L.turtle_stepper_advance_exp_n(stepper, C.c_long(n), position, direction, density, scale_height,
                                            budget, distance_max, C.c_double(np.inf), max_steps, index, depth,
                                            distance, n_steps, status, space)
        TA.binding._pending.clear()
        return TA.binding.RETURN_NAMES[rc]

    try:
        assert [call(stepper=None), call(position=None), call(direction=None), call(density=None),
                call(budget=None), call(index=None), call(status=None)] == ["BAD_ADDRESS"] * 7
        assert [call(max_steps=-1), call(space=2), call(space=-1)] == ["DOMAIN_ERROR"] * 3
        # no scale heights is no error: with a bad argument beside it, that argument's error
        assert call(scale_height=None, max_steps=-1) == "DOMAIN_ERROR"
        assert call(scale_height=None, budget=None) == "BAD_ADDRESS"
        assert call(n=0) == call(n=-3) == call(n=0, distance_max=None, depth=None) == "SUCCESS"
        assert call(n=0, scale_height=None) == "SUCCESS"
        assert (pos == 1).all() and (idx == -3).all() and (nst == -3).all() and (sta == -3).all()
        assert (dep == -7).all() and (dis == -8).all()
        # the messages carry the name of the call that was made
        rc = L.turtle_stepper_advance_exp_n(st.h, C.c_long(4), POS, D, RHO, SH, B, DM, C.c_double(np.inf), -1, IDX,
                                            DEP, DIS, NST, STA, TA.HOST)
        assert rc != 0 and "turtle_stepper_advance_exp_n" in TA.binding._pending[-1][1]
        TA.binding._pending.clear()
        rc = L.turtle_stepper_advance_n(st.h, C.c_long(4), POS, D, RHO, B, DM, C.c_double(np.inf), -1, IDX, DEP,
                                        DIS, NST, STA, TA.HOST)
        assert rc != 0 and "turtle_stepper_advance_n" in TA.binding._pending[-1][1]
        assert "advance_exp" not in TA.binding._pending[-1][1]
        TA.binding._pending.clear()
        with pytest.raises(TA.TurtleError) as err:                     # and through the binding
            st.advance(pos, d, rho, b, max_steps=-1, scale_height=sh)
        assert err.value.name == "DOMAIN_ERROR" and "turtle_stepper_advance_exp_n" in str(err.value)
        with pytest.raises(ValueError):
            st.advance(pos, d, rho, b, scale_height=np.ones(3))        # one scale height a medium
    finally:
        st.destroy()


@pytest.mark.parametrize("case", TC.CASES)
def test_checker_reproduces_the_fixture(golden, case):
    g, a = golden("traverse"), golden("advance_exp")
    geo = TC.oracle_geometry(case)
    for recipe in ("ground", "c2"):
        k = f"{case}_{recipe}_"
        out = AE.check(geo, g[k + "position"], g[k + "direction"], a[k + "density"], a[k + "scale_height"],
                       a[k + "budget"], a[k + "distance_max"], float(g[k + "ceiling"]))
        for name in AE.OUTPUTS:
            assert np.array_equal(out[name], a[k + name]), (case, recipe, name)
        # uncut: the D and T the fixture's budgets were drawn from
        n = out["status"].shape[0]
        full = AE.check(geo, g[k + "position"], g[k + "direction"], a[k + "density"], a[k + "scale_height"],
                        np.full(n, np.inf), None, float(g[k + "ceiling"]))
        assert np.array_equal(full["depth"], a[k + "D"]) and np.array_equal(full["distance"], a[k + "T"])


@pytest.mark.skipif(not R.available(), reason="oracle/_ref is not built (no reference sources here)")
@pytest.mark.parametrize("case", TC.CASES)
def test_the_reference_reproduces_the_fixture(golden, tmp_path, case):
    g, a = golden("traverse"), golden("advance_exp")
    m = R.RefMap.load(TC.write_tile(tmp_path, case))
    st = AE.reference_stepper(case, m)
    try:
        for recipe in ("ground", "c2"):
            k = f"{case}_{recipe}_"
            out = AE.reference_loop(st, g[k + "position"], g[k + "direction"], a[k + "density"],
                                    a[k + "scale_height"], a[k + "budget"], a[k + "distance_max"],
                                    float(g[k + "ceiling"]))
            for name in AE.OUTPUTS:
                assert np.array_equal(out[name], a[k + name]), (case, recipe, name)
    finally:
        st.destroy()
        m.destroy()
    R.errors()


def test_the_fixture_holds_what_it_is_meant_to(golden):
    g, a = golden("traverse"), golden("advance_exp")
    spent_in_air = far_in_air = 0
    for case, recipe in AE.BATCHES:
        k = f"{case}_{recipe}_"
        media = g[k + "length"].shape[0]
        assert np.array_equal(a[k + "density"], AE.DENSITY[media])
        assert np.array_equal(a[k + "scale_height"], AE.SCALE_HEIGHT[media])
        assert np.isinf(a[k + "scale_height"][:-1]).all() and a[k + "scale_height"][-1] == 8400.0
        status, index = a[k + "status"], a[k + "index"]
        T = a[k + "T"]
        moving = T > 0
        # the uncut loop is traverse's: its path is the sum of traverse's lengths, to rounding
        assert (np.abs(T - g[k + "length"].sum(axis=0)) <= 1e-9 * np.maximum(T, 1.0)).all(), k
        assert np.array_equal(a[k + "budget"][~moving], np.ones((~moving).sum()))
        assert np.isinf(a[k + "distance_max"][~moving]).all()
        air = index[:, 0] == media - 1
        spent, far = status == AE.SPENT, status == AE.DISTANCE
        spent_in_air += int((spent & air).sum())
        far_in_air += int((far & air).sum())
        counts = np.bincount(status, minlength=5)
        print(f"{k}: status {counts.tolist()}, in air: SPENT {int((spent & air).sum())}, DISTANCE "
              f"{int((far & air).sum())}")
        assert counts[AE.SPENT] > 0 and counts[AE.DISTANCE] > 0 and counts[AE.MAX_STEPS] == 0, k
        # a cut ray stands inside the medium its last step began in; an uncut one where traverse's does
        uncut = status >= AE.LEFT
        assert np.array_equal(index[uncut], g[k + "index"][uncut]), k
        assert np.array_equal(a[k + "n_steps"][uncut], g[k + "n_steps"][uncut]), k
        assert np.array_equal(a[k + "depth"][uncut], a[k + "D"][uncut]), k
        assert (index[~uncut, 0] >= 0).all() and (a[k + "n_steps"][~uncut] <= g[k + "n_steps"][~uncut]).all(), k
        assert np.array_equal(a[k + "depth"][spent], a[k + "budget"][spent]), k
        assert np.array_equal(a[k + "distance"][far], a[k + "distance_max"][far]), k
        # the air above is thinner than the air at altitude 0: a ray that only saw air has less depth
        # than its path at 1.205 kg/m^3 (and, under the fixtures' ceilings, more than a tenth of it)
        only_air = moving & (g[k + "length"][:-1].sum(axis=0) == 0) & uncut
        assert (a[k + "depth"][only_air] < 1.205 * T[only_air]).all(), k
    assert spent_in_air >= 200 and far_in_air >= 100, (spent_in_air, far_in_air)


@pytest.mark.parametrize("case", TC.CASES)
def test_uniform_scale_heights_are_advance(golden, case):
    """every scale height HUGE_VAL, and no scale heights at all: advance.npz, bit for bit"""
    g, a = golden("traverse"), golden("advance")
    geo = TC.oracle_geometry(case)
    for recipe in ("ground", "c2"):
        k = f"{case}_{recipe}_"
        for sh in (np.full(a[k + "density"].shape[0], np.inf), None):
            out = AE.check(geo, g[k + "position"], g[k + "direction"], a[k + "density"], sh, a[k + "budget"],
                           a[k + "distance_max"], float(g[k + "ceiling"]))
            for name in AE.OUTPUTS:
                assert np.array_equal(out[name], a[k + name]), (case, recipe, name)
