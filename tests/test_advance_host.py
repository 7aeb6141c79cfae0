"""turtle_stepper_advance_n without a GPU: the C ABI declares, exports, names and checks the call; the
CPU checker (tests/c/advance_loop.c over the oracle's restatement) and, where it is built, the
compiled reference reproduce tests/golden/advance.npz bit for bit; and the fixture holds what the
GPU tests lean on."""
import ctypes as C
import os

import numpy as np
import pytest

import turtle_amd as TA
from oracle import ref_ffi as R

import advance_cases as AC
import traverse_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_advance_declared_exported_named_and_bound():
    text = open(os.path.join(ROOT, "include", "turtle_amd.h")).read()
    assert "TURTLE_API enum turtle_return turtle_stepper_advance_n(" in text
    for value, name in enumerate(("SPENT", "DISTANCE", "LEFT", "CEILING", "MAX_STEPS")):
        assert f"TURTLE_AMD_ADVANCE_{name} = {value}" in text
        assert getattr(TA, "ADVANCE_" + name) == getattr(AC, name) == value
    assert hasattr(C.CDLL(TA.library_path()), "turtle_stepper_advance_n")
    L = TA.lib()
    f = L.turtle_error_function
    f.restype = C.c_char_p
    f.argtypes = [C.c_void_p]
    assert f(C.cast(L.turtle_stepper_advance_n, C.c_void_p).value) == b"turtle_stepper_advance_n"
    assert callable(TA.Stepper.advance)


def test_advance_argument_errors():
    """checked before anything touches a device; the outputs stay as they were"""
    st = TA.Stepper()
    st.add_flat(0.0)
    L = TA.lib()
    pos, d, rho, b, dm = np.ones((4, 3)), np.ones((4, 3)), np.ones(2), np.ones(4), np.ones(4)
    idx, nst, sta = (np.full(s, -3, dtype=np.int32) for s in ((4, 2), 4, 4))
    dep, dis = np.full(4, -7.0), np.full(4, -8.0)
    POS, D, RHO, B, DM, IDX, NST, STA, DEP, DIS = (a.ctypes.data_as(C.c_void_p)
                                                   for a in (pos, d, rho, b, dm, idx, nst, sta, dep, dis))

    def call(stepper=st.h, n=4, position=POS, direction=D, density=RHO, budget=B, distance_max=DM,
             max_steps=10, index=IDX, depth=DEP, distance=DIS, n_steps=NST, status=STA, space=TA.HOST):
        rc = L.turtle_stepper_advance_n(stepper, C.c_long(n), position, direction, density, budget,
                                        distance_max, C.c_double(np.inf), max_steps, index, depth, distance,
                                        n_steps, status, space)
        TA.binding._pending.clear()
        return TA.binding.RETURN_NAMES[rc]

    try:
        assert [call(stepper=None), call(position=None), call(direction=None), call(density=None),
                call(budget=None), call(index=None), call(status=None)] == ["BAD_ADDRESS"] * 7
        assert [call(max_steps=-1), call(space=2), call(space=-1)] == ["DOMAIN_ERROR"] * 3
        assert call(n=0) == call(n=-3) == call(n=0, distance_max=None, depth=None) == "SUCCESS"
        assert (pos == 1).all() and (idx == -3).all() and (nst == -3).all() and (sta == -3).all()
        assert (dep == -7).all() and (dis == -8).all()
        # the messages carry the call's own name
        rc = L.turtle_stepper_advance_n(st.h, C.c_long(4), POS, D, RHO, B, DM, C.c_double(np.inf), -1, IDX, DEP,
                                        DIS, NST, STA, TA.HOST)
        assert rc != 0 and "turtle_stepper_advance_n" in TA.binding._pending[-1][1]
        TA.binding._pending.clear()
        with pytest.raises(TA.TurtleError) as err:                     # and through the binding
            st.advance(pos, d, rho, b, max_steps=-1)
        assert err.value.name == "DOMAIN_ERROR"
        with pytest.raises(ValueError):
            st.advance(pos, d, np.ones(3), b)                          # one density a medium
    finally:
        st.destroy()


@pytest.mark.parametrize("case", TC.CASES)
def test_checker_reproduces_the_fixture(golden, case):
    g, a = golden("traverse"), golden("advance")
    geo = TC.oracle_geometry(case)
    for recipe in ("ground", "c2"):
        k = f"{case}_{recipe}_"
        out = AC.check(geo, g[k + "position"], g[k + "direction"], a[k + "density"], a[k + "budget"],
                       a[k + "distance_max"], float(g[k + "ceiling"]))
        for name in AC.OUTPUTS:
            assert np.array_equal(out[name], a[k + name]), (case, recipe, name)


@pytest.mark.skipif(not R.available(), reason="oracle/_ref is not built (no reference sources here)")
@pytest.mark.parametrize("case", TC.CASES)
def test_the_reference_reproduces_the_fixture(golden, tmp_path, case):
    g, a = golden("traverse"), golden("advance")
    m = R.RefMap.load(TC.write_tile(tmp_path, case))
    st = AC.reference_stepper(case, m)
    try:
        for recipe in ("ground", "c2"):
            k = f"{case}_{recipe}_"
            out = AC.reference_loop(st, g[k + "position"], g[k + "direction"], a[k + "density"], a[k + "budget"],
                                    a[k + "distance_max"], float(g[k + "ceiling"]))
            for name in AC.OUTPUTS:
                assert np.array_equal(out[name], a[k + name]), (case, recipe, name)
    finally:
        st.destroy()
        m.destroy()
    R.errors()


def test_the_fixture_holds_what_it_is_meant_to(golden):
    g, a = golden("traverse"), golden("advance")
    given = AC.golden_budgets(g, golden("crossings"))        # (asserts the margin, ray by ray)
    for case, recipe in AC.BATCHES:
        k = f"{case}_{recipe}_"
        b = given[case, recipe]
        for name in ("budget", "distance_max", "density"):
            assert np.array_equal(b[name], a[k + name]), (k, name)
        status, index = a[k + "status"], a[k + "index"]
        T = g[k + "length"].sum(axis=0)
        moving = T > 0
        assert (b["margin"][moving] >= AC.MARGIN).all(), k
        assert np.array_equal(a[k + "budget"][~moving], np.ones((~moving).sum()))
        assert np.isinf(a[k + "distance_max"][~moving]).all()
        # where and why the recipe's numpy says each ray stops is where and why the reference stops it
        assert np.array_equal(status, b["status"]), k
        assert (np.abs(a[k + "distance"] - b["stop"]) <= 1e-9 * np.maximum(T, 1.0)).all(), k
        counts = np.bincount(status, minlength=5)
        rock = int(((status == AC.SPENT) & (index[:, 0] == 0)).sum())
        print(f"{k}: status {counts.tolist()}, SPENT in rock {rock}, least margin {b['margin'].min():.2e} T")
        assert counts[AC.SPENT] > 0 and counts[AC.DISTANCE] > 0, k
        if case == "two":   # flat layers have no end: no ray of traverse.npz leaves them, the ceiling stops it
            assert (g[k + "index"][:, 0] >= 0).all() and counts[AC.LEFT] == 0 and counts[AC.CEILING] > 0, k
        else:
            assert counts[AC.LEFT] > 0, k
        assert counts[AC.MAX_STEPS] == 0, k
        if recipe == "c2":
            assert rock >= 100, k
        # a cut ray stands inside the medium its last step began in; an uncut one where traverse's does
        uncut = status >= AC.LEFT
        assert np.array_equal(index[uncut], g[k + "index"][uncut]), k
        assert np.array_equal(a[k + "n_steps"][uncut], g[k + "n_steps"][uncut]), k
        assert (index[~uncut, 0] >= 0).all() and (a[k + "n_steps"][~uncut] <= g[k + "n_steps"][~uncut]).all(), k
        spent = status == AC.SPENT
        assert np.array_equal(a[k + "depth"][spent], a[k + "budget"][spent]), k
        far = status == AC.DISTANCE
        assert np.array_equal(a[k + "distance"][far], a[k + "distance_max"][far]), k
