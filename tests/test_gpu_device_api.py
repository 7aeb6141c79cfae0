"""The device stepper API on the GPU: test kernels written on include/turtle_amd_device.h
(tests/c/device_loops.hip) against the library's own calls on the same inputs.

Bars.  Stepping::trip() and step() against turtle_stepper_traverse_n: the same bits, in both
arithmetics (k_traverse halves on closed-form samples in both).  Per-step records against the
reference's golden vectors at the bar test_gpu_parity.py holds step_n to; STRICT also bit for bit
against turtle_stepper_step_n.  The scattering walk against turtle_stepper_scatter_n: STRICT the same
bits; FAST no ray in another medium or with another step count, positions and lengths within 1e-6
(the figures of test_scattering_walk_against_oracle)."""
import os
import threading

import numpy as np
import pytest

import turtle_amd as TA
from turtle_amd import synth

import amd_build as B
import device_loops as DL
import traverse_cases as TC

pytestmark = pytest.mark.gpu

KEYS = ("position", "index", "length", "n_steps", "n_crossings")


@pytest.fixture(params=["fast", "strict"])
def math(request):
    TA.set_math(request.param)
    yield request.param
    TA.set_math("fast")


def same_bits(a, b, what=""):
    for k in KEYS:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (what, k)


def both_forms(st, math, pos, d, ceiling, what, max_steps=1000000, simple=True):
    """traverse_n, then the Stepping kernel (and the step() kernel) under a view: the same bits"""
    ref = st.traverse(pos.copy(), d, ceiling, max_steps=max_steps)
    with st.view() as v:
        got = DL.traverse(v, math, pos, d, ceiling, max_steps, st.media)
        same_bits(got, ref, what + " trip()")
        if simple:
            got = DL.traverse(v, math, pos, d, ceiling, max_steps, st.media, simple=1)
            same_bits(got, ref, what + " step()")
    return ref


@pytest.fixture(scope="module")
def steppers(tmp_path_factory):
    out, keep = {}, []
    for case in TC.CASES:
        m = TA.Map.load(TC.write_tile(tmp_path_factory.mktemp(case), case))
        st = TA.Stepper()
        if case == "two":
            for off in (-0.5, 0.0):
                st.add_layer()
                st.add_flat(off)
                st.add_map(m, off)
        else:
            st.add_map(m, 0.0)
        out[case] = st
        keep.append(m)
    yield out
    for st in out.values():
        st.destroy()
    for m in keep:
        m.destroy()


@pytest.fixture(scope="module")
def stack2x2(tmp_path_factory):
    """a resident 2 x 2 stack (stack_size 0): the ONE_STACK mode"""
    d = str(tmp_path_factory.mktemp("grid"))
    for la in (45, 46):
        for lo in (3, 4):
            synth.write_hgt(d, la, lo, 1201)
    stack = TA.Stack(d, 0)
    stack.load()
    st = TA.Stepper()
    st.add_stack(stack, 0.0)
    yield st, d
    st.destroy()
    stack.destroy()


def stack_rays(st, n, seed=5, height=300.0):
    rng = np.random.default_rng(seed)
    lat, lon = rng.uniform(45.1, 46.9, n), rng.uniform(3.1, 4.9, n)
    az, el = rng.uniform(0, 360, n), rng.uniform(-8.0, 3.0, n)
    pos, di = st.position(lat, lon, height)
    keep = di == 0
    return pos[keep], TA.ecef_from_horizontal(lat, lon, az, el)[keep]


@pytest.mark.parametrize("recipe", ["ground", "c2"])
@pytest.mark.parametrize("case", TC.CASES)
def test_stepping_and_step_are_traverse_n(steppers, golden, math, case, recipe):
    g = golden("traverse")
    k = f"{case}_{recipe}_"
    both_forms(steppers[case], math, g[k + "position"], g[k + "direction"], float(g[k + "ceiling"]),
               f"{case} {recipe} {math}")


def test_stepping_over_a_resident_stack(stack2x2, math):
    st, _ = stack2x2
    pos, d = stack_rays(st, 20000)
    ref = both_forms(st, math, pos, d, 2000.0, f"stack {math}")
    assert (ref["n_crossings"] > 0).sum() > 100


@pytest.mark.parametrize("name", ["nogeoid", "geoid"])
def test_stepping_with_a_geoid_and_a_projected_map(golden, math, name):
    g = golden("projection")
    m = TA.Map.create(g["nodes"], (495000.0, 497000.0), (5066000.0, 5068000.0), (0.0, 1000.0),
                      projection="UTM 31N")
    geoid = B.geoid_map(g["geoid_nodes"]) if name == "geoid" else None
    st = TA.Stepper()
    if geoid is not None:
        st.geoid_set(geoid)
    st.add_flat(-5.0)
    st.add_map(m, 0.0)
    try:
        both_forms(st, math, g[name + "_pos"], g[name + "_dir"], 1000.0, f"UTM {name} {math}",
                   max_steps=20000)
    finally:
        st.destroy()
        m.destroy()
        if geoid is not None:
            geoid.destroy()


def test_stepping_full_size_tile(math, tmp_path):
    """2e5 rays of the C2 recipe over the 3601 x 3601 tile, a 2000 m ceiling"""
    n = 200000
    m = TA.Map.load(synth.write_hgt(str(tmp_path), 45, 3, synth.HGT_N))
    st = TA.Stepper()
    st.add_map(m, 0.0)
    try:
        lat, lon, az, el = synth.uniform_rays(n, (45, 46), (3, 4), seed=0x5EED2026)
        pos, di = st.position(lat, lon, 500.0)
        assert (di >= 0).all()
        d = TA.ecef_from_horizontal(lat, lon, az, el)
        ref = both_forms(st, math, pos, d, 2000.0, f"hgt3601 {math}")
        assert (ref["n_crossings"] > 1).sum() > n // 10
        # results do not depend on lane or wave: another grid, the same bits
        with st.view() as v:
            for blocks in (7, 1000):
                same_bits(DL.traverse(v, math, pos, d, 2000.0, 1000000, st.media, blocks=blocks), ref,
                          f"{blocks} blocks")
    finally:
        st.destroy()
        m.destroy()


def test_per_step_records(golden, math):
    """G7 on sample() + step(): every step of 16 rays against the reference's records, and in
    STRICT against turtle_stepper_step_n without RESUME, bit for bit"""
    g = golden("steps")
    m = B.c1_map()
    st = B.c1_stepper(m)
    rec = g["record"]
    K = int(rec[:, 1].max())
    with st.view() as v:
        got, taken = DL.records(v, math, g["position"], g["direction"], K)
    pos = g["position"].copy()
    for k in range(1, K + 1):
        rows = rec[rec[:, 1] == k]
        rays = rows[:, 0].astype(int)
        mine = got[k - 1, rays]
        assert (taken[rays] >= k).all()
        assert np.array_equal(mine[:, 9:11].astype(np.int32), rows[:, 6:8].astype(np.int32))
        assert np.abs(mine[:, 3] - rows[:, 5]).max() <= 1e-6 * np.abs(rows[:, 5]).max()
        assert np.abs(mine[:, 0:3] - rows[:, 2:5]).max() < 1e-5
        if math == "strict":
            o = st.step(pos[rays].copy(), g["direction"][rays])
            assert np.array_equal(o["position"], mine[:, 0:3])
            assert np.array_equal(o["step"], mine[:, 3])
            assert np.array_equal(o["latitude"], mine[:, 4]) and np.array_equal(o["longitude"], mine[:, 5])
            assert np.array_equal(o["altitude"], mine[:, 6])
            assert np.array_equal(o["elevation"], mine[:, 7:9])
            assert np.array_equal(o["index"], mine[:, 9:11].astype(np.int32))
            pos[rays] = o["position"]
    st.destroy()
    m.destroy()


def test_a_scattering_walk_in_the_callers_kernel_is_scatter_n(stack2x2, math):
    st, _ = stack2x2
    n, K = 100000, 64
    lat, lon, _, _ = synth.uniform_rays(n, (45.0, 47.0), (3.0, 5.0), seed=8)
    pos, di = st.position(lat, lon, 20.0)
    pos = pos[di == 0]
    ref = st.scatter(pos.copy(), 4242, K, first_ray=17)
    o = st.step(pos.copy(), None)   # the origins' samples
    start = dict(position=pos.copy(), altitude=o["altitude"], elevation=o["elevation"], index=o["index"],
                 length=np.zeros(pos.shape[0]), steps=np.zeros(pos.shape[0], dtype=np.int32))
    with st.view() as v:
        got = DL.walk(v, math, start, 4242, K, first_ray=17)
        two = DL.walk(v, math, DL.walk(v, math, start, 4242, 10, first_ray=17), 4242, K - 10,
                      first_ray=17, first_step=10, blocks=33)
    flips = int(((got["index"][:, 0] != ref["index"][:, 0]) | (got["steps"] != ref["steps"])).sum())
    print(f"{math}: {flips} rays of {pos.shape[0]} in another medium or with another step count; "
          f"positions differ by {np.abs(got['position'] - ref['position']).max():.2e} m at most, "
          f"lengths by {np.abs(got['length'] - ref['length']).max():.2e} m")
    if math == "strict":
        for key in ("position", "index", "length", "steps"):
            assert np.array_equal(got[key], ref[key]), key
    else:
        assert flips == 0, flips
        assert np.abs(got["position"] - ref["position"]).max() < 1e-6
        assert np.abs(got["length"] - ref["length"]).max() <= max(1e-6 * ref["length"].max(), 1e-7)
    for key in ("position", "index", "length", "steps"):   # in two calls, on another grid
        assert np.array_equal(two[key], got[key]), key
    assert (ref["steps"] == K).sum() > n // 2


def in_time(call, seconds=120):
    """runs `call` in a thread of its own... no: a view belongs to the thread that holds it, so the
    call runs HERE, and a watchdog reports a hang instead of waiting for ever"""
    done = threading.Event()

    def watchdog():
        if not done.wait(seconds):
            os.write(2, b"a call made with a view out did not return\n")
            os._exit(3)

    t = threading.Thread(target=watchdog, daemon=True)
    t.start()
    try:
        return call()
    finally:
        done.set()


def test_lifetime_of_a_view(stack2x2, tmp_path):
    st, tiles = stack2x2
    TA.set_math("strict")
    pos, d = stack_rays(st, 5000, seed=11)
    m = B.c1_map()
    small = TA.Stack(tiles, 2)       # room for 2 of its 4 tiles
    paged = TA.Stepper()
    paged.add_stack(small, 0.0)
    try:
        ref = st.traverse(pos.copy(), d, 2000.0)
        with st.view() as v:
            # a batch call on the same resident stepper, then the kernel: the same bits as before
            same_bits(st.traverse(pos.copy(), d, 2000.0), ref, "batch call with the view out")
            same_bits(DL.traverse(v, "strict", pos, d, 2000.0, 1000000, st.media), ref, "kernel")
            # what would change the geometry fails in the holding thread, and does not hang
            for call in (lambda: m.fill(0, 0, 10.0), lambda: small.clear(), lambda: small.load(),
                         lambda: paged.traverse(pos.copy(), d, 2000.0), lambda: st.add_flat(0.0)):
                with pytest.raises(TA.TurtleError) as e:
                    in_time(call)
                assert e.value.name == "DOMAIN_ERROR" and "view" in str(e.value)
            with pytest.raises(TA.TurtleError) as e:   # one view of a stepper at a time
                in_time(lambda: st.view().__enter__())
            assert e.value.name == "DOMAIN_ERROR"
            same_bits(DL.traverse(v, "strict", pos, d, 2000.0, 1000000, st.media), ref, "after the errors")
        with pytest.raises(TA.TurtleError) as e:       # released already
            TA.binding._check(TA.lib().turtle_amd_stepper_view_release(st.h))
        assert e.value.name == "DOMAIN_ERROR"
        with pytest.raises(TA.TurtleError) as e:       # a stack that cannot keep its tiles
            with paged.view():
                pass
        assert e.value.name == "DOMAIN_ERROR" and "stack_size" in str(e.value)
        # after the release everything works as before
        m.fill(0, 0, 10.0)
        t = paged.traverse(pos.copy(), d, 2000.0)
        same_bits(t, ref, "the paged stepper after the release")
        same_bits(st.traverse(pos.copy(), d, 2000.0), ref, "after the release")
    finally:
        TA.set_math("fast")
        paged.destroy()
        small.destroy()
        m.destroy()
