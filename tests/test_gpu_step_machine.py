"""The edges of the ray queue that k_walk (queue_refill, device_common.h) and k_traverse (its own copy of
that loop) draw from, and of the step machine k_walk shares with Stepping::trip() (step_or_bisect,
turtle_amd_device.h; k_traverse has its own copy of that too).

257 rays over a resident 2 x 2 stack, every third one starting outside the data (k_walk loads
such a ray and draws again; k_traverse ends it at its origin sample), one with a NaN direction
component.  Each call is made on the first 1, 63, 64, 65 and 257 of them: 64 is what a wave draws
at once, so at 63 and 65 a wave has lanes that draw nothing, and a second draw that finds the
queue dry.  Rays are independent, so the rows of a short call are those of the long one BIT FOR
BIT (NaNs included: the bytes are compared), and the long traverse is the Stepping loop of
tests/c/device_loops.hip over the same rays; any difference is the queue's or the machine's."""
import numpy as np
import pytest

import turtle_amd as TA
from turtle_amd import synth

import device_loops as DL

pytestmark = pytest.mark.gpu

N = 257
SIZES = (1, 63, 64, 65, 257)
CEILING = 2000.0


@pytest.fixture(params=["fast", "strict"])
def math(request):
    TA.set_math(request.param)
    yield request.param
    TA.set_math("fast")


@pytest.fixture(scope="module")
def stack2x2(tmp_path_factory):
    """a resident 2 x 2 stack (stack_size 0), as in test_gpu_device_api.py"""
    d = str(tmp_path_factory.mktemp("grid"))
    for la in (45, 46):
        for lo in (3, 4):
            synth.write_hgt(d, la, lo, 1201)
    stack = TA.Stack(d, 0)
    stack.load()
    st = TA.Stepper()
    st.add_stack(stack, 0.0)
    yield st
    st.destroy()
    stack.destroy()


@pytest.fixture(scope="module")
def rays(stack2x2):
    rng = np.random.default_rng(257)
    lat, lon = rng.uniform(45.1, 46.9, N), rng.uniform(3.1, 4.9, N)
    az, el = rng.uniform(0, 360, N), rng.uniform(-8.0, 3.0, N)
    pos, di = stack2x2.position(lat, lon, 300.0)
    outside = (np.arange(N) % 3 == 0) | (di != 0)
    pos[outside] = TA.ecef_from_geodetic(lat[outside] + 3.0, lon[outside], np.full(outside.sum(), 1000.0))
    d = TA.ecef_from_horizontal(lat, lon, az, el)
    d[np.flatnonzero(~outside)[33], 1] = np.nan
    pos.setflags(write=False)
    d.setflags(write=False)
    return pos, d, outside


def same_bytes(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert a.tobytes() == b.tobytes(), what


@pytest.mark.parametrize("max_steps", [0, 1, 50])
def test_traverse_of_the_first_rays_is_the_whole_batch(stack2x2, rays, math, max_steps):
    st = stack2x2
    pos, d, outside = rays
    ref = st.traverse(pos.copy(), d, CEILING, max_steps=max_steps)
    assert (ref["index"][outside, 0] < 0).all() and (ref["n_steps"][outside] == 0).all()
    assert (ref["n_steps"] <= max_steps).all()
    with st.view() as v:
        loop = DL.traverse(v, math, pos, d, CEILING, max_steps, st.media)
    for key in ("position", "index", "length", "n_steps", "n_crossings"):
        same_bytes(loop[key], ref[key], f"Stepping loop, {key}")
    for n in SIZES:
        got = st.traverse(pos[:n].copy(), d[:n], CEILING, max_steps=max_steps)
        for key in ("position", "index", "n_steps", "n_crossings"):
            same_bytes(got[key], ref[key][:n], f"{n} rays, {key}")
        same_bytes(got["length"], ref["length"][:, :n], f"{n} rays, length")


@pytest.mark.parametrize("n_steps", [0, 1, 7])
def test_scatter_of_the_first_rays_is_the_whole_batch(stack2x2, rays, math, n_steps):
    st = stack2x2
    pos, _, outside = rays
    ref = st.scatter(pos.copy(), 4242, n_steps, first_ray=17)
    assert (ref["index"][outside, 0] < 0).all() and (ref["steps"][outside] == 0).all()
    assert (ref["steps"][~outside] == n_steps).sum() > N // 2
    for n in SIZES:
        got = st.scatter(pos[:n].copy(), 4242, n_steps, first_ray=17)
        for key in ("position", "altitude", "elevation", "index", "length", "steps"):
            same_bytes(got[key], ref[key][:n], f"{n} rays, {key}")
