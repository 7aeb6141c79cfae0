"""What the GPU tests of the calls over lines of sight share (test_gpu_horizon.py,
test_gpu_viewshed.py; test_gpu_normal.py takes `geometries`): the fixtures, imported into the test
modules by name, the rough-tile inputs, the profile of sines composed from the older batch calls,
and the build of an example."""
import contextlib
import os
import subprocess

import numpy as np
import pytest

import turtle_amd as TA
from turtle_amd import synth

import horizon_cases as HC
import normal_cases as NC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def geometries(tmp_path_factory):
    made = {}

    def get(case, stack_size=0):
        key = (case, stack_size)
        if key not in made:
            made[key] = NC.amd_geometry(case, str(tmp_path_factory.mktemp(f"{case}_{stack_size}")), stack_size)
        return made[key]

    yield get
    for geo in made.values():
        NC.destroy(geo)


class math_mode:
    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        TA.set_math(self.mode)

    def __exit__(self, *exc):
        TA.set_math("fast")
        return False


@pytest.fixture(scope="module")
def flat():
    st = TA.Stepper()
    st.add_flat(0.0)
    pos, _ = st.position(np.array([12.0]), np.array([34.0]), 800.0)
    yield st, pos
    st.destroy()


@contextlib.contextmanager
def rough_lines(directory):
    """a geometry larger than the fixtures': one rough tile of 1201 x 1201 nodes, 16 observers x 36
    azimuths x 200 distances -> dict(stepper, position, azimuth, distance)"""
    synth.write_rough_hgt(directory, 45, 3)
    stack = TA.Stack(directory, 0)
    st = TA.Stepper()
    st.add_stack(stack, 0.0)
    rng = np.random.Generator(np.random.Philox(81))
    n, n_az, n_d = 16, 36, 200
    try:
        with math_mode("strict"):
            pos, di = st.position(rng.uniform(45.2, 45.8, n), rng.uniform(3.2, 3.8, n), rng.uniform(2.0, 300.0, n))
        assert (di == 0).all()
        az = np.arange(n_az) * 10.0
        dist = 100.0 * 600.0 ** (np.arange(n_d) / (n_d - 1.0))                  # 100 m to 60 km
        yield dict(stepper=st, position=pos, azimuth=az, distance=dist)
    finally:
        st.destroy()
        stack.destroy()


def composed_profile(st, pos, az, dist):
    """the whole profile of sines [n][n_az][n_d] over layer 0 from turtle_ecef_to_geodetic_n (STRICT),
    turtle_ecef_from_horizontal_n, turtle_stepper_position_n and numpy -> (sine, skipped), the sine
    NaN where the definition skips the sample"""
    n, n_az, n_d = pos.shape[0], len(az), len(dist)
    with math_mode("strict"):
        la0, lo0, _ = TA.ecef_to_geodetic(pos)
        h = TA.ecef_from_horizontal(np.repeat(la0, n_az), np.repeat(lo0, n_az), np.tile(az, n),
                                    np.zeros(n * n_az)).reshape(n, n_az, 1, 3)
        p = pos.reshape(n, 1, 1, 3)
        s = dist.reshape(1, 1, n_d)
        q = np.stack([p[..., j] + s * h[..., j] for j in range(3)], -1)
        la, lo, _ = TA.ecef_to_geodetic(q.reshape(-1, 3))
        ground, di = st.position(la, lo, 0.0, 0)
    lam, phi = lo0 * np.pi / 180.0, la0 * np.pi / 180.0
    sl, cl, sp, cp = np.sin(lam), np.cos(lam), np.sin(phi), np.cos(phi)
    up = np.stack([cl * cp, sl * cp, sp], -1).reshape(n, 1, 1, 3)
    d = ground.reshape(n, n_az, n_d, 3) - p
    rr = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
    with np.errstate(invalid="ignore", divide="ignore"):
        sine = (up[..., 0] * d[..., 0] + up[..., 1] * d[..., 1] + up[..., 2] * d[..., 2]) / np.sqrt(rr)
    skipped = (di.reshape(n, n_az, n_d) < 0) | (rr <= HC.FLT_EPSILON)
    sine[skipped] = np.nan
    return sine, skipped


def build_example(name, tmp_path):
    """examples/<name>.c compiled against the library in use -> the program's path"""
    exe = str(tmp_path / name)
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", name + ".c"), "-o", exe,
                           "-L" + os.path.dirname(TA.library_path()), "-lturtle_amd",
                           "-Wl,-rpath," + os.path.dirname(TA.library_path()), "-lm"])
    return exe
