"""turtle_stepper_viewshed_n on the GPU: what observers see along each azimuth, against the call's
definition evaluated over the compiled reference (tests/golden/viewshed.npz, made by
tests/golden/generate_viewshed.py), against its own samples (the wave's scan is exact), against
the calls that existed before it, and on the edges of its chunks of 64 samples.

The bars.  At target height 0 the sines are turtle_stepper_horizon_n's expressions, and the bar is
that test's BAR_SINE (tests/test_gpu_horizon.py: ten times the worst seen there, 5.56e-12), taken
from the project.  The sine of a target ABOVE the ground is a new quantity; it cannot be derived
either (the last ulp of OCML's functions against glibc's, carried through latitude and longitude
into the ground under a sample), so it is measured: WORST_TARGET holds the largest |sine - fixture|
seen on the MI355X over every case at the mast's height, per arithmetic, and the bar is ten times
that, room for another libm build.  As a condition and not a measurement no bar may exceed 1e-9
(CAP_SINE's reasoning: one ulp of latitude moves the ground by under 1e-9 m).  Every
|sine - horizon| of the fixture is above 1e-8 (tests/test_viewshed_host.py), so every flag of it is
pinned and `visible` and `n_visible` are compared on every element.

Measured on the MI355X, the largest |sine - fixture| over EVERY sample with data (the horizon test
measures its 20 winners a case), FAST / STRICT:
  height 0:   map 1.27e-14 / 1.18e-14, stack 1.63e-12 / 1.63e-12, lambert 1.43e-11 / 1.85e-11,
              layers_geoid 1.83e-12 / 1.83e-12: all under the project's bar of 5.56e-11;
  height 10:  map 1.18e-14 / 1.18e-14, stack 1.61e-12 / 1.61e-12, lambert 1.54e-11 / 1.85e-11,
              layers_geoid 1.83e-12 / 1.83e-12: WORST_TARGET.
|horizon - fixture| is at most 1.43e-11 / 1.09e-11 (lambert).  No flag differs in any case.

The longitude of a sample is the closed form's atan2 in FAST as well (sight.hip, d_sight_sample's
CLOSED_LON).  Observer 0 of layers_geoid stands at longitude 11 exactly and azimuth 0 runs
due north, along the seam between the stack's tile 10..11 degrees east and the MISSING tile north
of latitude 1: the reference's transform returns 11 - 1 ulp there, the tile with data, and at 11.0
its own turtle_stepper_position finds none.  With the fast transform's own atan2 five samples of
that line (116 to 119 and 123) came back -1 where the fixture has data; test_against_the_fixture
[layers_geoid-*-fast] is what holds the kernel to the reference's side of a seam.
"""
import itertools
import subprocess

import numpy as np
import pytest

import turtle_amd as TA
from turtle_amd import synth

import horizon_cases as HC
import normal_cases as NC
import sight_cases as SC
import viewshed_cases as VC
from sight_cases import flat, geometries, math_mode  # noqa: F401 (the fixtures, for pytest to find)

pytestmark = pytest.mark.gpu

CAP_SINE = 1e-9
# tests/test_gpu_horizon.py: WORST_SINE, BAR_SINE (the ground's sines: the same expressions)
WORST_GROUND = {"fast": 5.56e-12, "strict": 5.56e-12}
# the target 10 m above the ground; MEASURED on the MI355X (see the header): the Lambert map sets both
WORST_TARGET = {"fast": 1.538e-11, "strict": 1.849e-11}
BAR_GROUND = {m: 10 * w for m, w in WORST_GROUND.items()}
BAR_TARGET = {m: 10 * w for m, w in WORST_TARGET.items()}
ALL = ("sine", "horizon", "n_visible")


def test_the_bars_are_below_their_cap():
    assert max(BAR_GROUND.values()) <= CAP_SINE and max(BAR_TARGET.values()) <= CAP_SINE


def inputs(golden, case):
    g = golden("horizon")
    return g[case + "_position"], g[case + "_azimuth"], g[case + "_distance"], int(g[case + "_layer"])


def same_bits(a, b, label):
    assert set(a) == set(b), label
    for name in a:
        x, y = np.asarray(a[name]), np.asarray(b[name])
        assert x.dtype == y.dtype and x.shape == y.shape, (label, name)
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8)), (label, name)      # (NaNs: their bits too)


def own_consistency(got, label):
    """the scan against the call's own samples, exact (target height 0: sine is the ground's)"""
    sine, horizon, visible = got["sine"], got["horizon"], got["visible"]
    assert np.array_equal(np.isnan(sine) & (visible != 0), visible == -1), label
    want = VC.running_maximum(sine)
    assert np.array_equal(horizon.view(np.uint64), want.view(np.uint64)), label       # bit for bit
    with np.errstate(invalid="ignore"):
        assert np.array_equal(visible[visible >= 0] == 1, (sine >= horizon)[visible >= 0]), label
    assert np.array_equal(got["n_visible"], (visible == 1).sum(-1)), label


# ---- 1: against the fixture ----------------------------------------------------------------------

@pytest.mark.parametrize("math", ["fast", "strict"])
@pytest.mark.parametrize("height", VC.TARGET_HEIGHTS)
@pytest.mark.parametrize("case", VC.CASES)
def test_against_the_fixture(golden, geometries, case, height, math):
    g = golden("viewshed")
    pos, az, dist, layer = inputs(golden, case)
    st = geometries(case)["stepper"]
    with math_mode(math):
        got = st.viewshed(pos, az, dist, layer, target_height=height)
    assert st.rounds == 1
    key = f"{case}_{VC.tag(height)}"
    want = {name: g[f"{key}_{name}"] for name in VC.OUTPUTS}
    assert got["visible"].dtype == np.int8 and got["n_visible"].dtype == np.int32
    # every figure first, over the samples that have a number on both sides; then the assertions
    other = np.argwhere(np.isnan(got["sine"]) != np.isnan(want["sine"]))
    with np.errstate(invalid="ignore"):
        worst_sine = np.nanmax(np.abs(got["sine"] - want["sine"]))
        both = np.isfinite(got["horizon"]) & np.isfinite(want["horizon"])
        worst_horizon = np.abs(got["horizon"][both] - want["horizon"][both]).max()
    wrong = np.argwhere(got["visible"] != want["visible"])
    print(f"MEASURED {key} {math}: worst sine difference {worst_sine:.3e}, horizon {worst_horizon:.3e}, "
          f"{len(wrong)} of {want['visible'].size} flags differ {wrong.tolist()}, {len(other)} samples have data "
          f"on one side only {other.tolist()}")
    # where a number stands, and where NaN / -inf: exactly
    assert np.array_equal(np.isnan(got["sine"]), np.isnan(want["sine"]))
    assert np.array_equal(np.isneginf(got["horizon"]), np.isneginf(want["horizon"]))
    assert not np.isnan(got["horizon"]).any() and not np.isposinf(got["horizon"]).any()
    assert np.array_equal(got["visible"], want["visible"])                 # every element, no exclusions
    assert np.array_equal(got["n_visible"], want["n_visible"])
    assert worst_sine <= (BAR_GROUND if height == 0.0 else BAR_TARGET)[math], (key, worst_sine)
    assert worst_horizon <= BAR_GROUND[math], (key, worst_horizon)         # (the ground's, at either height)


# ---- 2: the scan against the call's own samples ----------------------------------------------------

@pytest.mark.parametrize("case", VC.CASES)
def test_the_scan_is_exact_on_the_fixture_cases(golden, geometries, case):
    pos, az, dist, layer = inputs(golden, case)
    for math in ("fast", "strict"):
        with math_mode(math):
            own_consistency(geometries(case)["stepper"].viewshed(pos, az, dist, layer), f"{case} {math}")


@pytest.fixture(scope="module")
def rough(tmp_path_factory):
    """one rough tile of 1201 x 1201 nodes, 16 observers x 36 azimuths x 200 distances: the inputs of
    test_gpu_horizon.py's composition test, and the call's answer over them (STRICT)"""
    with SC.rough_lines(str(tmp_path_factory.mktemp("rough"))) as r:
        with math_mode("strict"):
            r["got"] = r["stepper"].viewshed(r["position"], r["azimuth"], r["distance"], 0)
        yield r


def test_the_scan_is_exact_on_a_rough_tile(rough):
    got = rough["got"]
    assert got["visible"].shape == (16, 36, 200)
    assert (got["visible"] == -1).any() and (got["visible"] == 0).any() and (got["visible"] == 1).any()
    own_consistency(got, "rough")


# ---- 3: the carry across chunks, and the wave and block remainders -----------------------------------

@pytest.mark.parametrize("m", [1, 63, 64, 65, 128, 129])
def test_prefixes_of_the_distances(golden, geometries, m):
    for case, height in (("map", 0.0), ("layers_geoid", 10.0)):
        pos, az, dist, layer = inputs(golden, case)
        st = geometries(case)["stepper"]
        full = st.viewshed(pos, az, dist, layer, target_height=height)
        part = st.viewshed(pos, az, dist[:m], layer, target_height=height)
        want = {name: np.ascontiguousarray(full[name][:, :, :m]) for name in ("visible", "sine", "horizon")}
        want["n_visible"] = (want["visible"] == 1).sum(-1).astype(np.int32)
        same_bits(part, want, f"{case} m={m}")


def test_items_that_do_not_fill_a_block_and_one_item_alone(golden, geometries):
    pos, az, dist, _ = inputs(golden, "stack")
    st = geometries("stack")["stepper"]
    full = st.viewshed(pos, az, dist, 0, target_height=10.0)
    for rows, cols in ((slice(2, 3), slice(3, 4)), (slice(1, 2), slice(1, 4)), (slice(0, 3), slice(4, 5)),
                       (slice(3, 4), slice(0, 5))):                         # 1, 3, 3 and 5 items
        part = st.viewshed(pos[rows], az[cols], dist, 0, target_height=10.0)
        same_bits(part, {name: np.ascontiguousarray(value[rows, cols]) for name, value in full.items()}, (rows, cols))


# ---- 4: edges ------------------------------------------------------------------------------------

def test_repeated_distances_and_a_nan(flat):
    """over a flat layer seen from 800 m up the sine rises with the distance up to 101 km (see
    test_gpu_horizon.py): increasing distances below that are all visible"""
    st, pos = flat
    rising = np.linspace(1e3, 50e3, 130)
    base = st.viewshed(pos, [0.0, 90.0], rising, 0)
    assert (base["visible"] == 1).all() and (base["n_visible"] == 130).all()
    own_consistency(base, "flat")
    # equal distances give equal sines: all seen, by >=, and the horizon is raised once
    tied = rising.copy()
    tied[60:70] = rising[60]                                               # across the chunks' border
    got = st.viewshed(pos, [0.0, 90.0], tied, 0)
    assert (got["visible"] == 1).all() and (got["n_visible"] == 130).all()
    assert (got["sine"][:, :, 60:70] == got["sine"][:, :, 60:61]).all()
    assert (got["horizon"][:, :, 61:71] == got["sine"][:, :, 60:61]).all()
    own_consistency(got, "ties")
    every = st.viewshed(pos, [0.0, 90.0], np.full(130, 60e3), 0)
    assert (every["visible"] == 1).all() and (every["horizon"][:, :, 1:] == every["sine"][:, :, :1]).all()
    # a NaN distance: a sample with data, never visible, raising nothing; its neighbours keep their bits
    holed = rising.copy()
    holed[[0, 5, 63, 64, 129]] = np.nan
    got = st.viewshed(pos, [0.0, 90.0], holed, 0)
    at = np.isnan(holed)
    assert (got["visible"][:, :, at] == 0).all() and np.isnan(got["sine"][:, :, at]).all()
    assert np.isneginf(got["horizon"][:, :, :2]).all()                      # (the NaN in front raised nothing)
    assert np.array_equal(got["visible"][:, :, ~at], base["visible"][:, :, ~at])
    assert np.array_equal(got["sine"][:, :, ~at].view(np.uint64), base["sine"][:, :, ~at].view(np.uint64))
    assert (got["n_visible"] == 125).all()
    own_consistency(got, "nan")
    falling = st.viewshed(pos, [0.0], rising[::-1].copy(), 0)              # swept inwards: the first hides the rest
    assert falling["visible"][0, 0].tolist() == [1] + [0] * 129


def test_a_line_off_the_data_and_the_foot_of_the_observer(golden, geometries):
    pos, az, dist, _ = inputs(golden, "map")
    st = geometries("map")["stepper"]
    away = TA.ecef_from_geodetic(np.array([5.0]), np.array([5.0]), np.array([1500.0]))     # 4 degrees off the map
    got = st.viewshed(np.concatenate([pos[:2], away, pos[2:]]), az, dist, 0)
    assert (got["visible"][2] == -1).all() and (got["n_visible"][2] == 0).all()
    assert np.isneginf(got["horizon"][2]).all() and np.isnan(got["sine"][2]).all()
    keep = [0, 1, 3, 4]
    same_bits({k: np.ascontiguousarray(v[keep]) for k, v in got.items()}, st.viewshed(pos, az, dist, 0), "beside it")
    # the observer at height 0: the sample at its own foot is skipped; from 2 m up it is seen, straight down
    assert (got["visible"][0, :, 0] == -1).all() and np.isnan(got["sine"][0, :, 0]).all()
    assert (got["visible"][1, :, 0] == 1).all() and np.abs(got["sine"][1, :, 0] + 1.0).max() < 1e-12


def test_every_subset_of_the_optional_outputs(golden, geometries):
    pos, az, dist, layer = inputs(golden, "layers_geoid")
    st = geometries("layers_geoid")["stepper"]
    full = st.viewshed(pos, az, dist, layer, target_height=10.0)
    assert set(full) == {"visible"} | set(ALL)
    for size in range(len(ALL)):
        for want in itertools.combinations(ALL, size):
            part = st.viewshed(pos, az, dist, layer, target_height=10.0, want=want)
            same_bits(part, {name: full[name] for name in ("visible",) + want}, want)


# ---- 5: against the older calls --------------------------------------------------------------------

def test_against_the_composition_of_the_older_calls(rough):
    """the whole profile from turtle_ecef_to_geodetic_n (STRICT), turtle_ecef_from_horizontal_n,
    turtle_stepper_position_n and numpy, as in test_gpu_horizon.py.  The flags are compared wherever
    |sine - running maximum| exceeds the bar; as a condition at most 1e-3 of the samples with data
    may be left out.  (On the CPU, with the definition restated over the compiled reference on
    these inputs: 109 825 samples with data, 19 158 of them visible, the smallest
    |sine - running maximum| 3.1e-7, none within 1e-9: nothing is expected to be left out.)"""
    st, pos, az, dist, got = (rough[k] for k in ("stepper", "position", "azimuth", "distance", "got"))
    sine, skipped = SC.composed_profile(st, pos, az, dist)
    horizon = VC.running_maximum(sine)
    visible, _ = VC.follows(sine, horizon, skipped)
    bar = BAR_GROUND["strict"]
    assert np.array_equal(got["visible"] == -1, skipped)
    with np.errstate(invalid="ignore"):
        pinned = ~skipped & ~(np.abs(sine - horizon) <= bar)               # (an infinite horizon pins)
    left_out = 1.0 - pinned.sum() / (~skipped).sum()
    worst = np.abs(got["sine"][~skipped] - sine[~skipped]).max()
    print(f"composition: {int((~skipped).sum())} samples with data, {int((visible == 1).sum())} visible, "
          f"{int((~skipped).sum() - pinned.sum())} left out, worst sine difference {worst:.3e}")
    assert left_out <= 1e-3
    assert np.array_equal(got["visible"][pinned], visible[pinned])
    assert worst <= bar
    finite = np.isfinite(horizon)
    assert np.array_equal(np.isfinite(got["horizon"]), finite)
    assert np.abs(got["horizon"][finite] - horizon[finite]).max() <= bar


# ---- 6: against turtle_stepper_horizon_n -------------------------------------------------------------

def test_agreement_with_horizon_n(rough, golden, geometries):
    sets = [("rough", rough["stepper"], rough["position"], rough["azimuth"], rough["distance"], 0)]
    for case in ("stack", "layers_geoid"):
        sets.append((case, geometries(case)["stepper"]) + inputs(golden, case))
    bar = BAR_GROUND["strict"]
    with math_mode("strict"):
        for label, st, pos, az, dist, layer in sets:
            sine = st.viewshed(pos, az, dist, layer, want=("sine",))["sine"]
            sky = st.horizon(pos, az, dist, layer)
            filled = np.where(np.isnan(sine), -np.inf, sine)
            best = filled.max(-1)
            none = np.isneginf(best)
            assert np.array_equal(sky["sample"] == 0, none), label
            pinned = ~none & (HC.gaps(sine) > bar)
            assert pinned.sum() >= 0.99 * (~none).sum(), label
            assert np.array_equal(sky["sample"][pinned], (filled.argmax(-1) + 1)[pinned]), label
            assert np.abs(np.sin(np.radians(sky["elevation"][~none])) - best[~none]).max() <= bar, label


# ---- 7: spaces and residency -----------------------------------------------------------------------

@pytest.mark.parametrize("case", ["stack", "layers_geoid"])
def test_spaces_give_the_same_bits_and_the_stream_is_honoured(golden, geometries, case):
    import torch
    pos, az, dist, layer = inputs(golden, case)
    st = geometries(case)["stepper"]
    host = st.viewshed(pos, az, dist, layer, target_height=10.0)
    stream = torch.cuda.Stream()
    try:
        with torch.cuda.stream(stream):
            TA.set_stream(stream)
            # inputs made, and outputs read, by work queued on the same stream around the call
            d_pos = torch.zeros(pos.shape, dtype=torch.float64, device="cuda")
            d_pos += torch.as_tensor(pos).pin_memory().to("cuda", non_blocking=True)
            dev = st.viewshed(d_pos, torch.as_tensor(az, device="cuda"), torch.as_tensor(dist, device="cuda"),
                              layer, target_height=10.0)
            back = {k: v.clone() for k, v in dev.items()}
        stream.synchronize()
    finally:
        TA.set_stream(None)
    assert dev["visible"].is_cuda and dev["visible"].dtype == torch.int8 and dev["n_visible"].dtype == torch.int32
    same_bits({k: v.cpu().numpy() for k, v in back.items()}, host, case)


def test_the_call_loads_the_tiles_it_needs(golden, tmp_path):
    g = golden("viewshed")
    pos, az, dist, _ = inputs(golden, "stack")
    geo = NC.amd_geometry("stack", str(tmp_path), 0)           # stack_size 0: no limit; nothing loaded yet
    try:
        stack = geo["layers"][0][0][1]
        assert stack.resident == 0
        got = geo["stepper"].viewshed(pos, az, dist, 0)
        assert stack.resident == 3 and geo["stepper"].rounds == 1
        assert np.array_equal(got["visible"], g["stack_h0_visible"])
        assert np.array_equal(got["n_visible"], g["stack_h0_n_visible"])
    finally:
        NC.destroy(geo)


def test_a_stack_too_small_for_its_tiles_is_refused(golden, tmp_path):
    pos, az, dist, _ = inputs(golden, "stack")
    geo = NC.amd_geometry("stack", str(tmp_path), 1)           # three tiles, room for one
    try:
        stack = geo["layers"][0][0][1]
        before = stack.resident
        with pytest.raises(TA.TurtleError) as err:
            geo["stepper"].viewshed(pos, az, dist, 0)
        assert err.value.name == "DOMAIN_ERROR" and "turtle_stepper_viewshed_n reads resident tiles only" in str(err.value)
        assert "turtle_stepper_horizon_n" not in str(err.value) and "stack_size 1" in str(err.value)
        assert stack.resident == before
    finally:
        NC.destroy(geo)


# ---- 8: the example --------------------------------------------------------------------------------

def test_viewshed_example(tmp_path):
    exe = SC.build_example("viewshed", tmp_path)
    tile = synth.write_rough_hgt(str(tmp_path), 45, 3)
    out = subprocess.run([exe, tile], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    lat0, lon0 = (float(v) for v in lines[0].split()[1:3])
    heads = [i for i, l in enumerate(lines) if l.startswith("target ")]
    assert [lines[i] for i in heads] == ["target 0 m above the ground", "target 10 m above the ground"]
    # the same lines through the binding (the distances are whole metres: the same doubles in C and here)
    m = TA.Map.load(tile)
    st = TA.Stepper()
    st.add_map(m, 0.0)
    try:
        pos, _ = st.position(np.array([lat0]), np.array([lon0]), 2.0)
        dist = 50.0 * np.arange(1, 257)
        for at, height in zip(heads, (0.0, 10.0)):
            got = st.viewshed(pos, 45.0 * np.arange(8), dist, 0, target_height=height)
            rows = [l for l in lines[at + 1:at + 17] if l.startswith("azimuth")]
            assert len(rows) == 8
            for a, row in enumerate(rows):
                flags = "".join("#" if v > 0 else "." if v == 0 else "?" for v in got["visible"][0, a])
                assert row == "azimuth %5.1f sees %3d of 256: %s" % (45.0 * a, got["n_visible"][0, a], flags), a
            assert (got["visible"][0] == 1).any() and (got["visible"][0] == 0).any()
            first = np.flatnonzero(got["visible"][0, 0] == 1)[0]
            assert lines[at + 2].startswith("  in view: %g-" % dist[first])
    finally:
        st.destroy()
        m.destroy()
