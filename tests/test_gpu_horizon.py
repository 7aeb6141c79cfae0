"""turtle_stepper_horizon_n on the GPU: the skyline around observers, against the call's definition
evaluated over the compiled reference (tests/golden/horizon.npz, made by
tests/golden/generate_horizon.py), against the composition of the batch calls that gave a skyline
before it existed, and on the edges of its wave-per-line reduction.

The bar.  The kernel evaluates the definition's expressions in its operand order in IEEE doubles;
what can differ from the fixture is the last ulp of OCML's functions against glibc's (and, in FAST
arithmetic, of the fast transform against the closed form), carried through latitude and longitude
into the ground under a sample.  That cannot be derived, so it is measured: WORST_* are the largest
differences seen on the MI355X over every case of the fixture, per arithmetic; the bars are ten
times those, to leave room for another libm build.  As a condition and not a measurement the sine's
bar may not exceed 1e-9: one ulp of latitude moves the ground by under 1e-9 m, so a larger
difference is a bug.  Every best-to-second gap of the fixture is above 1e-8
(tests/test_horizon_host.py), so the sample number is pinned on every line."""
import subprocess

import numpy as np
import pytest

import turtle_amd as TA
from turtle_amd import synth

import horizon_cases as HC
import normal_cases as NC
import sight_cases as SC
from sight_cases import flat, geometries, math_mode  # noqa: F401 (the fixtures, for pytest to find)

pytestmark = pytest.mark.gpu

# measured on the MI355X, the largest |sin(elevation) - expected| and |range - expected| (metres) of
# each case, FAST / STRICT:  map 2.1e-16 / 3.5e-18 and 3.3e-11 / 3.6e-12;  stack 1.7e-13 / 1.4e-17 and
# 1.6e-10 / 0;  layers_geoid 1.8e-13 / 8.8e-14 and 2.3e-10 / 1.2e-10;  lambert 5.56e-12 and 1.97e-9 in
# both (the projected map sets all four: the last ulp of the projection's functions on x, y of
# 10^6 m, as in test_gpu_normal.py)
WORST_SINE = {"fast": 5.56e-12, "strict": 5.56e-12}
WORST_RANGE = {"fast": 1.973e-9, "strict": 1.973e-9}
BAR_SINE = {m: 10 * w for m, w in WORST_SINE.items()}
BAR_RANGE = {m: 10 * w for m, w in WORST_RANGE.items()}
CAP_SINE = 1e-9
SENTINEL = HC.SENTINEL


def test_the_bar_is_below_its_cap():
    assert max(BAR_SINE.values()) <= CAP_SINE


def run(st, position, azimuth, distance, layer, want=("range",)):
    """the call over sentinels: dict(elevation, sample[, range])"""
    shape = (np.asarray(position).reshape(-1, 3).shape[0], len(azimuth))
    out = dict(elevation=np.full(shape, SENTINEL))
    if "range" in want:
        out["range"] = np.full(shape, SENTINEL)
    return st.horizon(position, azimuth, distance, layer, out=out, want=want)


def check_against(sine, got, bar_sine, bar_range, label, want_range=None):
    """`got` against a profile of sines [n][n_az][n_d] (NaN: skipped): the sample where the
    profile's gap pins it, else one within the bar of the maximum; sin(elevation); the sentinels.
    Returns the worst sine difference."""
    filled = np.where(np.isnan(sine), -np.inf, sine)
    best = filled.max(-1)
    want = np.where(np.isinf(best), 0, filled.argmax(-1) + 1)
    sample, elevation = got["sample"], got["elevation"]
    none = want == 0
    assert np.array_equal(sample == 0, none), label
    assert np.array_equal(elevation[none], np.full(int(none.sum()), SENTINEL)), label       # untouched, to the bit
    if "range" in got:
        assert np.array_equal(got["range"][none], np.full(int(none.sum()), SENTINEL)), label
    if none.all():
        return 0.0
    pinned = ~none & (HC.gaps(sine) > bar_sine)
    assert np.array_equal(sample[pinned], want[pinned]), (label, sample[pinned], want[pinned])
    at = np.take_along_axis(filled, np.maximum(sample - 1, 0)[..., None], -1)[..., 0]
    assert (best[~none] - at[~none] <= bar_sine).all(), label                               # (-inf: a skipped one)
    worst = np.abs(np.sin(np.radians(elevation[~none])) - best[~none]).max()
    line = f"{label}: {int((~none).sum())} lines, worst sine difference {worst:.3e}"
    worst_range = 0.0
    if want_range is not None:
        same = ~none & (sample == want)
        worst_range = np.abs(got["range"][same] - want_range[same]).max()
        line += f", worst range difference {worst_range:.3e} m"
    print(line)
    assert worst <= bar_sine, (label, worst)
    assert worst_range <= bar_range, (label, worst_range)
    return worst


# ---- 1, 2: against the reference ---------------------------------------------------------------

@pytest.mark.parametrize("math", ["fast", "strict"])
@pytest.mark.parametrize("case", HC.CASES)
def test_against_the_reference(golden, geometries, case, math):
    g = golden("horizon")
    st = geometries(case)["stepper"]
    with math_mode(math):
        got = run(st, g[case + "_position"], g[case + "_azimuth"], g[case + "_distance"], int(g[case + "_layer"]))
    assert st.rounds == 1
    assert (HC.gaps(g[case + "_sine"]) > CAP_SINE).all()       # the sample number is pinned on every line
    check_against(g[case + "_sine"], got, BAR_SINE[math], BAR_RANGE[math], f"{case} {math}", g[case + "_range"])
    assert np.array_equal(got["sample"], g[case + "_sample"])


# ---- 3: ties -----------------------------------------------------------------------------------

def test_ties_go_to_the_smaller_k(flat):
    """over a flat layer seen from 800 m up the sine -h / s - s / 2R rises with the distance up to
    sqrt(2 R h) = 101 km: below that the farther of two samples wins, and equal distances tie"""
    st, pos = flat
    near, far = run(st, pos, [0.0, 90.0], [20e3, 20e3, 10e3, 10e3], 0), run(st, pos, [0.0, 90.0], [10e3, 10e3, 20e3, 20e3], 0)
    assert (near["sample"] == 1).all() and (far["sample"] == 3).all()      # neighbouring lanes
    assert np.array_equal(near["elevation"], far["elevation"]) and np.array_equal(near["range"], far["range"])
    distance = np.linspace(1e3, 50e3, 130)
    for pair, winner in (((3, 67), 4),         # one lane's first and second turn
                         ((4, 67), 5),         # the lower lane (3) holds the larger k
                         ((66, 67), 67),       # neighbouring lanes, both on their second turn
                         ((1, 129), 2)):       # a third turn, which only lanes 0 and 1 take
        tied = distance.copy()
        tied[list(pair)] = 60e3
        assert (run(st, pos, [0.0, 90.0], tied, 0)["sample"] == winner).all(), pair
    distance[:] = 60e3                                                     # every sample ties
    assert (run(st, pos, [0.0, 90.0], distance, 0)["sample"] == 1).all()
    distance[5] = np.nan                                                   # a NaN never wins, nor hides a winner
    distance[0] = np.nan
    assert (run(st, pos, [0.0, 90.0], distance, 0)["sample"] == 2).all()
    only_nan = run(st, pos, [0.0, 90.0], [np.nan, np.nan], 0)
    assert (only_nan["sample"] == 0).all() and (only_nan["elevation"] == SENTINEL).all()


# ---- 4: shapes ---------------------------------------------------------------------------------

@pytest.mark.parametrize("n_d", [1, 63, 64, 65])
def test_prefixes_of_the_distances(golden, geometries, n_d):
    g = golden("horizon")
    for case in ("map", "layers_geoid"):
        st = geometries(case)["stepper"]
        got = run(st, g[case + "_position"], g[case + "_azimuth"], g[case + "_distance"][:n_d], int(g[case + "_layer"]))
        check_against(g[case + "_sine"][:, :, :n_d], got, BAR_SINE["fast"], BAR_RANGE["fast"], f"{case} n_d={n_d}")
        if n_d == 1:       # the sample at the foot alone: skipped from height 0, straight down from above
            assert got["sample"].tolist() == [[0] * 5] + [[1] * 5] * 3
            # (the fixture's sine there is within 1e-12 of -1: asin moves by sqrt(2e-12) rad = 8.1e-5 degrees)
            assert np.abs(got["elevation"][1:] + 90.0).max() < 2e-4


def test_items_that_do_not_fill_a_block_and_one_item_alone(golden, geometries):
    g = golden("horizon")
    st = geometries("stack")["stepper"]
    pos, az, dist = g["stack_position"], g["stack_azimuth"], g["stack_distance"]
    full = run(st, pos, az, dist, 0)
    for rows, cols in ((slice(2, 3), slice(3, 4)), (slice(1, 2), slice(1, 4)), (slice(0, 3), slice(4, 5)),
                       (slice(3, 4), slice(0, 5))):                         # 1, 3, 3 and 5 items
        part = run(st, pos[rows], az[cols], dist, 0)
        for name in ("elevation", "sample", "range"):
            assert np.array_equal(part[name], full[name][rows, cols]), (rows, cols, name)


# ---- 5: no data --------------------------------------------------------------------------------

def test_an_observer_off_the_data_keeps_its_outputs(golden, geometries):
    g = golden("horizon")
    st = geometries("map")["stepper"]
    away = TA.ecef_from_geodetic(np.array([5.0]), np.array([5.0]), np.array([1500.0]))     # 4 degrees off the map
    pos = np.concatenate([g["map_position"][:2], away, g["map_position"][2:]])
    az, dist = g["map_azimuth"], g["map_distance"]
    got = run(st, pos, az, dist, 0)
    assert (got["sample"][2] == 0).all() and (got["elevation"][2] == SENTINEL).all() and (got["range"][2] == SENTINEL).all()
    keep = [0, 1, 3, 4]
    assert np.array_equal(got["sample"][keep], g["map_sample"])
    bare = run(st, pos, az, dist, 0, want=())
    assert "range" not in bare
    assert np.array_equal(bare["elevation"], got["elevation"]) and np.array_equal(bare["sample"], got["sample"])


# ---- 6: spaces ---------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["stack", "layers_geoid"])
def test_spaces_give_the_same_bits_and_the_stream_is_honoured(golden, geometries, case):
    import torch
    g = golden("horizon")
    st = geometries(case)["stepper"]
    pos, az, dist, layer = g[case + "_position"], g[case + "_azimuth"], g[case + "_distance"], int(g[case + "_layer"])
    host = run(st, pos, az, dist, layer)
    stream = torch.cuda.Stream()
    try:
        with torch.cuda.stream(stream):
            TA.set_stream(stream)
            # inputs made, and outputs read, by work queued on the same stream around the call
            d_pos = torch.zeros(pos.shape, dtype=torch.float64, device="cuda")
            d_pos += torch.as_tensor(pos).pin_memory().to("cuda", non_blocking=True)
            out = dict(elevation=torch.full(host["elevation"].shape, SENTINEL, dtype=torch.float64, device="cuda"),
                       range=torch.full(host["range"].shape, SENTINEL, dtype=torch.float64, device="cuda"))
            dev = st.horizon(d_pos, torch.as_tensor(az, device="cuda"), torch.as_tensor(dist, device="cuda"),
                             layer, out=out)
            back = {k: v.clone() for k, v in dev.items()}
        stream.synchronize()
    finally:
        TA.set_stream(None)
    assert dev["elevation"] is out["elevation"] and dev["sample"].is_cuda
    for name in ("elevation", "sample", "range"):
        assert np.array_equal(back[name].cpu().numpy(), host[name]), name


# ---- 7: residency ------------------------------------------------------------------------------

def test_the_call_loads_the_tiles_it_needs(golden, tmp_path):
    g = golden("horizon")
    geo = NC.amd_geometry("stack", str(tmp_path), 0)           # stack_size 0: no limit; nothing loaded yet
    try:
        stack = geo["layers"][0][0][1]
        assert stack.resident == 0
        got = run(geo["stepper"], g["stack_position"], g["stack_azimuth"], g["stack_distance"], 0)
        assert stack.resident == 3 and geo["stepper"].rounds == 1
        assert np.array_equal(got["sample"], g["stack_sample"])
    finally:
        NC.destroy(geo)


def test_a_stack_too_small_for_its_tiles_is_refused(golden, tmp_path):
    g = golden("horizon")
    geo = NC.amd_geometry("stack", str(tmp_path), 1)           # three tiles, room for one
    try:
        stack = geo["layers"][0][0][1]
        before = stack.resident
        shape = g["stack_sample"].shape
        out = dict(elevation=np.full(shape, SENTINEL), range=np.full(shape, SENTINEL))
        with pytest.raises(TA.TurtleError) as err:
            geo["stepper"].horizon(g["stack_position"], g["stack_azimuth"], g["stack_distance"], 0, out=out)
        assert err.value.name == "DOMAIN_ERROR" and "turtle_stepper_horizon_n" in str(err.value)
        assert "a device view" not in str(err.value) and "stack_size 1" in str(err.value)
        assert (out["elevation"] == SENTINEL).all() and (out["range"] == SENTINEL).all()
        assert stack.resident == before
    finally:
        NC.destroy(geo)


# ---- 8: against the composition of the calls that existed before ----------------------------------

def test_against_the_composition_of_the_older_calls(tmp_path):
    """a geometry larger than the fixture's: one rough tile of 1201 x 1201 nodes, 16 observers x 36
    azimuths x 200 distances, the whole profile from turtle_ecef_to_geodetic_n (STRICT),
    turtle_ecef_from_horizontal_n, turtle_stepper_position_n and numpy"""
    with SC.rough_lines(str(tmp_path)) as r:
        st, pos, az, dist = (r[k] for k in ("stepper", "position", "azimuth", "distance"))
        with math_mode("strict"):
            got = run(st, pos, az, dist, 0)
        sine, _ = SC.composed_profile(st, pos, az, dist)
        assert np.isnan(sine).any() and not np.isnan(sine).all(-1).any()           # lines leave the tile
        want = np.nanargmax(sine, -1) + 1
        print("composition: winners on", len(set(want.ravel().tolist())), "different samples,",
              int((got["sample"] != want).sum()), "lines differ in the sample")
        check_against(sine, got, BAR_SINE["strict"], BAR_RANGE["strict"], "composition")


# ---- the example -------------------------------------------------------------------------------

def test_horizon_example(tmp_path):
    exe = SC.build_example("horizon", tmp_path)
    tile = synth.write_rough_hgt(str(tmp_path), 45, 3)
    out = subprocess.run([exe, tile], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    lat0, lon0 = (float(v) for v in lines[0].split()[1:3])
    rows = [l.split() for l in lines if l.startswith("azimuth")]
    assert len(rows) == 360 and all(r[3] != "none" for r in rows) and lines[-1].startswith("360 azimuths, open sky")
    # the same profile through the binding
    m = TA.Map.load(tile)
    st = TA.Stepper()
    st.add_map(m, 0.0)
    try:
        pos, _ = st.position(np.array([lat0]), np.array([lon0]), 2.0)
        dist = np.array([30.0 * (1e5 / 30.0) ** (k / 255.0) for k in range(256)])
        got = st.horizon(pos, np.arange(360.0), dist, 0)
        same = np.array([abs(float(r[5]) - dist[k - 1]) < 2e-3 for r, k in zip(rows, got["sample"][0])])
        print("example:", int(same.sum()), "of 360 lines on the binding's sample")
        assert same.all()          # (the C library's pow() against Python's moves a distance by an ulp, no winner)
        assert np.abs(np.array([float(r[3]) for r in rows]) - got["elevation"][0])[same].max() < 1e-4
        assert np.abs(np.array([float(r[8]) for r in rows]) - got["range"][0])[same].max() < 2e-3
    finally:
        st.destroy()
        m.destroy()
