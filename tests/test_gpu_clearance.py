"""turtle_stepper_clearance_n on the GPU: the minimum clearance of point-to-point lines, against the
call's definition evaluated over the compiled reference (tests/golden/clearance.npz, made by
tests/golden/generate_clearance.py), against the composition of the batch calls that could give it
before it existed, and on the edges of its wave-per-line reduction.

The bar.  The kernel evaluates the definition's expressions in its operand order in IEEE doubles;
what can differ from the fixture is the last ulp of OCML's functions against glibc's (and, in FAST
arithmetic, of the fast transform's latitude against the closed form's), carried through latitude
and longitude into the ground under a sample.  That cannot be derived, so it is measured: WORST is
the largest |clearance - expected| seen on the MI355X over every case of the fixture, per
arithmetic; the bar is ten times that, to leave room for another libm build.  As a condition and
not a measurement the bar may not exceed 1e-6 m: one ulp of a coordinate moves a point by under
2e-9 m and the ECEF differences round at about 1e-9 m each, so anything near a micrometre is a bug.
Every lowest-to-second gap of the fixture is above 1e-5 m (tests/test_clearance_host.py), so the
sample number is pinned on every line of it; n_data is compared exactly, which the fixture's
4-ulp condition (clearance_cases.data_is_robust) makes fair."""
import subprocess

import numpy as np
import pytest

import turtle_amd as TA
from turtle_amd import synth

import clearance_cases as CC
import normal_cases as NC
import sight_cases as SC
from sight_cases import geometries, math_mode  # noqa: F401 (the fixture, for pytest to find)

pytestmark = pytest.mark.gpu

# measured on the MI355X, the largest |clearance - expected| (metres) of each case, FAST / STRICT:
# map 4.5e-13 / 2.0e-13;  stack 9.4e-11 in both;  layers_geoid 9.1e-10 in both;  lambert 8.581e-9 /
# 3.277e-9 (the projected map sets both: the last ulp of the projection's functions on x, y of
# 10^6 m, as in test_gpu_horizon.py).  The end points over a flat layer: 7.0e-10 in both; the
# composition (STRICT, the library's own transform and position): 1.1e-13.
WORST = {"fast": 8.581e-9, "strict": 3.277e-9}
BAR = {m: 10 * w for m, w in WORST.items()}
CAP = 1e-6
SENTINEL = CC.SENTINEL


def test_the_bar_is_below_its_cap():
    assert max(BAR.values()) <= CAP


def run(st, observer, target, fraction, layer=0, paired=False, want=("n_data",)):
    """the call over sentinels: dict(clearance, sample[, n_data])"""
    n, m = np.asarray(observer).reshape(-1, 3).shape[0], np.asarray(target).reshape(-1, 3).shape[0]
    out = np.full((n,) if paired else (n, m), SENTINEL)
    return st.clearance(observer, target, fraction, layer, paired=paired, out=out, want=want)


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def check_against(profile, data_index, got, bar, label):
    """`got` against a profile of clearances [..][K] (NaN: skipped): n_data exactly; the sample where
    the profile's gap pins it, else one within the bar of the minimum; the clearance; the
    sentinels, to the bit.  Returns the worst difference."""
    want = CC.expected(profile, data_index)
    none = want["sample"] == 0
    if "n_data" in got:
        assert np.array_equal(got["n_data"], want["n_data"]), label
    assert np.array_equal(got["sample"] == 0, none), label
    assert np.array_equal(bits(got["clearance"][none]), bits(np.full(int(none.sum()), SENTINEL))), label
    if none.all():
        return 0.0
    pinned = ~none & (CC.gaps(profile) > bar)
    assert np.array_equal(got["sample"][pinned], want["sample"][pinned]), (label, got["sample"], want["sample"])
    filled = np.where(np.isnan(profile), np.inf, profile)
    at = np.take_along_axis(filled, np.maximum(got["sample"] - 1, 0)[..., None], -1)[..., 0]
    assert (at[~none] - want["clearance"][~none] <= bar).all(), label                       # (inf: a skipped one)
    worst = np.abs(got["clearance"][~none] - want["clearance"][~none]).max()
    print(f"{label}: {int((~none).sum())} lines, worst clearance difference {worst:.3e} m")
    assert worst <= bar, (label, worst)
    return worst


@pytest.fixture(scope="module")
def flat():
    """a flat layer at 0, with two points 800 m above it and 60 km apart, and a third at 300 m"""
    st = TA.Stepper()
    st.add_flat(0.0)
    pos, _ = st.position(np.array([12.0, 12.5, 12.2]), np.array([34.0, 34.2, 33.9]), np.array([800.0, 800.0, 300.0]))
    yield st, pos
    st.destroy()


# ---- against the reference -----------------------------------------------------------------------

@pytest.mark.parametrize("math", ["fast", "strict"])
@pytest.mark.parametrize("case", CC.CASES)
def test_against_the_reference(golden, geometries, case, math):
    g = golden("clearance")
    st = geometries(case)["stepper"]
    with math_mode(math):
        got = run(st, g[case + "_observer"], g[case + "_target"], g[case + "_fraction"], int(g[case + "_layer"]))
    assert st.rounds == 1
    assert (CC.gaps(g[case + "_profile"]) > CAP).all()         # the sample number is pinned on every line
    check_against(g[case + "_profile"], g[case + "_data_index"], got, BAR[math], f"{case} {math}")
    assert np.array_equal(got["sample"], g[case + "_sample"])
    assert np.array_equal(got["n_data"], g[case + "_n_data"])


# ---- ties, end points, NaN -------------------------------------------------------------------------

def test_ties_go_to_the_smaller_k(flat):
    st, pos = flat
    a, b = pos[:1], pos[1:2]
    for obs, tgt in ((a, b), (a, pos[2:3]), (pos[:2], pos)):
        got = run(st, obs, tgt, np.full(130, 0.37))                        # every sample ties
        assert (got["sample"] == 1).all() and (got["n_data"] == 130).all()
    # between points at equal height the chord is lowest at its middle: the first 0.5 wins, which is
    # lane 0's second turn, over the 64 samples at 0.3 before it and the 65 equal ones behind it
    got = run(st, a, b, [0.3] * 64 + [0.5] * 66)
    assert got["sample"].tolist() == [[65]] and got["clearance"][0, 0] < 800.0 - 60.0
    one = run(st, a, b, [0.5])
    assert np.array_equal(bits(one["clearance"]), bits(got["clearance"]))
    for pair, winner in (((3, 67), 4), ((4, 67), 5), ((66, 67), 67), ((1, 129), 2)):     # as test_gpu_horizon.py
        tied = np.linspace(0.05, 0.3, 130)
        tied[list(pair)] = 0.5
        assert run(st, a, b, tied)["sample"].tolist() == [[winner]], pair


def test_a_nan_fraction_never_wins(flat):
    st, pos = flat
    a, b = pos[:1], pos[1:2]
    fraction = np.full(130, 0.5)
    fraction[[0, 5, 64]] = np.nan
    got = run(st, a, b, fraction)
    assert got["sample"].tolist() == [[2]]
    assert np.array_equal(bits(got["clearance"]), bits(run(st, a, b, [0.5])["clearance"]))
    fraction = np.linspace(0.05, 0.3, 130)                                 # nor hides a winner behind it
    fraction[[99, 101]] = np.nan
    fraction[100] = 0.5
    assert run(st, a, b, fraction)["sample"].tolist() == [[101]]
    only_nan = run(st, a, b, [np.nan, np.nan, np.nan])
    assert only_nan["sample"].tolist() == [[0]]
    assert np.array_equal(bits(only_nan["clearance"]), bits(np.full((1, 1), SENTINEL)))


@pytest.mark.parametrize("math", ["fast", "strict"])
def test_the_end_points_stand_at_their_heights(flat, math):
    """over a flat layer at 0 a point's clearance is its geodetic altitude: fraction 0 gives the
    observer's height, fraction 1 the target's"""
    st, _ = flat
    heights = np.array([800.0, 2.0, 300.0, 4321.5])
    pos = TA.ecef_from_geodetic(np.array([12.0, 12.5, 12.2, 11.8]), np.array([34.0, 34.2, 33.9, 34.4]), heights)
    with math_mode(math):
        at_0, at_1 = run(st, pos, pos, [0.0]), run(st, pos, pos, [1.0])
    worst = max(np.abs(at_0["clearance"] - heights[:, None]).max(), np.abs(at_1["clearance"] - heights[None, :]).max())
    print(f"end points {math}: worst difference {worst:.3e} m")
    assert worst <= BAR[math]
    assert (at_0["sample"] == 1).all() and (at_1["sample"] == 1).all() and (at_0["n_data"] == 1).all()
    both = run(st, pos, pos, [1.0, 0.0])                                   # the lower of the two ends
    lower = np.minimum(heights[:, None], heights[None, :])
    assert np.abs(both["clearance"] - lower).max() <= BAR["fast"]
    off = ~np.eye(4, dtype=bool)
    assert np.array_equal(both["sample"][off], np.where(heights[None, :] < heights[:, None], 1, 2)[off])
    assert np.abs(np.diag(both["clearance"]) - heights).max() <= BAR["fast"]       # (p == t is not special)


# ---- shapes ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_f", [1, 63, 64, 65, 129])
def test_prefixes_of_the_fractions(golden, geometries, n_f):
    g = golden("clearance")
    for case in ("stack", "layers_geoid"):
        st = geometries(case)["stepper"]
        got = run(st, g[case + "_observer"], g[case + "_target"], g[case + "_fraction"][:n_f], int(g[case + "_layer"]))
        check_against(g[case + "_profile"][..., :n_f], g[case + "_data_index"][..., :n_f], got, BAR["fast"],
                      f"{case} n_fractions={n_f}")
        if n_f == 1:
            assert set(got["sample"].ravel().tolist()) == {1} and (got["n_data"] == 1).all()


def test_lines_that_do_not_fill_a_block_and_one_line_alone(golden, geometries):
    g = golden("clearance")
    st = geometries("stack")["stepper"]
    obs, tgt, fr = g["stack_observer"], g["stack_target"], g["stack_fraction"]
    full = run(st, obs, tgt, fr)
    for rows, cols in ((slice(2, 3), slice(3, 4)), (slice(1, 2), slice(1, 4)), (slice(0, 3), slice(5, 6)),
                       (slice(3, 4), slice(0, 5)), (slice(1, 2), slice(0, 6))):     # 1, 3, 3, 5 and 6 lines
        part = run(st, obs[rows], tgt[cols], fr)
        for name in CC.OUTPUTS:
            assert np.array_equal(part[name], full[name][rows, cols]), (rows, cols, name)


def test_paired_is_the_diagonal(golden, geometries):
    g = golden("clearance")
    for case in ("map", "layers_geoid"):
        st = geometries(case)["stepper"]
        obs, tgt, fr, layer = g[case + "_observer"], g[case + "_target"], g[case + "_fraction"], int(g[case + "_layer"])
        full = run(st, obs, tgt, fr, layer)
        for order in ([0, 1, 2, 3], [5, 0, 3, 3], [2]):
            n = len(order)
            got = run(st, obs[:n], tgt[order], fr, layer, paired=True)
            for name in CC.OUTPUTS:
                assert got[name].shape == (n,)
                assert np.array_equal(got[name], full[name][np.arange(n), order]), (case, order, name)
        out = np.full(4, SENTINEL)
        with pytest.raises(TA.TurtleError) as err:
            st.clearance(obs, tgt, fr, layer, paired=True, out=out)        # 4 observers, 6 targets
        assert err.value.name == "DOMAIN_ERROR" and "turtle_stepper_clearance_n" in str(err.value)
        assert (out == SENTINEL).all()


# ---- no data, the optional output --------------------------------------------------------------------

def test_a_line_off_the_data_keeps_its_clearance(golden, geometries):
    g = golden("clearance")
    st = geometries("map")["stepper"]
    away = TA.ecef_from_geodetic(np.array([5.0, 5.3]), np.array([5.0, 4.8]), np.array([1500.0, 30.0]))   # 4 degrees off
    obs = np.concatenate([g["map_observer"][:2], away[:1], g["map_observer"][2:]])
    tgt = np.concatenate([g["map_target"], away[1:]])
    got = run(st, obs, tgt, g["map_fraction"])
    assert got["sample"][2, 6] == 0 and got["n_data"][2, 6] == 0
    assert bits(got["clearance"])[2, 6] == bits(np.array([SENTINEL]))[0]
    assert (got["sample"][2, :5] > 0).all() and (got["sample"][:, 6] > 0)[[0, 1, 3, 4]].all()   # lines INTO the data
    keep = [0, 1, 3, 4]
    for name in ("sample", "n_data"):
        assert np.array_equal(got[name][keep][:, :6], g["map_" + name]), name
    bare = run(st, obs, tgt, g["map_fraction"], want=())                   # n_data NULL: no bit of the others moves
    assert "n_data" not in bare
    assert np.array_equal(bits(bare["clearance"]), bits(got["clearance"])) and np.array_equal(bare["sample"], got["sample"])


# ---- spaces ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["stack", "layers_geoid"])
def test_spaces_give_the_same_bits_and_the_stream_is_honoured(golden, geometries, case):
    import torch
    g = golden("clearance")
    st = geometries(case)["stepper"]
    obs, tgt, fr, layer = g[case + "_observer"], g[case + "_target"], g[case + "_fraction"], int(g[case + "_layer"])
    host = run(st, obs, tgt, fr, layer)
    stream = torch.cuda.Stream()
    try:
        with torch.cuda.stream(stream):
            TA.set_stream(stream)
            # inputs made, and outputs read, by work queued on the same stream around the call
            d_obs = torch.zeros(obs.shape, dtype=torch.float64, device="cuda")
            d_obs += torch.as_tensor(obs).pin_memory().to("cuda", non_blocking=True)
            d_tgt = torch.zeros(tgt.shape, dtype=torch.float64, device="cuda")
            d_tgt += torch.as_tensor(tgt).pin_memory().to("cuda", non_blocking=True)
            out = torch.full(host["clearance"].shape, SENTINEL, dtype=torch.float64, device="cuda")
            dev = st.clearance(d_obs, d_tgt, torch.as_tensor(fr, device="cuda"), layer, out=out)
            back = {k: v.clone() for k, v in dev.items()}
        stream.synchronize()
    finally:
        TA.set_stream(None)
    assert dev["clearance"] is out and dev["sample"].is_cuda and dev["n_data"].is_cuda
    for name in CC.OUTPUTS:
        assert np.array_equal(back[name].cpu().numpy(), host[name]), name


# ---- residency -------------------------------------------------------------------------------------

def test_the_call_loads_the_tiles_it_needs(golden, tmp_path):
    g = golden("clearance")
    geo = NC.amd_geometry("stack", str(tmp_path), 0)           # stack_size 0: no limit; nothing loaded yet
    try:
        stack = geo["layers"][0][0][1]
        assert stack.resident == 0
        got = run(geo["stepper"], g["stack_observer"], g["stack_target"], g["stack_fraction"])
        assert stack.resident == 3 and geo["stepper"].rounds == 1
        assert np.array_equal(got["sample"], g["stack_sample"]) and np.array_equal(got["n_data"], g["stack_n_data"])
    finally:
        NC.destroy(geo)


def test_a_stack_too_small_for_its_tiles_is_refused(golden, tmp_path):
    g = golden("clearance")
    geo = NC.amd_geometry("stack", str(tmp_path), 1)           # three tiles, room for one
    try:
        stack = geo["layers"][0][0][1]
        before = stack.resident
        out = np.full(g["stack_sample"].shape, SENTINEL)
        with pytest.raises(TA.TurtleError) as err:
            geo["stepper"].clearance(g["stack_observer"], g["stack_target"], g["stack_fraction"], 0, out=out)
        assert err.value.name == "DOMAIN_ERROR" and "turtle_stepper_clearance_n" in str(err.value)
        assert "a device view" not in str(err.value) and "stack_size 1" in str(err.value)
        assert (out == SENTINEL).all()
        assert stack.resident == before
    finally:
        NC.destroy(geo)


# ---- against the composition of the calls that existed before ------------------------------------------

def test_against_the_composition_of_the_older_calls(tmp_path):
    """a geometry larger than the fixture's: one rough tile of 1201 x 1201 nodes, 16 observers x 16
    targets x 200 fractions, every sample point built on the host and taken through
    turtle_ecef_to_geodetic_n (STRICT), turtle_stepper_position_n and numpy"""
    with SC.rough_lines(str(tmp_path)) as r:
        st, obs = r["stepper"], r["position"]
        rng = np.random.Generator(np.random.Philox(82))
        n, m, n_f = obs.shape[0], 16, 200
        # targets in the air, some of them beyond the tile's northern and eastern rims: lines leave the data
        tgt = TA.ecef_from_geodetic(rng.uniform(45.1, 46.2, m), rng.uniform(3.1, 4.2, m), rng.uniform(300.0, 5000.0, m))
        fr = CC.fractions(n_f)
        with math_mode("strict"):
            got = run(st, obs, tgt, fr)
            p, d = obs.reshape(n, 1, 1, 3), (tgt.reshape(1, m, 3) - obs.reshape(n, 1, 3)).reshape(n, m, 1, 3)
            q = np.stack([p[..., j] + fr.reshape(1, 1, n_f) * d[..., j] for j in range(3)], -1)
            la, lo, _ = TA.ecef_to_geodetic(q.reshape(-1, 3))
            ground, di = st.position(la, lo, 0.0, 0)
        lam, phi = lo * np.pi / 180.0, la * np.pi / 180.0
        sl, cl, sp, cp = np.sin(lam), np.cos(lam), np.sin(phi), np.cos(phi)
        up = np.stack([cl * cp, sl * cp, sp], -1)
        off = q.reshape(-1, 3) - ground
        profile = (up[:, 0] * off[:, 0] + up[:, 1] * off[:, 1] + up[:, 2] * off[:, 2]).reshape(n, m, n_f)
        di = di.reshape(n, m, n_f)
        profile[di < 0] = np.nan
        want = CC.expected(profile, di)
        assert (want["n_data"] < n_f).any() and (want["n_data"] > 0).all()             # lines leave the tile
        assert (want["clearance"] < -1.0).any() and (want["clearance"] > 1.0).any()    # blocked ones, open ones
        print("composition: winners on", len(set(want["sample"].ravel().tolist())), "different samples,",
              int((got["sample"] != want["sample"]).sum()), "lines differ in the sample")
        check_against(profile, di, got, BAR["strict"], "composition")


# ---- the example -------------------------------------------------------------------------------------

def test_clearance_example(tmp_path):
    exe = SC.build_example("clearance", tmp_path)
    tile = synth.write_rough_hgt(str(tmp_path), 45, 3)
    out = subprocess.run([exe, tile], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    rows = [l.split() for l in lines if l.startswith("station")]
    assert len(rows) == 20 and all(r[4] in ("seen", "blocked") for r in rows)
    assert lines[-1].endswith("of 20 pairs see each other")
    # the same matrix through the binding
    m = TA.Map.load(tile)
    st = TA.Stepper()
    st.add_map(m, 0.0)
    try:
        info = m.meta()
        (x0, x1), (y0, y1) = info["x"], info["y"]
        at = np.array([(0.2, 0.3), (0.7, 0.2), (0.5, 0.5), (0.3, 0.8), (0.85, 0.75)])
        air = np.array([(0.4, 0.4, 1200.0), (0.6, 0.7, 2500.0), (0.1, 0.6, 6000.0), (1.2, 0.5, 4000.0)])
        station, _ = st.position(y0 + at[:, 1] * (y1 - y0), x0 + at[:, 0] * (x1 - x0), 3.0)
        point = TA.ecef_from_geodetic(y0 + air[:, 1] * (y1 - y0), x0 + air[:, 0] * (x1 - x0), air[:, 2])
        fr = CC.fractions(512)
        got = st.clearance(station, point, fr)
        assert (got["n_data"][:, 3] < 512).all() and (got["n_data"][:, :3] == 512).all()
        seen = np.array([r[4] == "seen" for r in rows]).reshape(5, 4)
        assert np.array_equal(seen, got["clearance"] >= 0.0) and 0 < seen.sum() < 20
        assert lines[-1].startswith(f"{int(seen.sum())} of 20")
        assert np.abs(np.array([float(r[6]) for r in rows]).reshape(5, 4) - got["clearance"]).max() < 2e-3
        assert np.abs(np.array([float(r[10]) for r in rows]).reshape(5, 4) - fr[got["sample"] - 1]).max() < 1e-6
        assert np.array_equal(np.array([int(r[11][1:]) for r in rows]).reshape(5, 4), got["n_data"])
    finally:
        st.destroy()
        m.destroy()
