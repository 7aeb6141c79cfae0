"""trace_n and step_n over rough and void ground (tests/rough_cases.py), against the reference's
own outputs (tests/golden/rough.npz) and, at full size, against the CPU restatement.

The bar, for every ray and in both arithmetics: the same final index pair, the path length within
1e-6 of the reference's, the step count within one.  A ray outside it is classified here, by
replaying the oracle (pinned bit for bit to the reference by test_oracle_golden.py) to the
reference's last step and working out that step's bracket [L, L + ds] by the reference's rule
[ref stepper.c:799-813]:
  * "other root": the GPU took as many steps and its end lies in that bracket, but farther than
    the bar (and 1e-8 m) from the reference's end: on another crossing -- the bracket held several,
    and the GPU located another one than the reference's halving does.  Never allowed.
  * "grazing": any other ray outside the bar -- a decision taken within an ulp of a surface, or a
    sliver thinner than a step, that went the other way earlier on.  Named below,
    by run, and at most max(3, 1e-4 n) of the n rays of a run.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import turtle_amd as TA
from oracle import ffi as O

import rough_cases as RC
import terrains as T

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BAR = 1e-6
FULL = 1_000_000
MACHINERY = 100_000

# The grazing rays of each run, by id: (run, arithmetic) -> ray ids
GRAZING = {
    ("void_ground", "fast"): [9409],     # a path of 1.5 mm: the bar (1.5e-9 m) is below the bracket's 1e-8 m
    ("rough3601", "fast"): [502277],     # two steps fewer, the same end to 7e-10 m
    ("stack", "fast"): [47927],          # likewise: a path of millimetres
}


@pytest.fixture(params=["fast", "strict"])
def math(request):
    TA.set_math(request.param)
    yield request.param
    TA.set_math("fast")


def step_length(alt, elevation, medium, n_layers, slope=0.4, resolution=1e-2):
    """[ref stepper.c:799-813] the tentative step from a sample"""
    ds = np.zeros(alt.shape)
    for i in (0, 1):
        use = (medium != 0) if i == 0 else (medium != n_layers)
        dsi = np.abs(alt - elevation[:, i])
        ds = np.where(use & ((dsi < ds) | (ds <= 0.)), dsi, ds)
    ds *= slope
    return np.where(ds < resolution, resolution, ds)


def classify(geo, pos, d, got, ref):
    """(ids outside the bar, "other root" ids, grazing ids)"""
    L, L0 = np.asarray(got["length"]), ref["length"]
    bad = (np.asarray(got["index"]) != ref["index"]).any(axis=1)
    bad |= np.abs(L - L0) > BAR * np.maximum(L0, 1e-300)
    bad |= np.abs(np.asarray(got["n_steps"]) - ref["n_steps"]) > 1
    ids = np.flatnonzero(bad)
    other = []
    for r in ids:
        n = int(ref["n_steps"][r])
        if n < 1:
            continue
        # the reference before its last step, and the bracket [L, L + ds] that step explored
        t = geo.trace(pos[r:r + 1], d[r:r + 1], max_steps=n - 1)
        s = geo.step(t["position"])
        ds = step_length(s["altitude"], s["elevation"], s["index"][:, 0], geo.n_layers)
        assert ds[0] == s["step"][0]   # (the rule is the restatement's)
        lo, hi = t["length"][0], t["length"][0] + ds[0]
        tol = max(BAR * L0[r], 1e-8)   # (1e-8 m: where the reference's halving ends)
        same_steps = np.asarray(got["n_steps"])[r] == n
        if same_steps and (lo - tol <= L[r] <= hi + tol) and (abs(L[r] - L0[r]) > tol):
            other.append(int(r))
    grazing = sorted(set(ids.tolist()) - set(other))
    return ids, other, grazing


def assert_bar(geo, pos, d, got, ref, run, math):
    n = pos.shape[0]
    ids, other, grazing = classify(geo, pos, d, got, ref)
    L, L0 = np.asarray(got["length"]), ref["length"]
    dsteps = np.asarray(got["n_steps"]) - ref["n_steps"]
    print(f"\n[{run} {math}] {n} rays: {ids.size} outside the bar, {len(other)} other root, "
          f"{len(grazing)} grazing")
    for r in ids[:40]:
        print(f"  ray {r}: {'OTHER ROOT' if r in other else 'grazing'} dL {L[r] - L0[r]:+.3e} m of "
              f"{L0[r]:.1f}, index {np.asarray(got['index'])[r]} vs {ref['index'][r]}, steps {dsteps[r]:+d}")
    print(f"  GRAZING[({run!r}, {math!r})] = {grazing}")
    assert other == [], f"{run} {math}: {len(other)} rays end on another root: {other[:20]}"
    assert len(grazing) <= max(3, int(1e-4 * n)), f"{run} {math}: {len(grazing)} grazing rays"
    assert grazing == sorted(GRAZING.get((run, math), [])), f"{run} {math}: grazing rays {grazing}"


@pytest.fixture(scope="module")
def tiles(tmp_path_factory):
    out = {}
    for case in RC.CASES:
        m = TA.Map.load(RC.write_tile(tmp_path_factory.mktemp(case), case))
        st = TA.Stepper()
        st.add_map(m, 0.0)
        out[case] = (m, st, RC.oracle_geometry(case))
    yield out
    for m, st, _ in out.values():
        st.destroy()
        m.destroy()


def golden_rays(g, case, recipe):
    pos, d = RC.oracle_rays(case, recipe)
    k = f"{case}_{recipe}_"
    assert RC.sha(pos) == str(g[k + "origin_sha"]) and RC.sha(d) == str(g[k + "direction_sha"])
    ref = dict(index=g[k + "index"].astype(np.int32), length=g[k + "length"], n_steps=g[k + "n_steps"])
    return pos, d, ref


@pytest.mark.parametrize("case, recipe", [(c, r) for c in RC.CASES for r in RC.recipes(c)])
def test_trace_matches_the_reference(tiles, golden, math, case, recipe):
    g = golden("rough")
    assert RC.sha(RC.nodes(case)) == str(g[f"{case}_nodes_sha"])
    m, st, geo = tiles[case]
    pos, d, ref = golden_rays(g, case, recipe)
    t = st.trace(pos.copy(), d)
    assert_bar(geo, pos, d, t, ref, f"{case}_{recipe}", math)
    s = st.trace_stats()
    assert s["rays"] == pos.shape[0] and s["steps"] == int(t["n_steps"].sum()) and s["capped"] == 0


@pytest.mark.parametrize("case", RC.CASES)
def test_step_n_per_step_records(tiles, golden, math, case):
    """every step of 2 000 rays through every medium (k_step_fast + k_bisect in the fast arithmetic),
    from the reference's position before it, with the bar of test_c1_per_step_records.

    A step that starts where the step before it located a crossing starts ON the ground, within the
    1e-8 m of the reference's bracket: a fresh sample there (turtle_stepper_step_n without
    TURTLE_AMD_STEP_RESUME) may find either medium by an ulp of the transform.  Where the library's
    sample of the start finds another medium than the reference's, the step is another one -- it
    bisects back to its start, or does not -- and only these steps may fall outside the bar; they end
    in the reference's medium, within one minimum step (1e-2 m) of the reference's end."""
    g = golden("rough")
    m, st, geo = tiles[case]
    pos, d, _ = golden_rays(g, case, "ground")
    pos, d = pos[:RC.STEP_RAYS], d[:RC.STEP_RAYS]
    ds, index, position = RC.oracle_step_records(geo, pos, d)
    assert RC.sha(position) == str(g[f"{case}_steps_position_sha"]) and RC.sha(ds) == str(g[f"{case}_steps_ds_sha"])
    assert np.array_equal(index, g[f"{case}_steps_index"].astype(np.int32))
    medium0 = geo.step(pos)["index"][:, 0]
    on_ground = flipped = 0
    for k in range(RC.STEPS):
        rays = np.flatnonzero(index[:, k, 0] != -2)
        before = pos[rays] if k == 0 else position[rays, k - 1]
        o = st.step(before.copy(), d[rays])
        bad = (o["index"] != index[rays, k]).any(axis=1)
        bad |= np.abs(o["step"] - ds[rays, k]) > 1e-6 * np.abs(ds[rays, k]).max()
        bad |= np.abs(o["position"] - position[rays, k]).max(axis=1) >= 1e-5
        if k == 0:
            assert not bad.any()
            continue
        # the steps that start on a crossing located by the step before, and of those the ones
        # whose start the library samples in another medium than the reference
        came_from = medium0[rays] if k == 1 else index[rays, k - 2, 0]
        starts_on_ground = index[rays, k - 1, 0] != came_from
        on_ground += int(starts_on_ground.sum())
        start = st.step(before.copy())["index"][:, 0]
        other_start = starts_on_ground & (start != geo.step(before)["index"][:, 0])
        flipped += int(other_start.sum())
        assert not (bad & ~other_start).any(), (k, rays[bad & ~other_start])
        assert np.array_equal(o["index"][bad], index[rays[bad], k])
        assert (np.abs(o["position"] - position[rays, k]).max(axis=1)[bad] <= 1.01e-2).all()
    print(f"\n[{case} {math}] {on_ground} steps start on a crossing; the library samples {flipped} of "
          f"those starts in the other medium")
    assert on_ground > 1000 and flipped <= 0.1 * on_ground


def test_fast_transform_deep_below_the_ellipsoid(golden):
    """The fast ECEF -> geodetic of the trace kernel 25 .. 40 km below the ellipsoid (where a ray over
    an HGT void runs), with the bar of test_fast_transform_accuracy"""
    g = golden("rough")
    TA.set_math("fast")
    # the reference's points and answers, as the oracle (pinned to them by sha256) recomputes them
    e, (lat, lon, alt) = RC.deep_transforms(O.ecef_from_geodetic, O.ecef_to_geodetic)
    assert RC.sha(e) == str(g["deep_ecef_sha"]) and RC.sha(np.stack([lat, lon, alt])) == str(g["deep_geodetic_sha"])
    la, lo, al = TA.ecef_to_geodetic(e)
    dlat, dlon, dalt = np.abs(la - lat), np.abs(lo - lon), np.abs(al - alt)
    print(f"fast transform, 25-40 km down: max |dlat| {dlat.max():.2e} deg, |dlon| {dlon.max():.2e} deg, "
          f"|dalt| {dalt.max():.2e} m")
    assert dlat.max() < 5e-14 and dalt.max() < 6e-9 and dlon.max() < 1e-13


@pytest.fixture(scope="module")
def full_size(tmp_path_factory, golden):
    """10^6 rays of C2's recipe over the full-size rough tile, and the CPU restatement's traces"""
    nodes = RC.nodes("rough", RC.FULL_N)
    assert RC.sha(nodes) == str(golden("rough")["rough3601_nodes_sha"])
    m = TA.Map.load(RC.synth.write_nodes_hgt(str(tmp_path_factory.mktemp("rough3601")), RC.LAT0, RC.LON0, nodes))
    st = TA.Stepper()
    st.add_map(m, 0.0)
    geo = RC.oracle_geometry("rough", RC.FULL_N)
    pos, d = RC.rays("rough", "c2", geo.position, O.ecef_from_horizontal, FULL)
    ref = geo.trace(pos, d, max_steps=1000000, threads=max(1, min(16, os.cpu_count() or 1)))
    yield dict(stepper=st, geo=geo, pos=pos, dir=d, ref=ref)
    st.destroy()
    m.destroy()


def test_full_size_against_cpu_oracle(full_size, math):
    f = full_size
    t = f["stepper"].trace(f["pos"].copy(), f["dir"], max_steps=1000000)
    assert_bar(f["geo"], f["pos"], f["dir"], t, f["ref"], "rough3601", math)
    assert (t["index"][:, 0] == 0).sum() > FULL // 2   # most of them hit the ground


def test_optional_machinery_gives_the_same_bits(tmp_path):
    """The ray pool, the rays in the order of where they start and the ordered hand-over, all forced
    on, all forced off and at their defaults, each in a process of its own (the library reads the
    switches once): the same bits on the rough and void tiles, and through the 2 x 2 stack paged one
    tile at a time in STRICT.  In FAST a ray that waited for a tile goes on along a new line, laid
    where it waited (test_gpu_paging.test_trace_paged): the same media and step counts, the lengths
    within 1e-9.  Both paged runs meet the bar against the oracle's mosaic."""
    settings = {"off": dict(TURTLE_AMD_POOL="0", TURTLE_AMD_SPATIAL="0", TURTLE_AMD_SORT_KEY="0"),
                "on": dict(TURTLE_AMD_POOL="1", TURTLE_AMD_SPATIAL="1", TURTLE_AMD_SORT_KEY="1"),
                "defaults": {}}
    env0 = {k: v for k, v in os.environ.items()
            if k not in ("TURTLE_AMD_POOL", "TURTLE_AMD_SPATIAL", "TURTLE_AMD_SORT_KEY")}
    results = {}
    for tag, env in settings.items():
        out = os.path.join(tmp_path, f"{tag}.npz")
        subprocess.run([sys.executable, os.path.join(HERE, "rough_probe.py"), out, str(tmp_path / f"work_{tag}"),
                        str(MACHINERY)], check=True, env=dict(env0, **env), timeout=600)
        results[tag] = dict(np.load(out))
    base = results["off"]
    assert base["stack_strict_rounds"] > 1 and base["stack_fast_rounds"] > 1
    for tag, r in results.items():
        for key, ref in base.items():
            if key.startswith("stack_fast_"):
                continue
            if not key.endswith("_rounds"):
                assert np.array_equal(r[key], ref), (tag, key)
        for key in ("index", "n_steps"):
            assert np.array_equal(r["stack_fast_" + key], base["stack_fast_" + key]), (tag, key)
        L, L0 = r["stack_fast_length"], base["stack_fast_length"]
        assert (np.abs(L - L0) <= 1e-9 * np.maximum(L0, 1.0)).all(), tag
    geo = T.mosaic_oracle_nodes(RC.stack_nodes(), 45, 3, 2, 2)
    pos, d = base["stack_origin"], base["stack_direction"]
    ref = geo.trace(pos, d, max_steps=1000000, threads=max(1, min(16, os.cpu_count() or 1)))
    for math in ("strict", "fast"):
        got = {k: base[f"stack_{math}_{k}"] for k in ("index", "length", "n_steps")}
        assert_bar(geo, pos, d, got, ref, "stack", math)
    lat0, lon0, _ = O.ecef_to_geodetic(pos)
    lat1, lon1, _ = O.ecef_to_geodetic(base["stack_strict_position"])
    assert ((np.floor(lat1) != np.floor(lat0)) | (np.floor(lon1) != np.floor(lon0))).sum() > 100
