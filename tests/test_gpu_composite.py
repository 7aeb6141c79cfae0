"""The stepping kernels over composite geometries (tests/composite_cases.py) -- all of them
TAMD_MODE_GENERIC: a stack beside maps and flats in one layer, overlapping maps, layers without data,
a projected map beside other data, a geoid -- against the reference's own results
(tests/golden/composite.npz) and the CPU restatement, itself pinned on these geometries to the
reference bit for bit (tests/test_oracle_golden.py, g14).

What forks here and nowhere else in the suite: the reference's "last added first" priority within a
layer, falling through to the next data where a map ends or the stack has a hole, a layer that has
no data at a point, k_trace<GENERIC>'s second phase (the hand-over at step 512), the CAN_PAGE
instances of k_trace, k_cross and k_traverse for GENERIC, and k_walk, k_step and k_traverse<REC>
for GENERIC over anything but one map twice.

The bars are those of the one-map and one-stack tests, named at each test.  No ray is set apart:
OUTSIDE is empty."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

import turtle_amd as TA
from oracle import ffi as O

import composite_cases as CO
import crossings_cases as CC
import traverse_cases as TC
from test_gpu_crossings import outside_bar
from test_gpu_device_api import both_forms
from test_gpu_parity import check_trace
from test_gpu_properties import HAND_OVER_MOVED
from test_gpu_traverse import assert_bar, same_bits

pytestmark = pytest.mark.gpu

# (case, math) -> rays of "sight" outside the bar; only rays whose first disagreement follows a
# reference crossing located within 1e-9 degree of a rim line (CO.on_a_rim) may be named.  None is.
OUTSIDE = {}
DBL_MAX = np.finfo(np.float64).max
MODE_OFFSET = 72        # struct tamd_view (include/turtle_amd_device.h): six pointers, n_layers, geoid,
GENERIC = 0             # slope, resolution, then `mode`


@pytest.fixture(params=["fast", "strict"])
def math(request):
    TA.set_math(request.param)
    yield request.param
    TA.set_math("fast")


@pytest.fixture(scope="module")
def made(tmp_path_factory):
    """case -> dict(amd: the resident geometry, stepper, geo: the restatement, graze: (pos, dir),
    ref: the restatement's trace of graze); built once, left unchanged"""
    out = {}

    def get(case):
        if case not in out:
            amd = CO.amd_geometry(case, tmp_path_factory.mktemp(case))
            geo = CO.oracle_geometry(case)
            pos, d, _ = CO.graze(case, geo)
            ref = geo.trace(pos, d, max_steps=CO.GRAZE_MAX_STEPS, threads=8)
            out[case] = dict(amd=amd, stepper=amd["stepper"], geo=geo, graze=(pos, d), ref=ref)
        return out[case]

    yield get
    for s in out.values():
        CO.destroy(s["amd"])


def report(tag, t, ref):
    L, L0 = np.asarray(t["length"]), ref["length"]
    rel = np.abs(L - L0) / np.maximum(np.abs(L0), 1e-300)
    print(f"\n[{tag}] {int((np.asarray(t['n_steps']) > 512).sum())} rays beyond 512 steps, "
          f"{int((t['index'] != ref['index']).any(axis=1).sum())} index pairs differ, worst |dL|/L "
          f"{rel[L0 > 0].max():.3e}, {int((t['n_steps'] != ref['n_steps']).sum())} step counts differ")


# ---- flattening -------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CO.CASES + ("example_open",))
def test_flattening(made, case):
    st = made(case)["stepper"]
    layers = len(CO.RECIPES[case][1])
    assert st.media == layers + 1
    with st.view() as v:
        assert struct.unpack_from("i", v, MODE_OFFSET)[0] == GENERIC
        assert struct.unpack_from("i", v, 48)[0] == layers


# ---- rims -------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CO.CASES)
def test_rims(made, golden, math, case):
    """position_n on every layer below the lid and step_n without a direction, 1e-12 .. 1e-4 degree
    either side of every rim line -- the maps' rims, the stack's, the edges of its missing tile --
    against the reference: the same data index and inside verdict, the same index pair; positions
    within 5e-9 m (test_gpu_irregular.test_lookups), elevations within 1e-9 m and the +-DBL_MAX
    sentinels exact (test_layers_offsets_flat_geoid).  STRICT on every point; FAST leaves out the
    points closer than 1e-9 degree to their rim."""
    g, st = golden("composite"), made(case)["stepper"]
    k = f"{case}_rim_"
    lat, lon, eps = CO.rim_points(case)
    assert CO.sha(np.stack([lat, lon])) == str(g[k + "points_sha"])
    keep = np.ones(lat.size, dtype=bool) if math == "strict" else eps >= 1e-9
    assert keep.sum() >= (1.0 if math == "strict" else 0.6) * lat.size
    answers = set()
    for layer in range(len(CO.RECIPES[case][1]) - 1):
        pos, di = st.position(lat, lon, 100.0, layer=layer)
        di0, pos0 = g[k + f"data{layer}"].astype(np.int32), g[k + f"position{layer}"]
        answers |= {(layer, int(v)) for v in np.unique(di0)}
        bad = np.flatnonzero((di != di0) & keep)
        assert bad.size == 0, (layer, bad[:10], eps[bad[:10]], di[bad[:10]], di0[bad[:10]])
        inside = keep & (di0 >= 0)
        assert np.abs(pos - pos0)[inside].max() < 5e-9
    start = O.ecef_from_geodetic(lat, lon, np.full(lat.size, 2500.0))
    assert CO.sha(start) == str(g[k + "start_sha"])
    o, rows = st.step(start.copy(), None), g[k + "step"]
    bad = np.flatnonzero((o["index"] != rows[:, 5:7].astype(np.int32)).any(axis=1) & keep)
    assert bad.size == 0, (bad[:10], eps[bad[:10]], o["index"][bad[:10]], rows[bad[:10], 5:7])
    e, e0 = o["elevation"][keep], rows[keep, 3:5]
    big = np.abs(e0) > 1e300
    assert np.array_equal(e[big], e0[big])
    off = np.where(big, 0.0, np.abs(e - e0)).max(axis=1)
    print(f"\n[{case} {math}] rims: worst elevation difference {off.max():.3e} m")
    for r in np.argsort(-off)[:8]:
        if off[r] >= 1e-9:
            q = np.flatnonzero(keep)[r]
            print(f"  point {q}: lat {lat[q]!r} lon {lon[q]!r} eps {eps[q]:.0e}: elevation {e[r]} vs {e0[r]}, "
                  f"latitude {o['latitude'][q] - rows[q, 0]:+.3e} longitude {o['longitude'][q] - rows[q, 1]:+.3e}")
    assert off.max() < 1e-9
    assert np.abs(o["altitude"][keep] - rows[keep, 2]).max() < 5e-9
    assert len(answers) >= 3                                 # the points do fork: (layer, data index)


# ---- trace ------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CO.CASES)
def test_trace(made, golden, math, case):
    """"graze" and "under": the reference's 500 golden rays at range 0 and at range 1, then all
    1 500 (and the 750 from below the composite layer) against the restatement, no ray allowed
    for: identical index PAIR, path length within 1e-6, step counts within check_trace's own
    allowance; at least 300 rays pass the hand-over at step 512 by the GPU's own count."""
    s, g = made(case), golden("composite")
    st, (pos, d), ref = s["stepper"], s["graze"], s["ref"]
    t = st.trace(pos.copy(), d, max_steps=CO.GRAZE_MAX_STEPS)
    report(f"{case} {math} graze", t, ref)
    n = CO.GOLDEN_RAYS
    head = {key: np.asarray(v)[:n] for key, v in t.items()}
    for tag in ("r0", "r1"):
        k = f"{case}_{tag}_"
        check_trace(head, g[k + "index"].astype(np.int32), g[k + "length"], g[k + "n_steps"],
                    f"{case} {math} golden {tag}", allow=0)
        assert np.array_equal(head["index"], g[k + "index"].astype(np.int32))
    check_trace(t, ref["index"], ref["length"], ref["n_steps"], f"{case} {math}", allow=0)
    assert np.array_equal(t["index"], ref["index"])
    assert (np.asarray(t["n_steps"]) > 512).sum() >= 300
    # (the end point is the origin and the length along the direction: the bar on the length)
    off = np.abs(t["position"] - ref["position"]).max(axis=1)
    assert (off <= 1e-6 * np.maximum(ref["length"], 1.0)).all()
    stats = st.trace_stats()
    assert stats["rays"] == pos.shape[0] and stats["steps"] == int(t["n_steps"].sum()) and stats["capped"] == 0
    # from below the composite layer: the data changes on the way (test_composite_host.py)
    pos, d, _ = CO.under(case, s["geo"])
    ref = s["geo"].trace(pos, d, max_steps=CO.GRAZE_MAX_STEPS, threads=8)
    t = st.trace(pos.copy(), d, max_steps=CO.GRAZE_MAX_STEPS)
    report(f"{case} {math} under", t, ref)
    check_trace(t, ref["index"], ref["length"], ref["n_steps"], f"{case} {math} under", allow=0)
    assert np.array_equal(t["index"], ref["index"])
    assert (np.asarray(t["n_steps"]) > 512).sum() >= 200


@pytest.mark.parametrize("case", CO.CASES)
def test_resumed_trace(made, math, case):
    """each ray continued from where the reference's ended, with resume_index, twice, as
    test_layers_offsets_flat_geoid does it: against the restatement's continuation.  A flat has
    no end, so a ray may go on for ever above the lid or under the ground: the rays continued are
    those whose continuation ends before 20 000 steps in the restatement."""
    s = made(case)
    st, geo, (_, d), last = s["stepper"], s["geo"], s["graze"], s["ref"]
    rows = np.arange(d.shape[0])
    for leg in (2, 3):
        ref = geo.trace(last["position"], d[rows], max_steps=20000, threads=8)
        ends = (ref["n_steps"] < 20000) & np.isfinite(ref["length"]) & (last["index"][:, 0] >= 0)
        assert ends.sum() >= 100, (leg, ends.sum())
        t = st.trace(last["position"][ends].copy(), d[rows][ends], max_steps=20000,
                     resume_index=last["index"][ends])
        ref = {k: v[ends] for k, v in ref.items() if isinstance(v, np.ndarray)}
        report(f"{case} {math} leg {leg}", t, ref)
        check_trace(t, ref["index"], ref["length"], ref["n_steps"], f"{case} {math} leg {leg}", allow=0)
        assert np.array_equal(t["index"], ref["index"])
        rows, last = rows[ends], ref


@pytest.mark.parametrize("case", CO.CASES)
def test_odd_batch_sizes(made, math, case):
    """the first 1, 63, 64, 65 and 257 rays of "graze" sorted longest first, alone: the bits they get
    in the whole batch.  The single ray is one that hands over at step 512.  (The few rays beyond
    25 000 steps are left to test_trace: a lone ray of 84 000 steps takes a second a launch.)"""
    s = made(case)
    order = np.argsort(-s["ref"]["n_steps"], kind="stable")
    order = order[s["ref"]["n_steps"][order] <= 25000]
    assert order.size > 1400
    pos, d = np.ascontiguousarray(s["graze"][0][order]), np.ascontiguousarray(s["graze"][1][order])
    whole = s["stepper"].trace(pos.copy(), d, max_steps=CO.GRAZE_MAX_STEPS)
    assert whole["n_steps"][0] > 10000 and whole["n_steps"][256] > 512
    for n in (1, 63, 64, 65, 257):
        t = s["stepper"].trace(pos[:n].copy(), d[:n], max_steps=CO.GRAZE_MAX_STEPS)
        for k in ("index", "length", "n_steps", "position"):
            assert np.array_equal(t[k], whole[k][:n]), (n, k)


# ---- traverse and crossings -------------------------------------------------------------------

@pytest.mark.parametrize("case", CO.CASES)
def test_traverse_and_crossings(made, golden, math, case):
    """2 000 lines of sight up to 5 000 m, 20 000 steps at most, against the loops of traverse_cases
    and crossings_cases over the restatement (their first 500 the reference's own: composite.npz)
    at their bars: the same final index pair, crossing and step counts, every per-medium length,
    crossing distance and point within 1e-6 of the ray's path; crossings_n's shared outputs are the
    bits of traverse_n."""
    s, g = made(case), golden("composite")
    st, geo = s["stepper"], s["geo"]
    pos, d = CO.sight(case)
    ref = CC.check(geo, pos, d, CO.CEILING, max_steps=CO.SIGHT_MAX_STEPS, threads=8)
    same_bits(TC.check(geo, pos, d, CO.CEILING, max_steps=CO.SIGHT_MAX_STEPS, threads=8), ref,
              ("index", "length", "n_steps", "n_crossings"))
    k, n = f"{case}_sight_", CO.GOLDEN_RAYS
    assert np.array_equal(ref["length"][:, :n], g[k + "length"]) and np.array_equal(ref["n_steps"][:n], g[k + "n_steps"])
    t = st.traverse(pos.copy(), d, CO.CEILING, max_steps=CO.SIGHT_MAX_STEPS)
    total = ref["length"].sum(axis=0)
    off = np.abs(t["length"] - ref["length"]).max(axis=0) / np.maximum(total, 1e-300)
    print(f"\n[{case} {math}] sight: {int((t['n_steps'] > 512).sum())} rays beyond 512 steps, worst |dL|/L "
          f"{off.max():.3e}, {int((t['n_steps'] != ref['n_steps']).sum())} step counts and "
          f"{int((t['n_crossings'] != ref['n_crossings']).sum())} crossing counts differ")
    named = OUTSIDE.get((case, math), ())
    assert len(named) <= (0 if math == "strict" else CO.SIGHT // 100)
    assert_bar(t, ref, f"{case} {math}", named)
    capacity = int(ref["n_crossings"].max()) + 1
    x = st.crossings(pos.copy(), d, CO.CEILING, max_steps=CO.SIGHT_MAX_STEPS, capacity=capacity)
    same_bits(t, x)
    outside = outside_bar(x, ref, total)
    assert outside.tolist() == sorted(named), outside[:10]


@pytest.mark.parametrize("case", ["example", "layers"])
def test_device_api(made, math, case):
    """Stepping::trip() and step() under a view: the bits of traverse_n"""
    pos, d = CO.sight(case, 500)
    ref = both_forms(made(case)["stepper"], math, pos, d, CO.CEILING, f"{case} {math}",
                     max_steps=CO.SIGHT_MAX_STEPS)
    assert (ref["n_crossings"] > 1).sum() > 250


# ---- step, walk and scatter -------------------------------------------------------------------

@pytest.mark.parametrize("case", ["layers", "example"])
def test_step_walk_and_scatter(made, math, case):
    """test_gpu_irregular.test_step_walk_and_scatter's body and bars: 512 rays, 48 generations of
    isotropic directions.  step_n with the sample handed back against the restatement's single
    steps, generation by generation; walk_n the bits of that loop; scatter_n that loop -- bit for
    bit in STRICT; in FAST the same media and step counts, positions and lengths within 1e-6 m --
    and the restatement's loop.  Flats have no rim and an optimistic step never crosses a flat: no
    ray leaves here and hardly one changes medium; what forks is the data under each walker, which
    sets the length of its every step."""
    s = made(case)
    st, geo = s["stepper"], s["geo"]
    K, seed, first = CO.WALK_GENERATIONS, 777, 5
    lat, lon, height = CO.walk_origins(case)
    pos, di = st.position(lat, lon, height)
    assert (di >= 0).all()
    n = pos.shape[0]
    _, below = geo.position(lat, lon, 0.0, layer=CO.COMPOSITE_LAYER[case])
    # (the UTM map covers 3 % of "example"'s box: some 16 of the 512 walkers)
    assert all((below == k).sum() >= 10 for k in ((-1, 0, 1) if case == "layers" else (0, 1, 2)))

    state = st.step(pos.copy(), None)
    walk = st.walk(pos.copy())
    assert np.array_equal(state["index"], walk["index"]) and np.array_equal(state["step"], walk["next"])
    o = geo.step(pos)
    assert np.array_equal(state["index"], o["index"])
    ref_pos, alive = pos.copy(), o["index"][:, 0] >= 0
    total, moved = np.zeros(n), np.zeros(n, dtype=np.int32)
    ref_total, ref_steps = np.zeros(n), np.zeros(n, dtype=np.int32)
    for k in range(K):
        inside = state["index"][:, 0] >= 0
        d = TA.isotropic(n, seed, k, first_ray=first, device=False)
        state = st.step(state["position"], d, resume=state)
        walk = st.walk(None, d, state=walk)
        for name in ("position", "index", "step"):
            assert np.array_equal(walk[name], state[name]), (k, name)
        moved += inside
        total += np.where(inside, state["step"], 0.0)
        assert np.array_equal(inside, alive), k
        o = geo.step(ref_pos, d)
        same = (state["index"][alive] == o["index"][alive]).all(axis=1)
        assert same.all(), (k, np.flatnonzero(alive)[~same][:10])
        ok = alive & (o["index"][:, 0] >= 0)
        assert np.abs(state["step"][ok] - o["step"][ok]).max() <= max(1e-6 * o["step"][ok].max(), 1e-7)
        assert np.abs(state["position"][alive] - o["position"][alive]).max() < 1e-6
        ref_pos = np.where(alive[:, None], o["position"], ref_pos)
        ref_total += np.where(alive, o["step"], 0.0)
        ref_steps += alive
        alive = alive & (o["index"][:, 0] >= 0)
    assert alive.all()

    w = st.scatter(pos.copy(), seed, K, first_ray=first)
    assert st.trace_stats()["steps"] == int(w["steps"].sum())
    if math == "strict":
        assert np.array_equal(w["position"], state["position"]) and np.array_equal(w["index"], state["index"])
        assert np.array_equal(w["steps"], moved) and np.array_equal(w["length"], total)
    else:
        assert np.array_equal(w["index"][:, 0], state["index"][:, 0]) and np.array_equal(w["steps"], moved)
        assert np.abs(w["position"] - state["position"]).max() < 1e-6
        assert np.abs(w["length"] - total).max() < 1e-6
    assert np.array_equal(w["index"][:, 0], o["index"][:, 0]) and np.array_equal(w["steps"], ref_steps)
    assert np.abs(w["position"] - ref_pos).max() < 1e-5
    assert (np.abs(w["length"] - ref_total) / np.maximum(ref_total, 1e-300)).max() <= 1e-6


# ---- paged ------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", [1, 2])
@pytest.mark.parametrize("case", ["layers", "offsets"])
def test_paged(made, math, case, size, tmp_path):
    """the stack with room for 1 or 2 of its 3 tiles inside the composite geometry -- the CAN_PAGE
    instances of k_trace, k_cross and k_traverse for GENERIC -- against every tile resident, at
    test_gpu_irregular.test_paged's bars: STRICT the same bits; FAST the same media and step
    counts, lengths within 1e-9 (a ray that waited goes on along a new line), traverse within its
    bar; single steps the same bits."""
    s = made(case)
    sf = s["stepper"]
    pos, d = s["graze"][0][:300], s["graze"][1][:300]
    paged = CO.amd_geometry(case, tmp_path, stack_size=size)
    sp, stack = paged["stepper"], paged["stack"]
    try:
        t0 = sf.trace(pos.copy(), d, max_steps=CO.GRAZE_MAX_STEPS)
        stack.clear()
        t1 = sp.trace(pos.copy(), d, max_steps=CO.GRAZE_MAX_STEPS)
        assert sp.rounds > 1 and stack.resident <= size
        stats = sp.trace_stats()
        assert stats["rays"] == pos.shape[0] and stats["steps"] == int(t1["n_steps"].sum())
        assert np.array_equal(t0["index"], t1["index"]) and np.array_equal(t0["n_steps"], t1["n_steps"])
        if math == "strict":
            assert np.array_equal(t0["length"], t1["length"]) and np.array_equal(t0["position"], t1["position"])
        else:
            rel = np.abs(t0["length"] - t1["length"]) / np.maximum(t0["length"], 1e-300)
            assert rel.max() < 1e-9 and np.abs(t0["position"] - t1["position"]).max() < 1e-5
        spos, sd = CO.sight(case, 300)
        v0 = sf.traverse(spos.copy(), sd, CO.CEILING, max_steps=CO.SIGHT_MAX_STEPS)
        stack.clear()
        v1 = sp.traverse(spos.copy(), sd, CO.CEILING, max_steps=CO.SIGHT_MAX_STEPS)
        assert sp.rounds > 1 and stack.resident <= size
        if math == "strict":
            same_bits(v0, v1)
        else:
            assert_bar(v1, v0, f"paged {case} {size}")
        stack.clear()
        a, b = sf.step(pos.copy(), None), sp.step(pos.copy(), None)
        for k in ("index", "altitude", "elevation"):
            assert np.array_equal(a[k], b[k]), k
        for gen in range(12):
            di = TA.isotropic(pos.shape[0], 11, gen, 0, device=False)
            a = sf.step(a["position"], di, resume=a)
            b = sp.step(b["position"], di, resume=b)
            for k in ("index", "position", "step", "altitude", "elevation"):
                assert np.array_equal(a[k], b[k]), (gen, k)
            assert stack.resident <= size
    finally:
        CO.destroy(paged)


# ---- the hand-over ----------------------------------------------------------------------------

def test_hand_over_step_moves_no_result(tmp_path):
    """test_gpu_properties.test_hand_over_step_moves_no_result for GENERIC, at its bar: "layers" /
    "graze" with the hand-over never (0: one phase), at step 32, 512 (the default for a layered
    geometry) and 2048 ends in the same media, path lengths agree to 1e-7, and no ray takes another
    step count."""
    here = os.path.dirname(os.path.abspath(__file__))
    results = {}
    for park in ("0", "32", "512", "2048"):
        out = os.path.join(tmp_path, f"park{park}.npz")
        env = dict(os.environ, TURTLE_AMD_PARK=park)
        subprocess.run([sys.executable, os.path.join(here, "composite_probe.py"), out,
                        os.path.join(tmp_path, f"work{park}")], check=True, env=env, timeout=300)
        results[park] = dict(np.load(out))
    base = results["0"]
    assert (base["fast_n_steps"] > 2048).sum() > 100
    for park, r in results.items():
        for tag in ("fast", "strict"):
            assert np.array_equal(r[f"{tag}_index"], base[f"{tag}_index"]), (park, tag)
            rel = np.abs(r[f"{tag}_length"] - base[f"{tag}_length"]) / np.maximum(base[f"{tag}_length"], 1.0)
            assert rel.max() < 1e-7, (park, tag, rel.max())
            moved = int((r[f"{tag}_n_steps"] != base[f"{tag}_n_steps"]).sum())
            print(f"hand-over at {park}, {tag}: {moved} of {base[f'{tag}_n_steps'].size} rays take another step count")
            assert moved <= HAND_OVER_MOVED, (park, tag, moved)


# ---- no lid -----------------------------------------------------------------------------------

def test_a_flat_world_has_no_end(made, math):
    """"example" without its lid: a ray above the ground climbs for ever in steps that grow, to the
    cap of 3 000 steps, and some overflow to NaN on the way.  The same index pair and step count
    as the restatement, finite where it is finite, and the finite lengths within 1e-6
    (test_degenerate_inputs' form).  Rays CO.OPEN_LEFT_OUT overflow around the cap: left out."""
    s = made("example_open")
    pos, d = s["graze"][0][:CO.OPEN_RAYS], s["graze"][1][:CO.OPEN_RAYS]
    keep = np.setdiff1d(np.arange(CO.OPEN_RAYS), CO.OPEN_LEFT_OUT)
    ref = s["geo"].trace(pos, d, max_steps=CO.OPEN_MAX_STEPS, threads=8)
    t = s["stepper"].trace(pos.copy(), d, max_steps=CO.OPEN_MAX_STEPS)
    assert (ref["n_steps"] == CO.OPEN_MAX_STEPS).sum() > 50 and (~np.isfinite(ref["length"])).sum() > 20
    assert np.array_equal(t["index"][keep], ref["index"][keep])
    assert np.array_equal(np.asarray(t["n_steps"])[keep], ref["n_steps"][keep])
    L, L0 = np.asarray(t["length"])[keep], ref["length"][keep]
    assert np.array_equal(np.isfinite(L), np.isfinite(L0))
    ok = np.isfinite(L0)
    assert (np.abs(L[ok] - L0[ok]) <= 1e-6 * np.maximum(np.abs(L0[ok]), 1e-300)).all()
