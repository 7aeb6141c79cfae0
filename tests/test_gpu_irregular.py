"""The stepping kernels over irregular tile stacks (tests/irregular_cases.py), against the CPU
restatement, itself pinned on these stacks to the reference (tests/test_irregular_host.py).

tamd_stepper_flatten calls a stack regular when its resident tiles share one shape and encoding, sit
on the directory's lattice and the directory has at most 254 slots; the lookups, k_trace, k_walk,
k_step_fast, k_traverse and k_cross fork on that.  The stacks here, by the criterion that makes them
irregular:
  mixed       .asc: tile shape, and z0 / dz (an .asc tile's own range)     twin (int16): shape only
  slots255    .asc: 255 slots, and z0 / dz                                 twin: the count only
  slots254    .asc: z0 / dz only                                           twin: REGULAR (254 slots)
  slots256    .asc: 256 slots, and z0 / dz
slots254's twin and slots255's pin the slot << 24 | cell id limit from both sides.

The bars are those of the regular stacks' tests, named at each test; no ray is set apart."""
import numpy as np
import pytest

import turtle_amd as TA
from oracle import ffi as O

import crossings_cases as CC
import irregular_cases as IC
import traverse_cases as TC
from test_gpu_crossings import outside_bar
from test_gpu_parity import check_trace
from test_gpu_traverse import assert_bar, same_bits

pytestmark = pytest.mark.gpu

KEYS = [(case, False) for case in IC.CASES] + [(case, True) for case in IC.TWINS]
IDS = [case + ("_int16" if twin else "") for case, twin in KEYS]
MIXED = [("mixed", False), ("mixed", True)]
WALKS = [("mixed", False), ("mixed", True), ("slots255", False), ("slots255", True),
         ("slots254", True)]        # (the last one is regular: what this test found holds there too)


def ids(keys):
    return [IDS[KEYS.index(k)] for k in keys]


@pytest.fixture(params=["fast", "strict"])
def math(request):
    TA.set_math(request.param)
    yield request.param
    TA.set_math("fast")


@pytest.fixture(scope="module")
def stacks(tmp_path_factory):
    """key -> dict(dir, stack (every tile resident), stepper, geo (the restatement), pos, dir_, ref)"""
    made = {}

    def get(key):
        if key not in made:
            case, twin = key
            d = tmp_path_factory.mktemp(IDS[KEYS.index(key)])
            path = (IC.write_twin if twin else IC.write_asc)(d / "tiles", case)
            stack = TA.Stack(path, 0)
            stack.load()
            assert stack.resident == len(IC.DIRECTORIES[case][3])
            st = TA.Stepper()
            st.add_stack(stack, 0.0)
            geo = IC.oracle_geometry(case, twin)
            pos, dire = IC.rays(case)
            ref = geo.trace(pos, dire, max_steps=IC.MAX_STEPS, threads=8)
            made[key] = dict(path=path, stack=stack, stepper=st, geo=geo, pos=pos, dir=dire, ref=ref)
        return made[key]

    yield get
    for s in made.values():
        s["stepper"].destroy()
        s["stack"].destroy()


# ---- lookups ----------------------------------------------------------------------------

@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_lookups(stacks, golden, key):
    """Stack.elevation and inside: the restatement's bits.  Stack.gradient: the reference's bits
    (irregular.npz; for the int16 twins the restatement's, which that file pins).
    Stepper.position: within 5e-9 m (OCML's sin and cos against glibc's), the same data index."""
    case, twin = key
    s = stacks(key)
    lat, lon = IC.lookup_points(case)
    z, inside = s["stack"].elevation(lat, lon)
    z0, in0 = s["geo"].stack_elevation(0, lat, lon)
    assert np.array_equal(inside, in0) and np.array_equal(z, z0)
    assert 0.5 * lat.size < in0.sum() < 0.95 * lat.size
    glat, glon, gin = s["stack"].gradient(lat, lon)
    if twin:
        glat0, glon0, gin0 = IC.stack_gradient(s["geo"], case, lat, lon)
    else:
        g = golden("irregular")
        assert IC.sha(np.stack([lat, lon])) == str(g[f"{case}_points_sha"])
        glat0, glon0, gin0 = g[f"{case}_glat"], g[f"{case}_glon"], g[f"{case}_inside"].astype(np.int32)
        assert np.array_equal(z0, g[f"{case}_z"])
    assert np.array_equal(gin, gin0)
    assert np.array_equal(glat, glat0) and np.array_equal(glon, glon0)
    for mode in ("fast", "strict"):
        TA.set_math(mode)
        try:
            pos, di = s["stepper"].position(lat, lon, 100.0)
        finally:
            TA.set_math("fast")
        pos0, di0 = s["geo"].position(lat, lon, 100.0)
        assert np.array_equal(di, di0) and np.array_equal(di0 == 0, in0 == 1)
        assert np.abs(pos - pos0)[di0 == 0].max() < 5e-9


# ---- trace ------------------------------------------------------------------------------

@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_trace(stacks, math, key):
    """2 000 rays a stack against the restatement, no ray allowed for: identical medium, path
    length within 1e-6, step counts within check_trace's own allowance.  slots254's twin is the
    regular neighbour of slots255's: the id limit from both sides."""
    case, twin = key
    s = stacks(key)
    ref, n = s["ref"], s["pos"].shape[0]
    # the batch is not trivial (from the restatement alone)
    assert (ref["n_steps"] < IC.MAX_STEPS).all()
    assert (ref["index"][:, 0] == -1).sum() > 0.15 * n            # rays leave the mosaic
    assert (ref["index"][:, 0] == 0).sum() > 0.40 * n             # rays hit the ground
    assert ref["n_steps"].max() > 2000
    if case in ("slots255", "slots256"):
        lat, lon, _ = O.ecef_to_geodetic(ref["position"])
        assert (IC.slot_of(case, lat, lon) >= 250).sum() > 0      # ends beyond slot 250
    t = s["stepper"].trace(s["pos"].copy(), s["dir"], max_steps=IC.MAX_STEPS)
    L, L0 = np.asarray(t["length"]), ref["length"]
    print(f"\n[{IDS[KEYS.index(key)]} {math}] {int((t['index'][:, 0] != ref['index'][:, 0]).sum())} media differ, "
          f"worst |dL|/L {np.max(np.abs(L - L0) / np.maximum(L0, 1e-300)):.3e}, "
          f"{int((t['n_steps'] != ref['n_steps']).sum())} step counts differ")
    check_trace(t, ref["index"], ref["length"], ref["n_steps"], f"{key} {math}", allow=0)
    assert np.array_equal(t["index"], ref["index"])
    stats = s["stepper"].trace_stats()
    assert stats["rays"] == n and stats["steps"] == int(t["n_steps"].sum()) and stats["capped"] == 0


@pytest.mark.parametrize("key", MIXED, ids=ids(MIXED))
def test_odd_batch_sizes(stacks, math, key):
    """the first 1, 63, 65 and 257 rays alone: the bits they get in the whole batch"""
    s = stacks(key)
    whole = s["stepper"].trace(s["pos"].copy(), s["dir"], max_steps=IC.MAX_STEPS)
    for n in (1, 63, 65, 257):
        t = s["stepper"].trace(s["pos"][:n].copy(), s["dir"][:n], max_steps=IC.MAX_STEPS)
        for k in ("index", "length", "n_steps", "position"):
            assert np.array_equal(t[k], whole[k][:n]), (n, k)


# ---- the rim, the seams and the hole ------------------------------------------------------

@pytest.mark.parametrize("key", MIXED, ids=ids(MIXED))
def test_rim_seams_and_the_hole(stacks, math, key):
    """test_gpu_parity.test_stack_rim_and_seams over "mixed": fresh samples 1e-12 .. 1e-4 degree
    either side of every line of the lattice -- the rim, the seams between tiles of 9, 17, 33, 5
    and 3 nodes a side, the four edges of the missing tile -- and the corners; then one step from
    each.  The same index, the elevation within 1e-9 m, the step within 1e-6."""
    s = stacks(key)
    st, geo = s["stepper"], s["geo"]
    lat, lon = IC.edge_points(key[0])
    pos = O.ecef_from_geodetic(lat, lon, np.full(lat.size, 2500.0))
    mine = st.step(pos.copy(), None)
    ref = geo.step(pos)
    assert np.array_equal(mine["index"], ref["index"])
    inside = ref["index"][:, 0] >= 0
    assert inside.sum() > 0.4 * lat.size and (~inside).sum() > 0.2 * lat.size
    assert np.abs(mine["elevation"][inside] - ref["elevation"][inside]).max() < 1e-9
    d = TA.isotropic(lat.size, 7, 0, device=False)
    mine2 = st.step(mine["position"], d, resume=mine)
    ref2 = geo.step(ref["position"], d)
    same = mine2["index"][:, 0] == ref2["index"][:, 0]
    assert (~same).sum() == 0, np.flatnonzero(~same)[:10]
    ok = same & (ref2["index"][:, 0] >= 0)
    assert np.abs(mine2["step"][ok] - ref2["step"][ok]).max() < 1e-6 * ref2["step"][ok].max()


# ---- step, walk and scatter ---------------------------------------------------------------

@pytest.mark.parametrize("key", WALKS, ids=ids(WALKS))
def test_step_walk_and_scatter(stacks, math, key):
    """512 rays, 48 generations of isotropic directions (the library's Philox).  step_n with the
    sample handed back against the restatement's single steps, generation by generation (the bar of
    test_scattering_walk_against_oracle); walk_n the bits of that loop (test_walk_n_is_the_step_loop_
    with_less_state); scatter_n that loop -- bit for bit in STRICT; in FAST the same media and step
    counts, positions and lengths within 1e-6 m (test_scatter_n_is_the_step_loop) -- and the
    restatement's loop (test_scatter_over_a_stack_against_the_oracle).

    A ray that has left stays out: step_n and walk_n used to sample it afresh, 1e-8 m from the rim,
    and in FAST one in ten came back in by an ulp of the transform (a quarter of the rays start at
    30 km and leave in 10 km steps; then they are dead for most of the walk)."""
    case, _ = key
    s = stacks(key)
    st, geo = s["stepper"], s["geo"]
    n, K, seed, first = 512, 48, 777, 5
    (south, north), (west, east) = IC.box(case)
    rng = np.random.default_rng(21)
    lat, lon = rng.uniform(south, north, n), rng.uniform(west, east, n)
    height = np.where(np.arange(n) % 4 == 0, 30000.0, 60.0)       # the high ones take 10 km steps: they leave
    pos, di = st.position(lat, lon, height)
    pos = np.ascontiguousarray(pos[di == 0])
    n = pos.shape[0]
    assert n > 400

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
        # the restatement samples every start afresh; a ray that has left stays where it is
        assert np.array_equal(inside, alive), k
        o = geo.step(ref_pos, d)
        same = state["index"][alive, 0] == o["index"][alive, 0]
        assert same.all(), (k, np.flatnonzero(alive)[~same][:10])
        ok = alive & (o["index"][:, 0] >= 0)
        assert np.abs(state["step"][ok] - o["step"][ok]).max() <= max(1e-6 * o["step"][ok].max(), 1e-7)
        assert np.abs(state["position"][alive] - o["position"][alive]).max() < 1e-6
        ref_pos = np.where(alive[:, None], o["position"], ref_pos)
        ref_total += np.where(alive, o["step"], 0.0)
        ref_steps += alive
        alive = alive & (o["index"][:, 0] >= 0)
    assert (ref_steps < K).sum() > 20                              # rays did leave: the hole, the rim

    w = st.scatter(pos.copy(), seed, K, first_ray=first)
    assert st.trace_stats()["steps"] == int(w["steps"].sum())
    if math == "strict":
        assert np.array_equal(w["position"], state["position"]) and np.array_equal(w["index"], state["index"])
        assert np.array_equal(w["steps"], moved) and np.array_equal(w["length"], total)
    else:
        assert np.array_equal(w["index"][:, 0], state["index"][:, 0]) and np.array_equal(w["steps"], moved)
        assert np.abs(w["position"] - state["position"]).max() < 1e-6
        assert np.abs(w["length"] - total).max() < 1e-6
    ref_medium = np.where(alive, o["index"][:, 0], -1)
    assert np.array_equal(w["index"][:, 0], ref_medium) and np.array_equal(w["steps"], ref_steps)
    assert np.abs(w["position"] - ref_pos).max() < 1e-5
    assert (np.abs(w["length"] - ref_total) / np.maximum(ref_total, 1e-300)).max() <= 1e-6


# ---- traverse and crossings ---------------------------------------------------------------

@pytest.mark.parametrize("key", MIXED, ids=ids(MIXED))
def test_traverse_and_crossings(stacks, math, key):
    """lines of sight up to 5 000 m over "mixed" against the loops of traverse_cases and
    crossings_cases over the restatement, at their bars with no ray named: the same final index
    pair, crossing and step counts, every per-medium length, crossing distance and point within 1e-6
    of the ray's path; crossings_n's shared outputs are the bits of traverse_n."""
    s = stacks(key)
    st, geo, pos, d = s["stepper"], s["geo"], s["pos"], s["dir"]
    ref = CC.check(geo, pos, d, IC.CEILING, threads=8)
    same_bits(TC.check(geo, pos, d, IC.CEILING, threads=8), ref, ("index", "length", "n_steps", "n_crossings"))
    assert (ref["n_crossings"] > 1).sum() > 100 and (ref["index"][:, 0] == -1).sum() > 100
    t = st.traverse(pos.copy(), d, IC.CEILING)
    assert_bar(t, ref, f"{key} {math}")
    capacity = int(ref["n_crossings"].max()) + 1
    x = st.crossings(pos.copy(), d, IC.CEILING, capacity=capacity)
    same_bits(t, x)
    outside = outside_bar(x, ref, ref["length"].sum(axis=0))
    assert outside.size == 0, outside[:10]


# ---- paged ----------------------------------------------------------------------------------

@pytest.mark.parametrize("size", [2, 3])
@pytest.mark.parametrize("key", MIXED, ids=ids(MIXED))
def test_paged(stacks, math, key, size):
    """"mixed" with room for 2 or 3 of its 8 tiles against the same stack with every tile resident,
    as test_gpu_paging and test_traverse_paged_stack assert it for regular stacks: STRICT the same
    bits; FAST the same media and step counts, lengths within 1e-9 (a ray that waited goes on along
    a new line), traverse within its bar; single steps the same bits.

    `regular` is decided from the RESIDENT tiles: each batch starts with only the two tiles of 9
    nodes a side in memory and its rays over those tiles first, so that the first flattening sees
    one shape (a regular stack, for the int16 twin) and tiles of other shapes page in afterwards."""
    case, _ = key
    s = stacks(key)
    sf, pos, d = s["stepper"], s["pos"], s["dir"]
    tiles = IC.DIRECTORIES[case][3]
    nine = [iy * 3 + ix for (iy, ix), (n, _) in tiles.items() if n == 9]
    assert len(nine) == 2
    lat, lon, _ = O.ecef_to_geodetic(pos)
    first = np.isin(IC.slot_of(case, lat, lon), nine)
    # 300 rays that start over the tiles of 9 nodes, then 300 that start elsewhere
    order = np.concatenate([np.flatnonzero(first)[:300], np.flatnonzero(~first)[:300]])
    pos, d = np.ascontiguousarray(pos[order]), np.ascontiguousarray(d[order])
    assert order.size == 600
    warm_lat = np.array([0.5, 1.5])                               # inside tiles (0, 0) and (1, 2)
    warm_lon = np.array([10.5, 12.5])

    paged = TA.Stack(s["path"], size)
    sp = TA.Stepper()
    sp.add_stack(paged, 0.0)

    def warm():
        paged.clear()
        z, inside = paged.elevation(warm_lat, warm_lon)
        assert inside.all() and paged.resident == 2

    try:
        warm()
        t0 = sf.trace(pos.copy(), d, max_steps=IC.MAX_STEPS)
        t1 = sp.trace(pos.copy(), d, max_steps=IC.MAX_STEPS)
        assert sp.rounds > 1 and paged.resident <= size
        stats = sp.trace_stats()
        assert stats["rays"] == pos.shape[0] and stats["steps"] == int(t1["n_steps"].sum())
        assert np.array_equal(t0["index"], t1["index"]) and np.array_equal(t0["n_steps"], t1["n_steps"])
        if math == "strict":
            assert np.array_equal(t0["length"], t1["length"]) and np.array_equal(t0["position"], t1["position"])
        else:
            rel = np.abs(t0["length"] - t1["length"]) / np.maximum(t0["length"], 1e-300)
            assert rel.max() < 1e-9 and np.abs(t0["position"] - t1["position"]).max() < 1e-5
        warm()
        v0 = sf.traverse(pos.copy(), d, IC.CEILING)
        v1 = sp.traverse(pos.copy(), d, IC.CEILING)
        assert sp.rounds > 1 and paged.resident <= size
        if math == "strict":
            same_bits(v0, v1)
        else:
            assert_bar(v1, v0, f"paged {key} {size}")
        warm()
        a, b = sf.step(pos.copy(), None), sp.step(pos.copy(), None)
        for k in ("index", "altitude", "elevation"):
            assert np.array_equal(a[k], b[k]), k
        for gen in range(12):
            di = TA.isotropic(pos.shape[0], 11, gen, 0, device=False)
            a = sf.step(a["position"], di, resume=a)
            b = sp.step(b["position"], di, resume=b)
            for k in ("index", "position", "step", "altitude", "elevation"):
                assert np.array_equal(a[k], b[k]), (gen, k)
            assert paged.resident <= size
    finally:
        sp.destroy()
        paged.destroy()
