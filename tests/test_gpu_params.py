"""The stepping kernels at slope and resolution other than the defaults (tests/params_cases.py):
against the reference's own traces (tests/golden/params.npz) and the CPU restatement and its loops,
which take both numbers as arguments.

The bar, in both arithmetics and with no allowance, for every ray the reference's arithmetic alone
does not set apart (params_cases.ill_conditioned, capped by tests/test_params_host.py): the same
index pair, the same step count, |dL| / L <= 1e-6.  One ray is named outside it
(params_cases.OUTSIDE)."""
import contextlib
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import turtle_amd as TA
from oracle import ffi as O
from turtle_amd import synth

import advance_cases as AC
import advance_exp_cases as AE
import amd_build as B
import composite_cases as CO
import crossings_cases as CC
import device_loops as DL
import params_cases as PC
import terrains as T
import traverse_cases as TC
from test_gpu_advance import off_the_bar, on_the_ray
from test_gpu_crossings import outside_bar
from test_gpu_traverse import assert_bar, same_bits

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
TRACE_KEYS = ("position", "index", "length", "n_steps")
OUTSIDE = PC.OUTSIDE      # the rays outside the bar, by name: see params_cases


@pytest.fixture(params=["fast", "strict"])
def math(request):
    TA.set_math(request.param)
    yield request.param
    TA.set_math("fast")


@contextlib.contextmanager
def at(st, name):
    """the stepper at a setting of the table; the defaults again afterwards"""
    st.slope, st.resolution = PC.SETTINGS[name]
    try:
        yield st
    finally:
        st.slope, st.resolution = PC.DEFAULT


@pytest.fixture(scope="module")
def steppers(tmp_path_factory):
    """the three geometries of traverse_cases, through the public API"""
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
    maps = dict(zip(TC.CASES, keep))
    yield dict(out, maps=maps)
    for st in out.values():
        st.destroy()
    for m in keep:
        m.destroy()


@pytest.fixture(scope="module")
def stacks(tmp_path_factory):
    """the 2 x 2 stack of 1201^2 tiles: resident, and with room for two tiles"""
    d = str(tmp_path_factory.mktemp("grid"))
    for la, lo in PC.STACK_TILES:
        synth.write_hgt(d, la, lo, TC.N)
    full, paged = TA.Stack(d, 0), TA.Stack(d, 2)
    full.load()
    out = {}
    for tag, stack in (("resident", full), ("paged", paged)):
        out[tag] = TA.Stepper()
        out[tag].add_stack(stack, 0.0)
    out["stack"] = paged
    yield out
    for o in (out["resident"], out["paged"], full, paged):
        o.destroy()


def trace_bar(t, ref, bad, what):
    """the bar for every ray outside the mask `bad`; returns the worst relative path-length difference"""
    L, L0 = np.asarray(t["length"]), ref["length"]
    with np.errstate(invalid="ignore"):
        rel = np.where(L0 == 0, np.abs(L), np.abs(L - L0) / np.maximum(np.abs(L0), 1e-300))
    wrong = (np.asarray(t["index"]) != ref["index"]).any(axis=1) | (np.asarray(t["n_steps"]) != ref["n_steps"])
    wrong = (wrong | ~(rel <= PC.BAR)) & ~bad
    ids = np.flatnonzero(wrong)
    named = sorted(OUTSIDE.get(what, ()))
    counted = ~bad
    counted[named] = False
    worst = float(rel[counted].max())
    print(f"\n[{what}] masked {int(bad.sum())} of {bad.size}, worst |dL|/L {worst:.3e}, beyond 32 steps "
          f"{int((ref['n_steps'] > 32).sum())}, beyond 512 {int((ref['n_steps'] > 512).sum())}")
    # even a named ray ends where the reference's does
    assert np.array_equal(np.asarray(t["index"])[named], ref["index"][named]), what
    assert ids.tolist() == named, \
        f"{what}: rays {ids[:10]}: |dL|/L {rel[ids[:10]]}, steps {np.asarray(t['n_steps'])[ids[:10]]} vs " \
        f"{ref['n_steps'][ids[:10]]}, index {np.asarray(t['index'])[ids[:10]].tolist()} vs " \
        f"{ref['index'][ids[:10]].tolist()}"
    return worst


def stats_agree(st, t):
    s = st.trace_stats()
    assert s["rays"] == t["index"].shape[0] and s["steps"] == int(np.asarray(t["n_steps"]).sum())
    assert s["capped"] == 0


# ---- trace_n --------------------------------------------------------------------------------

@pytest.mark.parametrize("case,name", [(case, name) for case in PC.CASES for name in PC.settings(case)])
def test_trace_matches_the_reference(steppers, golden, math, case, name):
    """the three recipes of params.npz in one batch of 3000 rays, against the reference's own
    index, length and step count (`steep` is not run on the rough tile: params_cases.settings)"""
    g = golden("params")
    pos = np.concatenate([g[f"{case}_{r}_position"] for r in PC.RECIPES])
    d = np.concatenate([g[f"{case}_{r}_direction"] for r in PC.RECIPES])
    ref = {k: np.concatenate([g[f"{case}_{r}_{name}_{k}"] for r in PC.RECIPES]) for k in ("index", "length", "n_steps")}
    ref["index"] = ref["index"].astype(np.int32)
    slope, resolution = PC.SETTINGS[name]
    bad, base = PC.trace_mask((case, name), TC.oracle_geometry(case), pos, d, slope, resolution)
    assert bad.sum() <= PC.cap(case, name) * bad.size
    assert all(np.array_equal(base[k], ref[k]) for k in ref)        # (the restatement is the reference)
    assert (ref["n_steps"] > 32).sum() > 50 and (case == "rough" or (ref["n_steps"] > 512).sum() > 10)
    with at(steppers[case], name) as st:
        t = st.trace(pos.copy(), d, max_steps=PC.MAX_STEPS)
        trace_bar(t, ref, bad, f"trace {case} {name} {math}")
        stats_agree(st, t)


@pytest.mark.parametrize("name", list(PC.SETTINGS))
@pytest.mark.parametrize("how", ["resident", "paged"])
def test_trace_over_a_stack(stacks, math, how, name):
    """fresh seeded rays over the 2 x 2 stack, every tile resident and with room for two (the rays
    page tiles in, round by round), against the restatement"""
    geo = PC.stack_oracle()
    pos, d = PC.stack_rays()
    slope, resolution = PC.SETTINGS[name]
    bad, ref = PC.trace_mask(("stack", name), geo, pos, d, slope, resolution)
    assert bad.sum() <= PC.cap("stack", name) * bad.size
    assert (ref["n_steps"] > 32).sum() > 50 and (ref["n_steps"] > 512).sum() > 10
    if how == "paged":
        stacks["stack"].clear()
    with at(stacks[how], name) as st:
        t = st.trace(pos.copy(), d, max_steps=PC.MAX_STEPS)
        trace_bar(t, ref, bad, f"trace stack {how} {name} {math}")
        stats_agree(st, t)
        if how == "paged":
            assert st.rounds > 1 and stacks["stack"].resident <= 2


SHIFT = 5e-9


@pytest.mark.parametrize("name", ["fine", "coarse", "mixed"])
@pytest.mark.parametrize("where", ["map", "stack"])
def test_a_resumed_trace_starts_with_the_resolution(steppers, stacks, golden, math, where, name):
    """A trace resumed ON a boundary (TURTLE_AMD_TRACE_RESUME): the rays of a batch that ended in the
    ground, from 5e-9 m BEFORE the reference's end point -- where a fresh sample still gives the air
    (checked with the restatement) -- with the index pair the first trace returned.  The medium
    handed in wins, and the first step has the length `resolution` [ref stepper.c:812-813]; the
    restatement continues from the end point itself, in the ground by its own sample and with a
    clearance below 1e-8 m, i.e. with the same first step.  The same index pair and step count, and
    the same path but for the 5e-9 m, at the bar."""
    slope, resolution = PC.SETTINGS[name]
    if where == "map":
        g = golden("params")
        geo, st = TC.oracle_geometry("hgt"), steppers["hgt"]
        pos, d = g["hgt_c2_position"], g["hgt_c2_direction"]
    else:
        geo, st = PC.stack_oracle(), stacks["resident"]
        pos, d = PC.stack_rays()
    first = geo.trace(pos, d, max_steps=PC.MAX_STEPS, slope=slope, resolution=resolution, threads=8)
    start = first["position"] - SHIFT * d
    hit = (first["index"][:, 0] == 0) & (geo.step(start)["index"][:, 0] == 1)
    hit &= geo.step(first["position"])["index"][:, 0] == 0
    assert hit.sum() > 400
    ref = geo.trace(first["position"][hit], d[hit], max_steps=PC.MAX_STEPS, slope=slope, resolution=resolution,
                    threads=8)
    assert (ref["n_steps"] < PC.MAX_STEPS).all() and (ref["n_steps"] > 32).sum() > 50
    with at(st, name):
        t = st.trace(start[hit].copy(), d[hit], max_steps=PC.MAX_STEPS, resume_index=first["index"][hit])
    t = dict(t, length=t["length"] - SHIFT)
    trace_bar(t, ref, np.zeros(int(hit.sum()), dtype=bool), f"resumed {where} {name} {math}")


# ---- the generic step machine ---------------------------------------------------------------

@pytest.fixture(scope="module")
def layers(tmp_path_factory):
    amd = CO.amd_geometry(PC.GENERIC_CASE, tmp_path_factory.mktemp("layers"))
    yield amd["stepper"], CO.oracle_geometry(PC.GENERIC_CASE)
    CO.destroy(amd)


def sight_bar(st, geo, pos, d, ceiling, slope, resolution, bad, what, max_steps=1000000):
    """traverse_n and crossings_n against their CPU checkers at their bars (test_gpu_traverse.assert_bar,
    test_gpu_crossings.outside_bar), minus the masked rays; returns (traverse's result, the checker's)"""
    ref = CC.check(geo, pos, d, ceiling, max_steps=max_steps, slope=slope, resolution=resolution)
    keep = np.flatnonzero(~bad)
    t = st.traverse(pos.copy(), d, ceiling, max_steps=max_steps)
    stats_agree(st, t)
    total = ref["length"].sum(axis=0)
    off = np.abs(t["length"] - ref["length"]).max(axis=0) / np.maximum(total, 1e-300)
    print(f"\n[{what}] masked {int(bad.sum())} of {bad.size}, worst per-medium |dL|/L {off[keep].max():.3e}, "
          f"{int((t['n_steps'] > 512).sum())} rays beyond 512 steps, crossings max {int(ref['n_crossings'].max())}")
    cut = lambda r: dict(index=r["index"][keep], length=r["length"][:, keep], n_steps=r["n_steps"][keep],
                         n_crossings=r["n_crossings"][keep])
    assert_bar(cut(t), cut(ref), what)
    x = st.crossings(pos.copy(), d, ceiling, max_steps=max_steps, capacity=int(ref["n_crossings"].max()) + 1)
    same_bits(t, x)
    outside = outside_bar(x, ref, total)
    assert np.setdiff1d(outside, np.flatnonzero(bad)).size == 0, (what, outside[:10])
    return t, ref


@pytest.mark.parametrize("name", PC.GENERIC_SETTINGS)
def test_the_generic_step_machine(layers, math, name):
    """composite_cases' "layers" (a geoid, a flat, a stack under a map, a lid): trace, traverse and
    crossings against the restatement and its loops"""
    st, geo = layers
    slope, resolution = PC.SETTINGS[name]
    pos, d, _ = CO.graze(PC.GENERIC_CASE, geo)
    bad, ref = PC.trace_mask(("generic", name), geo, pos, d, slope, resolution)
    assert bad.sum() <= 0.005 * bad.size and (ref["n_steps"] > 512).sum() > 300
    spos, sd = PC.generic_sight()
    sbad, _ = PC.traverse_mask(("generic sight", name), geo, spos, sd, CO.CEILING, slope, resolution,
                               max_steps=CO.SIGHT_MAX_STEPS)
    assert sbad.sum() <= 0.005 * sbad.size
    with at(st, name):
        t = st.trace(pos.copy(), d, max_steps=PC.MAX_STEPS)
        trace_bar(t, ref, bad, f"generic trace {name} {math}")
        stats_agree(st, t)
        sight_bar(st, geo, spos, sd, CO.CEILING, slope, resolution, sbad, f"generic sight {name} {math}",
                  max_steps=CO.SIGHT_MAX_STEPS)


# ---- traverse_n, crossings_n, advance_n, advance_exp_n --------------------------------------

def lines_of_sight(steppers, golden, math, case, recipe, name, shallow=False):
    geo = TC.oracle_geometry(case)
    pos, d, ceiling = PC.sight_rays(case, recipe, golden("traverse"), shallow=shallow)
    slope, resolution = PC.SETTINGS[name]
    key = ("two shallow", recipe, name) if shallow else (case, recipe, name)
    bad, _ = PC.traverse_mask(key, geo, pos, d, ceiling, slope, resolution)
    assert bad.sum() <= PC.cap(case, name) * bad.size
    keep = ~bad
    with at(steppers[case], name) as st:
        what = f"{case}{' (shallow)' if shallow else ''} {recipe} {name} {math}"
        t, ref = sight_bar(st, geo, pos, d, ceiling, slope, resolution, bad, "sight " + what)
        rho, sh = AC.DENSITY[st.media], AE.SCALE_HEIGHT[st.media]
        rng = np.random.default_rng([AC.SEED, zlib.crc32(f"{case} {recipe} {name}".encode())])
        b = AC.budgets(rng, ref["length"], ref["index"], ref["offset"], ref["distance"], ref["media"], rho)
        T_, D_ = ref["length"].sum(axis=0), (rho[:, None] * ref["length"]).sum(axis=0)
        for tag, scale in (("advance", None), ("advance_exp", sh)):
            if scale is None:
                want = AC.check(geo, pos, d, rho, b["budget"], b["distance_max"], ceiling, slope=slope,
                                resolution=resolution)
            else:
                want = AE.check(geo, pos, d, rho, scale, b["budget"], b["distance_max"], ceiling, slope=slope,
                                resolution=resolution)
            a = st.advance(pos.copy(), d, rho, b["budget"], b["distance_max"], ceiling, scale_height=scale)
            ids = np.setdiff1d(off_the_bar(a, want, D_, T_), np.flatnonzero(bad))
            print(f"[{tag} {what}] status counts {np.bincount(a['status'], minlength=5).tolist()}, distance off by "
                  f"{np.max(np.abs(a['distance'] - want['distance'])[keep] / np.maximum(T_[keep], 1e-300)):.2e} T")
            assert ids.size == 0, (tag, what, ids[:10], a["status"][ids[:10]], want["status"][ids[:10]],
                                   a["n_steps"][ids[:10]], want["n_steps"][ids[:10]])
            on_the_ray(a, pos, d, T_)
            spent, far = a["status"] == AC.SPENT, a["status"] == AC.DISTANCE
            assert spent.sum() > 20 and far.sum() > 20
            assert np.array_equal(a["depth"][spent], b["budget"][spent])
            assert np.array_equal(a["distance"][far], b["distance_max"][far])


@pytest.mark.parametrize("name", PC.SIGHT_SETTINGS)
@pytest.mark.parametrize("recipe", ["ground", "c2"])
@pytest.mark.parametrize("case", PC.SIGHT_CASES)
def test_lines_of_sight(steppers, golden, math, case, recipe, name):
    """traverse_n and crossings_n at the bars of their own test files; advance_n and advance_exp_n
    with budgets and distance limits drawn by advance_cases.budgets from this batch's own traverse
    and crossings at this setting, at test_gpu_advance's bar"""
    lines_of_sight(steppers, golden, math, case, recipe, name)


@pytest.mark.parametrize("name", PC.SHALLOW_SETTINGS)
@pytest.mark.parametrize("recipe", ["ground", "c2"])
def test_shallow_lines_of_sight_over_flat_layers(steppers, golden, math, recipe, name):
    """the same over traverse.npz's own "two" rays -- shallow rays that climb to the ceiling over flat
    layers, up to 11 crossings -- at the settings where the reference alone keeps them under the
    mask's cap (params_cases.SHALLOW_SETTINGS)"""
    lines_of_sight(steppers, golden, math, "two", recipe, name, shallow=True)


# ---- step_n, walk_n, scatter_n --------------------------------------------------------------

@pytest.mark.parametrize("name", ["example", "coarse"])
def test_step_walk_and_scatter(math, name):
    """test_scattering_walk_against_oracle's loop in small (1000 rays, 20 generations of isotropic
    directions): step_n with the sample handed back against the restatement's single steps; walk_n
    the bits of that loop; scatter_n the bits of it in STRICT (FAST: the same media and step counts,
    positions and lengths within 1e-6 m, as test_scatter_n_is_the_step_loop holds it)"""
    geo = T.c1_oracle()
    m = B.c1_map()
    st = B.c1_stepper(m)
    slope, resolution = PC.SETTINGS[name]
    st.slope, st.resolution = slope, resolution
    try:
        n, K, seed, first = 1000, 20, 99, 3
        lat, lon, _, _ = synth.uniform_rays(n, T.C1_Y, T.C1_X, seed=55)
        pos, _ = st.position(lat, lon, 30.0)
        ref_pos = pos.copy()
        state = st.step(pos.copy(), None)
        walk = st.walk(pos.copy())
        assert np.array_equal(state["index"], walk["index"]) and np.array_equal(state["step"], walk["next"])
        total, moved, flips = np.zeros(n), np.zeros(n, dtype=np.int32), 0
        for k in range(K):
            inside = state["index"][:, 0] >= 0
            d = TA.isotropic(n, seed, k, first_ray=first, device=False)
            state = st.step(state["position"], d, resume=state)
            walk = st.walk(None, d, state=walk)
            for key in ("position", "index", "step"):
                assert np.array_equal(walk[key], state[key]), (k, key)
            moved += inside
            total += np.where(inside, state["step"], 0.0)
            o = geo.step(ref_pos, d, slope=slope, resolution=resolution)
            ref_pos = o["position"]
            same = state["index"][:, 0] == o["index"][:, 0]
            flips += int((~same).sum())
            ok = same & (o["index"][:, 0] >= 0)
            assert np.abs(state["step"][ok] - o["step"][ok]).max() <= max(1e-6 * o["step"][ok].max(), 1e-7)
            assert np.abs(state["position"][same] - ref_pos[same]).max() < 1e-6
            if flips:
                break
        assert flips == 0, flips
        w = st.scatter(pos.copy(), seed, K, first_ray=first)
        assert st.trace_stats()["steps"] == int(w["steps"].sum())
        if math == "strict":
            for key, other in (("position", state["position"]), ("index", state["index"]), ("steps", moved),
                               ("length", total)):
                assert np.array_equal(w[key], other), key
        else:
            assert np.array_equal(w["index"][:, 0], state["index"][:, 0]) and np.array_equal(w["steps"], moved)
            assert np.abs(w["position"] - state["position"]).max() < 1e-6
            assert np.abs(w["length"] - total).max() < 1e-6
        assert (moved == K).sum() > n // 2
    finally:
        st.destroy()
        m.destroy()


# ---- the device API -------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["example", "coarse"])
def test_the_view_carries_the_settings(steppers, golden, math, name):
    """Stepping::trip() and step() in the caller's own kernel give the bits of traverse_n, and the
    caller's scattering walk those of scatter_n and of the walk_n loop over the same directions, in
    both arithmetics, at the setting of the stepper the view was acquired from"""
    g = golden("params")
    pos, d = g["hgt_c2_position"], g["hgt_c2_direction"]
    with at(steppers["hgt"], name) as st:
        ref = st.traverse(pos.copy(), d, 2000.0)
        K = 20
        start = g["hgt_graze_position"]
        sc = st.scatter(start.copy(), 4242, K, first_ray=17)
        o = st.step(start.copy(), None)
        begin = dict(position=start.copy(), altitude=o["altitude"], elevation=o["elevation"], index=o["index"],
                     length=np.zeros(start.shape[0]), steps=np.zeros(start.shape[0], dtype=np.int32))
        w, total = st.walk(start.copy()), np.zeros(start.shape[0])
        for k in range(K):
            inside = w["index"][:, 0] >= 0
            w = st.walk(None, TA.isotropic(start.shape[0], 4242, k, first_ray=17, device=False), state=w)
            total += np.where(inside, w["step"], 0.0)
        with st.view() as v:
            same_bits(DL.traverse(v, math, pos, d, 2000.0, 1000000, st.media), ref)
            same_bits(DL.traverse(v, math, pos, d, 2000.0, 1000000, st.media, simple=1), ref)
            got = DL.walk(v, math, begin, 4242, K, first_ray=17)
    st = steppers["hgt"]
    other = st.traverse(pos.copy(), d, 2000.0)        # the defaults again: another answer
    assert not np.array_equal(other["n_steps"], ref["n_steps"])
    for key in ("position", "index", "length", "steps"):        # both arithmetics
        assert np.array_equal(got[key], sc[key]), key
    for key, other in (("position", w["position"]), ("index", w["index"]), ("length", total)):
        assert np.array_equal(got[key], other), ("the walk_n loop", key)
    assert (sc["steps"] == K).sum() > start.shape[0] // 2


# ---- settings are state, and per stepper ------------------------------------------------------

def equal_traces(a, b, what=""):
    for k in TRACE_KEYS:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (what, k)


def test_settings_are_state(steppers, golden, math):
    """a setting made after a trace reaches the device, and setting it back restores every bit; a
    clone carries the settings it was made with"""
    g = golden("params")
    pos = np.concatenate([g[f"hgt_{r}_position"] for r in PC.RECIPES])
    d = np.concatenate([g[f"hgt_{r}_direction"] for r in PC.RECIPES])
    st = steppers["hgt"]
    assert (st.slope, st.resolution) == PC.DEFAULT
    fresh, clone = TA.Stepper(), None
    try:
        first = st.trace(pos.copy(), d)
        with at(st, "mixed"):
            assert (st.slope, st.resolution) == PC.SETTINGS["mixed"]
            second = st.trace(pos.copy(), d)
            clone = st.clone()
        third = st.trace(pos.copy(), d)
        fresh.slope, fresh.resolution = PC.SETTINGS["mixed"]
        fresh.add_map(steppers["maps"]["hgt"], 0.0)
        equal_traces(first, third, "the defaults, before and after")
        equal_traces(second, fresh.trace(pos.copy(), d), "mixed: set later, set first")
        assert not np.array_equal(first["n_steps"], second["n_steps"])
        assert (clone.slope, clone.resolution) == PC.SETTINGS["mixed"]
        equal_traces(second, clone.trace(pos.copy(), d), "the clone")
        clone.slope, clone.resolution = PC.DEFAULT      # ... and has settings of its own from then on
        equal_traces(first, clone.trace(pos.copy(), d), "the clone at the defaults")
        equal_traces(third, st.trace(pos.copy(), d), "the original after the clone changed")
    finally:
        fresh.destroy()
        if clone is not None:
            clone.destroy()


def test_two_steppers_at_two_settings_in_flight(steppers, golden, math):
    """two steppers over one map, at `example` and at `coarse`, each on a stream of its own and taking
    batches in turn (test_two_batches_in_flight_give_the_same_bits): each gives its own bits"""
    import torch
    g = golden("params")
    pos = np.concatenate([g[f"hgt_{r}_position"] for r in PC.RECIPES])
    d = np.concatenate([g[f"hgt_{r}_direction"] for r in PC.RECIPES])
    names = ("example", "coarse")
    refs = []
    for name in names:
        with at(steppers["hgt"], name) as st:
            refs.append(st.trace(pos.copy(), d))
    assert not np.array_equal(refs[0]["n_steps"], refs[1]["n_steps"])
    dev = torch.device("cuda", 0)
    pos0, dd = torch.as_tensor(pos, device=dev), torch.as_tensor(d, device=dev)
    pair, streams = [], []
    try:
        for name in names:
            st = TA.Stepper()
            st.add_map(steppers["maps"]["hgt"], 0.0)
            st.slope, st.resolution = PC.SETTINGS[name]
            pair.append(st)
            streams.append(torch.cuda.Stream(device=dev))
        torch.cuda.synchronize()
        TA.set_in_flight(2)
        outs, bufs = [None, None], [pos0.clone(), pos0.clone()]
        for k in range(6):
            w = k % 2
            torch.cuda.set_stream(streams[w])
            TA.set_stream(streams[w])
            bufs[w].copy_(pos0)
            outs[w] = pair[w].trace(bufs[w], dd)
        torch.cuda.synchronize()
        for out, ref, name in zip(outs, refs, names):
            equal_traces({k: out[k].cpu().numpy() for k in TRACE_KEYS}, ref, name)
    finally:
        TA.set_in_flight(1)
        torch.cuda.set_stream(torch.cuda.default_stream(dev))
        TA.set_stream(None)
        for st in pair:
            st.destroy()


# ---- optional machinery ---------------------------------------------------------------------

CONFIGURATIONS = (
    ("all off", dict(TURTLE_AMD_POOL="0", TURTLE_AMD_CREEP_LANES="0", TURTLE_AMD_DENSE_GO="0")),
    ("defaults", {}),
    ("pool, dense", dict(TURTLE_AMD_POOL="1", TURTLE_AMD_CREEP_LANES="64")),
    ("sorted, spatial", dict(TURTLE_AMD_SORT_KEY="1", TURTLE_AMD_SPATIAL="1")),
    ("one phase", dict(TURTLE_AMD_PARK="0")),
)


@pytest.mark.parametrize("name", ["example", "coarse"])
def test_optional_machinery_changes_no_bit(tmp_path, name):
    """the lean loop, the ray pool, the ordered hand-over and the spatial order, off and on
    (test_creep_loop_changes_no_bit): equal bits; the hand-over at step 32 (the default) against
    never (test_hand_over_step_moves_no_result): the same media, lengths within 1e-7"""
    slope, resolution = PC.SETTINGS[name]
    results = {}
    for k, (tag, env) in enumerate(CONFIGURATIONS):
        out = os.path.join(tmp_path, f"run{k}.npz")
        work = os.path.join(tmp_path, f"work{k}")
        subprocess.run([sys.executable, os.path.join(HERE, "params_probe.py"), out, work, repr(slope),
                        repr(resolution)], check=True, env=dict(os.environ, **env), timeout=120)
        results[tag] = dict(np.load(out))
    base = results["all off"]
    assert base["map_n_steps"].max() > 1000 and base["stack_n_steps"].max() > 1000
    assert (base["map_n_steps"] > 512).sum() > 100
    for tag, r in results.items():
        if tag == "one phase":
            continue
        for key, ref in base.items():
            assert np.array_equal(r[key], ref), (tag, key)
    one, two = results["one phase"], results["defaults"]
    for tag in ("map", "stack"):
        assert np.array_equal(one[f"{tag}_index"], two[f"{tag}_index"]), tag
        rel = np.abs(one[f"{tag}_length"] - two[f"{tag}_length"]) / np.maximum(two[f"{tag}_length"], 1.0)
        assert rel.max() < 1e-7, (tag, rel.max())
        moved = int((one[f"{tag}_n_steps"] != two[f"{tag}_n_steps"]).sum())
        print(f"[{name}] hand-over never against at step 32, {tag}: {moved} of {two[f'{tag}_n_steps'].size} rays "
              f"take another step count, lengths within {rel.max():.1e}")


# ---- edges ------------------------------------------------------------------------------------

@pytest.mark.parametrize("edge", list(PC.EDGES))
def test_edges(math, edge):
    """test_degenerate_inputs' 12 rays and a ragged batch of 65, 600 steps at most, at settings no
    harness should make (params_cases.EDGES): every ray has the restatement's index pair and step
    count and a finite length where the restatement's is, within test_degenerate_inputs' bar
    (1e-6 of the length, of a millimetre at least: the ray with a NaN in its direction has the 6e-9 m
    a bisection from a bracket of 25 km leaves).  No ray is set apart.  max_steps bounds every kernel.

    A resolution below the 1e-8 m of the bisection's bracket is served by the STRICT kernels in
    either mode (device_launch.h, strict_math): with FAST's samples, a few 1e-9 m off, 8 of the 65 rays
    crept over the ground 4 to 32 steps of 1e-9 m earlier or later than the reference's, and 3 of
    them ended on the other side of the 600 steps (rays 0, 34, 37; lengths within 5e-11)."""
    slope, resolution = PC.EDGES[edge]
    geo = T.c1_oracle()
    m = B.c1_map()
    st = B.c1_stepper(m)
    st.slope, st.resolution = slope, resolution
    try:
        for p, q in PC.edge_batches():
            with np.errstate(all="ignore"):
                ref = geo.trace(p.copy(), q, max_steps=PC.EDGE_MAX_STEPS, slope=slope, resolution=resolution)
            t = st.trace(p.copy(), q, max_steps=PC.EDGE_MAX_STEPS)
            off = np.flatnonzero((t["index"] != ref["index"]).any(axis=1) | (t["n_steps"] != ref["n_steps"]))
            assert off.size == 0, (off, t["index"][off], ref["index"][off], t["n_steps"][off], ref["n_steps"][off])
            assert (t["n_steps"] <= PC.EDGE_MAX_STEPS).all()
            ok = np.isfinite(ref["length"])
            assert np.array_equal(np.isfinite(t["length"]), ok)
            bar = PC.BAR * np.maximum(ref["length"][ok], 1e-3)
            assert (np.abs(t["length"][ok] - ref["length"][ok]) <= bar).all(), (t["length"], ref["length"])
            if edge == "no step at all":
                live = ref["index"][:, 0] >= 0
                assert live.any() and (t["n_steps"][live] == PC.EDGE_MAX_STEPS).all()
                assert (t["length"][live] == 0).all()
            assert st.trace_stats()["steps"] == int(t["n_steps"].sum())
    finally:
        st.destroy()
        m.destroy()
