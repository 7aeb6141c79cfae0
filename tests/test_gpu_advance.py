"""turtle_stepper_advance_n on the GPU: rays advanced by a column-depth budget and a distance limit,
against the reference's loop (tests/golden/advance.npz), the CPU checker (tests/c/advance_loop.c),
traverse_n and crossings_n.

The bar, in both arithmetics: the same status, final medium and step count, depth within 1e-6 of the
ray's full depth, distance and position within 1e-6 of its total path."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import turtle_amd as TA

import advance_cases as AC
import crossings_cases as CC
import traverse_cases as TC
from test_gpu_crossings import c2_rays
from test_gpu_traverse import BAR, OUTSIDE as TRAVERSE_OUTSIDE

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = AC.OUTPUTS
INF = float("inf")


@pytest.fixture(params=["fast", "strict"])
def math(request):
    TA.set_math(request.param)
    yield request.param
    TA.set_math("fast")


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
    yield out
    for st in out.values():
        st.destroy()
    for m in keep:
        m.destroy()


def same_bits(a, b, keys=KEYS):
    for k in keys:
        if a[k] is not None and b[k] is not None:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k


def rays(t, mask):
    """the outputs of the rays of `mask`"""
    return {k: (None if t[k] is None else np.asarray(t[k])[mask]) for k in KEYS}


def off_the_bar(t, ref, D, T):
    """the rays that miss the bar against `ref`"""
    bad = (t["status"] != ref["status"]) | (t["index"][:, 0] != ref["index"][:, 0]) | (t["n_steps"] != ref["n_steps"])
    bad |= np.abs(t["depth"] - ref["depth"]) > BAR * D
    bad |= np.abs(t["distance"] - ref["distance"]) > BAR * T
    bad |= np.linalg.norm(t["position"] - ref["position"], axis=1) > BAR * T
    return np.flatnonzero(bad)


def on_the_ray(t, origin, direction, T):
    """every ray ends on its own line, at the distance it reports"""
    where = origin + direction * t["distance"][:, None]
    off = np.linalg.norm(t["position"] - where, axis=1)
    assert (off <= BAR * np.maximum(T, 1.0)).all(), (int(np.argmax(off)), float(off.max()))


def batch(golden, case, recipe):
    g, a = golden("traverse"), golden("advance")
    k = f"{case}_{recipe}_"
    out = {name: g[k + name] for name in ("position", "direction", "length")}
    out.update(ceiling=float(g[k + "ceiling"]), traverse_index=g[k + "index"])
    out.update({name: a[k + name] for name in ("budget", "distance_max", "density")})
    out["ref"] = {name: a[k + name] for name in KEYS}
    out["T"] = out["length"].sum(axis=0)
    out["D"] = (out["density"][:, None] * out["length"]).sum(axis=0)
    return out


@pytest.mark.parametrize("recipe", ["ground", "c2"])
@pytest.mark.parametrize("case", TC.CASES)
def test_advance_matches_the_reference(steppers, golden, math, case, recipe):
    b = batch(golden, case, recipe)
    st = steppers[case]
    assert st.media == b["density"].shape[0]
    t = st.advance(b["position"].copy(), b["direction"], b["density"], b["budget"], b["distance_max"], b["ceiling"])
    ids = off_the_bar(t, b["ref"], b["D"], b["T"])
    for r in ids:
        print(f"{case} {recipe} {math}: ray {r} status {t['status'][r]} / {b['ref']['status'][r]}, steps "
              f"{t['n_steps'][r]} / {b['ref']['n_steps'][r]}, depth off {abs(t['depth'][r] - b['ref']['depth'][r]):.3e} "
              f"of {b['D'][r]:.3e}, distance off {abs(t['distance'][r] - b['ref']['distance'][r]):.3e} of {b['T'][r]:.3e}")
    # the only rays excused: those that miss traverse's own bar in this batch and arithmetic
    assert set(ids.tolist()) <= set(TRAVERSE_OUTSIDE.get((f"{case}_{recipe}", math), [])), ids.tolist()
    assert len(ids) <= 3
    on_the_ray(t, b["position"], b["direction"], b["T"])
    s = st.trace_stats()
    assert s["rays"] == t["status"].shape[0] and s["steps"] == int(t["n_steps"].sum()) and s["capped"] == 0
    assert st.rounds == 1
    # a ray the budget stopped has spent it to the bit; one the limit stopped stands at the limit
    spent, far = t["status"] == AC.SPENT, t["status"] == AC.DISTANCE
    assert np.array_equal(t["depth"][spent], b["budget"][spent])
    assert np.array_equal(t["distance"][far], b["distance_max"][far])


@pytest.mark.parametrize("case", TC.CASES)
def test_advance_without_a_budget_is_traverse(steppers, golden, math, case):
    """budget = inf, no distance limit: the bits of traverse_n, its statistics, and the path that
    crossings_n records where a ray leaves the data"""
    st = steppers[case]
    for recipe in ("ground", "c2"):
        b = batch(golden, case, recipe)
        n = b["position"].shape[0]
        args = (b["direction"], b["ceiling"])
        tr = st.traverse(b["position"].copy(), *args)
        s = st.trace_stats()
        t = st.advance(b["position"].copy(), b["direction"], b["density"], np.full(n, INF), None, b["ceiling"])
        assert st.trace_stats() == s
        same_bits(tr, t, ("position", "index", "n_steps"))
        assert np.isin(t["status"], (AC.LEFT, AC.CEILING)).all()
        assert np.array_equal(t["status"] == AC.LEFT, tr["index"][:, 0] < 0)
        capacity = int(tr["n_crossings"].max()) + 1
        x = st.crossings(b["position"].copy(), *args, capacity=capacity)
        left = np.flatnonzero((x["index"][:, 0] < 0) & (x["n_crossings"] > 0) & (x["n_crossings"] <= capacity))
        assert np.array_equal(t["distance"][left], x["distance"][x["n_crossings"][left] - 1, left])
        if case != "two":
            assert left.size > 100
        # unit densities: the depth is the distance, to the bit
        one = np.ones(st.media)
        u = st.advance(b["position"].copy(), b["direction"], one, np.full(n, INF), None, b["ceiling"])
        same_bits(t, u, ("position", "index", "distance", "n_steps", "status"))
        assert np.array_equal(u["depth"], u["distance"])
        # ... and with a distance limit: on the bit of the limit, the depth within 4 ulp of it
        v = st.advance(b["position"].copy(), b["direction"], one, np.full(n, INF), b["distance_max"], b["ceiling"])
        far = v["status"] == AC.DISTANCE
        assert far.sum() > 50 and not (v["status"] == AC.SPENT).any()
        assert np.array_equal(v["distance"][far], b["distance_max"][far])
        assert (np.abs(v["depth"][far] - v["distance"][far]) <= 4 * np.spacing(v["distance"][far])).all()
        assert np.array_equal(v["depth"][~far], v["distance"][~far])
        same_bits(rays(u, ~far), rays(v, ~far))           # the limit changes nothing for the others


def test_advance_against_crossings_20000_rays(math, tmp_path):
    """20 000 C2 rays over the rough tile, budgets by the recipe from this run's own traverse and
    crossings: numpy's piecewise-linear stop agrees with the call, and the CPU checker at the bar"""
    n = 20000
    m = TA.Map.load(TC.write_tile(tmp_path, "rough"))
    st = TA.Stepper()
    st.add_map(m, 0.0)
    try:
        pos, d = c2_rays(st, n, TC.LAT0, TC.LON0)
        ceiling = 2000.0
        tr = st.traverse(pos.copy(), d, ceiling)
        x = st.crossings(pos.copy(), d, ceiling, capacity=int(tr["n_crossings"].max()) + 1)
        rows = CC.ragged(x)
        density = AC.DENSITY[2]
        b = AC.budgets(np.random.default_rng(AC.SEED), x["length"], x["index"], rows["offset"], rows["distance"],
                       rows["media"], density)
        T = x["length"].sum(axis=0)
        D = (density[:, None] * x["length"]).sum(axis=0)
        t = st.advance(pos.copy(), d, density, b["budget"], b["distance_max"], ceiling)
        counts = np.bincount(t["status"], minlength=5)
        print(f"{math}: status {counts.tolist()}, least margin {b['margin'].min():.2e} T")
        assert counts[AC.SPENT] > n // 4 and counts[AC.DISTANCE] > n // 20 and counts[AC.LEFT] > n // 20
        assert np.array_equal(t["status"], b["status"])
        assert (np.abs(t["distance"] - b["stop"]) <= 1e-9 * T).all()
        assert (np.abs(t["depth"] - b["depth"]) <= 1e-9 * D).all()
        on_the_ray(t, pos, d, T)
        ref = AC.check(TC.oracle_geometry("rough"), pos, d, density, b["budget"], b["distance_max"], ceiling)
        ids = off_the_bar(t, ref, D, T)
        for r in ids:
            print(f"{math}: ray {r} off the bar: status {t['status'][r]} / {ref['status'][r]}, steps {t['n_steps'][r]} / "
                  f"{ref['n_steps'][r]}, distance off {abs(t['distance'][r] - ref['distance'][r]):.3e} of {T[r]:.3e}")
        assert len(ids) <= n // 2000, ids.tolist()
    finally:
        st.destroy()
        m.destroy()


def test_advance_is_additive(steppers, golden, math):
    """advance by b1, then from where that ended by b2 (fresh samples): the depths and distances
    add up to those of one advance by b1 + b2"""
    st = steppers["hgt"]
    b = batch(golden, "hgt", "c2")
    b1 = b2 = 0.5 * b["budget"]          # (b1 + b2 is the budget to the bit)
    args = (b["direction"], b["density"])
    one = st.advance(b["position"].copy(), *args, b["budget"], None, b["ceiling"])
    first = st.advance(b["position"].copy(), *args, b1, None, b["ceiling"])
    second = st.advance(first["position"].copy(), *args, b2, None, b["ceiling"])
    on = first["status"] == AC.SPENT
    assert on.sum() > 400
    tol = BAR * b["T"][on]
    assert (np.abs(first["depth"] + second["depth"] - one["depth"])[on] <= tol).all()
    assert (np.abs(first["distance"] + second["distance"] - one["distance"])[on] <= tol).all()
    assert np.array_equal(second["status"][on], one["status"][on])
    assert (np.linalg.norm(second["position"] - one["position"], axis=1)[on] <= tol).all()


def test_advance_edges(steppers, golden, math):
    st = steppers["hgt"]
    b = batch(golden, "hgt", "c2")
    pos, d, rho, ceiling = b["position"][:64], b["direction"][:64], b["density"], b["ceiling"]
    n = 64
    assert (b["T"][:n] > 0).all()
    # a budget of 0, or NaN: spent at the origin; a limit of 0: reached there
    for budget, limit, status in ((0.0, None, AC.SPENT), (np.nan, None, AC.SPENT), (-1.0, None, AC.SPENT),
                                  (INF, 0.0, AC.DISTANCE), (0.0, 0.0, AC.SPENT)):
        t = st.advance(pos.copy(), d, rho, np.full(n, budget), None if limit is None else np.full(n, limit), ceiling)
        assert (t["status"] == status).all() and (t["n_steps"] == 0).all()
        assert np.array_equal(t["position"], pos) and (t["depth"] == 0).all() and (t["distance"] == 0).all()
        assert (t["index"][:, 0] == 1).all()                 # (in the air, 500 m above the ground)
    # a start outside the data, and one above the ceiling: rays [-32:-16] and [-16:] of the recipe
    tail = st.advance(b["position"][-32:].copy(), b["direction"][-32:], rho, np.full(32, 1.0), np.full(32, 1.0), ceiling)
    assert (tail["status"][:16] == AC.LEFT).all() and (tail["index"][:16, 0] == -1).all()
    assert (tail["status"][16:] == AC.CEILING).all() and (tail["index"][16:, 0] == 1).all()
    assert (tail["n_steps"] == 0).all() and np.array_equal(tail["position"], b["position"][-32:])
    assert (tail["depth"] == 0).all() and (tail["distance"] == 0).all()
    # max_steps
    full = st.advance(pos.copy(), d, rho, np.full(n, INF), None, ceiling)
    t = st.advance(pos.copy(), d, rho, np.full(n, INF), None, ceiling, max_steps=5)
    capped = t["status"] == AC.MAX_STEPS
    assert np.array_equal(capped, full["n_steps"] > 5) and capped.sum() > n // 2
    assert (t["n_steps"][capped] == 5).all() and st.trace_stats()["capped"] == int(capped.sum())
    same_bits(rays(full, ~capped), rays(t, ~capped))
    zero = st.advance(pos.copy(), d, rho, np.full(n, INF), None, ceiling, max_steps=0)
    assert (zero["status"] == AC.MAX_STEPS).all() and np.array_equal(zero["position"], pos)
    # vacuum above the ground: nothing is spent in the air, and a tiny budget lasts down to the rock
    tr = st.traverse(pos.copy(), d, ceiling)
    x = st.crossings(pos.copy(), d, ceiling, capacity=max(int(tr["n_crossings"].max()) + 1, 2))
    vac = np.array([2650.0, 0.0])
    t = st.advance(pos.copy(), d, vac, np.full(n, INF), None, ceiling)
    same_bits(full, t, ("position", "index", "distance", "n_steps", "status"))
    assert (np.abs(t["depth"] - 2650.0 * tr["length"][0]) <= 1e-9 * 2650.0 * tr["length"][0]).all()
    t = st.advance(pos.copy(), d, vac, np.full(n, 1.0), None, ceiling)
    hit = (x["n_crossings"] > 0) & (x["media"][0, :, 1] == 0)      # the ray's first crossing enters the rock
    assert hit.sum() > n // 2
    # ... for more than a metre (2650 kg/m^2, where the budget is 1)
    deep = hit & (np.where(x["n_crossings"] > 1, x["distance"][1], INF) - x["distance"][0] > 1.0)
    assert deep.sum() > n // 2
    assert (t["status"][deep] == AC.SPENT).all() and (t["index"][deep, 0] == 0).all() and (t["depth"][deep] == 1.0).all()
    assert (np.abs(t["distance"][deep] - (x["distance"][0, deep] + 1.0 / 2650.0)) <= 1e-9 * b["T"][:n][deep]).all()
    never = tr["length"][0] == 0
    assert (t["status"][never] != AC.SPENT).all() and (t["depth"][never] == 0).all()
    # an infinite density: the ray stops where its first step in that medium starts
    t = st.advance(pos.copy(), d, np.array([INF, 1.205]), np.full(n, 1e9), None, ceiling)
    assert (t["status"][hit] == AC.SPENT).all() and (t["index"][hit, 0] == 0).all() and (t["depth"][hit] == 1e9).all()
    assert np.array_equal(t["position"][hit], x["point"][0, hit])
    assert np.array_equal(t["distance"][hit], x["distance"][0, hit])
    same_bits(rays(full, ~hit), rays(t, ~hit), ("position", "index", "distance", "n_steps", "status"))


def test_advance_outputs_sizes_and_spaces(steppers, golden, math):
    import torch
    st = steppers["two"]
    parts = [batch(golden, "two", "c2"), batch(golden, "two", "ground")] * 3
    pos, d, budget, limit = (np.concatenate([p[name] for p in parts])
                             for name in ("position", "direction", "budget", "distance_max"))
    rho, ceiling = parts[0]["density"], 2000.0
    n = pos.shape[0]   # 6000
    full = st.advance(pos.copy(), d, rho, budget, limit, ceiling)
    assert {AC.SPENT, AC.DISTANCE, AC.CEILING} <= set(full["status"].tolist())
    optional = ("depth", "distance", "n_steps")
    # optional outputs: asking for fewer changes no bit of the rest
    for k in range(len(optional) + 1):
        for want in itertools.combinations(optional, k):
            t = st.advance(pos.copy(), d, rho, budget, limit, ceiling, want=want)
            same_bits(full, t)
            for name in optional:
                assert (t[name] is None) == (name not in want)
    # ... and no limit at all is a limit of inf
    same_bits(st.advance(pos.copy(), d, rho, budget, None, ceiling),
              st.advance(pos.copy(), d, rho, budget, np.full(n, INF), ceiling))
    # batch sizes that are not multiples of 64: the same bits as one batch
    at = 0
    for size in (1, 63, 65, 1000, n - 1129):
        cut = slice(at, at + size)
        t = st.advance(pos[cut].copy(), d[cut], rho, budget[cut], limit[cut], ceiling)
        same_bits(t, {k: full[k][cut] for k in KEYS})
        at += size
    assert at == n
    # numpy (HOST) and torch (DEVICE): the same bits
    dev = [torch.tensor(a, device="cuda") for a in (pos, d, rho, budget, limit)]
    t = st.advance(*dev, ceiling)
    torch.cuda.synchronize()
    same_bits(full, {k: v.cpu().numpy() for k, v in t.items()})
    # the raw call over outputs full of garbage: every element written
    out = dict(position=pos.copy(), index=np.full((n, 2), -9, np.int32), depth=np.full(n, np.nan),
               distance=np.full(n, -7.0), n_steps=np.full(n, -5, np.int32), status=np.full(n, -3, np.int32))
    p = {k: v.ctypes.data_as(C.c_void_p) for k, v in out.items()}
    ins = [np.ascontiguousarray(a).ctypes.data_as(C.c_void_p) for a in (d, rho, budget, limit)]
    assert TA.lib().turtle_stepper_advance_n(st.h, C.c_long(n), p["position"], *ins, C.c_double(ceiling), 1000000,
                                             p["index"], p["depth"], p["distance"], p["n_steps"], p["status"],
                                             TA.HOST) == 0
    same_bits(full, out)


def test_advance_over_stacks(tmp_path):
    """a 2 x 2 stack, every tile loaded: the call made again gives the same bits; a stack without
    room for its tiles is refused"""
    d = str(tmp_path / "grid")
    for la, lo in ((45, 3), (45, 4), (46, 3), (46, 4)):
        TA.synth.write_hgt(d, la, lo, 1201)
    full, small = TA.Stack(d, 0), TA.Stack(d, 1)
    full.load()
    sf, ss = TA.Stepper(), TA.Stepper()
    sf.add_stack(full, 0.0)
    ss.add_stack(small, 0.0)
    try:
        rng = np.random.default_rng(9)
        n = 3000
        lat, lon = rng.uniform(45.1, 46.9, n), rng.uniform(3.1, 4.9, n)
        az, el = rng.uniform(0, 360, n), rng.uniform(-8.0, 3.0, n)
        p0, _ = sf.position(lat, lon, 300.0)
        dire = TA.ecef_from_horizontal(lat, lon, az, el)
        rho = AC.DENSITY[2]
        for math in ("strict", "fast"):
            TA.set_math(math)
            tr = sf.traverse(p0.copy(), dire, 2000.0)
            budget = rng.uniform(0.05, 1.6, n) * (rho[:, None] * tr["length"]).sum(axis=0)
            limit = rng.uniform(0.5, 3.0, n) * tr["length"].sum(axis=0)
            t1 = sf.advance(p0.copy(), dire, rho, budget, limit, 2000.0)
            assert sf.rounds == 1
            same_bits(t1, sf.advance(p0.copy(), dire, rho, budget, limit, 2000.0))
            assert {AC.SPENT, AC.DISTANCE, AC.LEFT} <= set(t1["status"].tolist())
            same_bits(tr, sf.advance(p0.copy(), dire, rho, np.full(n, INF), None, 2000.0), ("position", "index", "n_steps"))
            with pytest.raises(TA.TurtleError) as err:
                ss.advance(p0.copy(), dire, rho, budget, limit, 2000.0)
            assert err.value.name == "DOMAIN_ERROR" and "resident tiles only" in str(err.value)
            assert "turtle_stepper_advance_n" in str(err.value)
    finally:
        TA.set_math("fast")
        for o in (sf, ss, full, small):
            o.destroy()


def test_column_depth_example(tmp_path):
    exe = str(tmp_path / "column_depth")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "column_depth.c"), "-o", exe,
                           "-L" + os.path.dirname(TA.library_path()), "-lturtle_amd",
                           "-Wl,-rpath," + os.path.dirname(TA.library_path()), "-lm"])
    tile = TC.write_tile(tmp_path, "rough")
    out = subprocess.run([exe, tile], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    lat0, lon0 = (float(v) for v in lines[0].split()[1:3])
    rows = [l.split() for l in lines if l.startswith("ray")]
    assert len(rows) == 324 and any(r[10] == "spent" for r in rows)
    assert lines[-1].startswith("chord") and lines[-1].split()[4] in ("distance", "left")
    # the same fan through the binding: three of its stops, one for each budget
    TA.set_math("fast")
    m = TA.Map.load(tile)
    st = TA.Stepper()
    st.add_map(m, 0.0)
    try:
        r = np.arange(324)
        f = r % 108
        az, el = 360.0 * (f % 36) / 36, 2.0 + 6.0 * (f // 36)
        lat, lon = np.full(324, lat0), np.full(324, lon0)
        pos, _ = st.position(lat, lon, np.full(324, 0.5))
        budget = np.array([4.84e4, 4.08e5, 2.45e6])[r // 108]
        t = st.advance(pos, TA.ecef_from_horizontal(lat, lon, az, el), np.array([2650.0, 1.205]), budget, None, 4000.0)
        names = ("spent", "distance", "left", "ceiling", "max_steps")
        for ray in (7, 108 + 50, 216 + 101):
            row = rows[ray]
            assert int(row[1]) == ray and row[10] == names[t["status"][ray]]
            assert abs(float(row[12]) - t["distance"][ray]) < 1e-5
            assert abs(float(row[15]) - t["depth"][ray]) <= 1e-6 * t["depth"][ray]
        # the last line: the rock between the point and the example's second one, point to point
        last = lines[-1].split()
        origin, _ = st.position(lat[:1], lon[:1], np.full(1, 0.5))
        target, _ = st.position(lat[:1] + 0.03, lon[:1] + 0.03, np.full(1, 300.0))
        length = np.linalg.norm(target - origin, axis=1)
        c = st.advance(origin.copy(), (target - origin) / length, np.array([1.0, 0.0]), np.full(1, INF), length, INF)
        assert abs(float(last[1]) - length[0]) < 1e-5 and last[4] == names[c["status"][0]]
        assert abs(float(last[6]) - c["depth"][0]) < 1e-5 and c["depth"][0] <= length[0]
    finally:
        st.destroy()
        m.destroy()
