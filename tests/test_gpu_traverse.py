"""turtle_stepper_traverse_n on the GPU: lines of sight through every medium, against the
reference's loop (tests/golden/traverse.npz) and the CPU checker (tests/c/traverse_loop.c).

The bar, in both arithmetics and with no allowance: the same final index pair, crossing count and
step count, and every per-medium length within 1e-6 of that ray's total path."""
import os
import subprocess

import numpy as np
import pytest

import turtle_amd as TA
from turtle_amd import synth

import traverse_cases as TC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-6


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


# The rays outside the bar, by name.  An optimistic stepper decides, sample by
# sample, whether a step lands inside a surface; a ray that grazes a surface, or cuts through a sliver
# of it thinner than its step, can decide differently on an ulp -- the last ulp of asin/acos/atan2
# (STRICT against the x86 libm) or the fast transform's few ulps (FAST) -- and then takes a few more
# or fewer steps there (the same path length to 1e-10), or finds one more pair of crossings (the rough
# tile's 200 m per-node noise: slivers of rock a few metres thick).  "two"/"ground": rays that climb
# 2000 m through air over flat layers, where each step is 0.4 x the clearance below, so that an
# altitude difference grows by (1 + 0.4 sin(elevation)) a step and reaches the last step's overshoot
# of the ceiling; same steps and crossings, the air length within 7e-6.
OUTSIDE = {
    ("two_ground", "strict"): [465, 727],
    ("two_ground", "fast"): [465, 727, 745],
    ("hgt3601", "strict"): [32503, 187152],
    ("hgt3601", "fast"): [177167, 187152],
    ("rough1201", "strict"): [214, 2663, 5005, 13630, 14166, 21361, 23632, 27011, 35702, 45543, 48825, 49196, 51092, 53348, 55578, 82896, 100402, 103944, 111155, 115131, 117014, 120543, 127412, 130638, 131619, 139398, 141638, 142717, 147106, 150722, 150812, 152229, 157758, 158589, 160434, 164355, 167965, 169559, 177108, 177462, 185682, 194125, 194730, 198254],
    ("rough1201", "fast"): [2663, 4608, 13630, 16153, 16887, 20546, 21361, 21555, 23632, 27011, 48825, 49196, 50691, 51092, 53348, 70136, 82896, 100054, 100402, 103944, 111155, 127412, 131619, 134035, 139398, 139456, 139605, 141638, 147106, 150812, 158589, 164355, 169559, 177108, 177462, 185682, 194730, 198254, 199595],
}


def assert_bar(got, ref, what="", outside=()):
    """the bar for every ray; the named rays outside it are exactly the ones that fall outside"""
    total = ref["length"].sum(axis=0)
    off = np.abs(got["length"] - ref["length"]).max(axis=0)
    bad = (off > BAR * np.maximum(total, 1e-300)) | (got["n_steps"] != ref["n_steps"])
    bad |= (got["n_crossings"] != ref["n_crossings"]) | (got["index"] != ref["index"]).any(axis=1)
    ids = np.flatnonzero(bad)
    assert ids.tolist() == sorted(outside), \
        f"{what}: rays {ids[:10]}: off by {off[ids[:10]]} of {total[ids[:10]]}, steps " \
        f"{got['n_steps'][ids[:10]]} vs {ref['n_steps'][ids[:10]]}"
    # even those end where the reference's do
    assert np.array_equal(got["index"], ref["index"]), what


def same_bits(a, b, keys=("position", "index", "length", "n_steps", "n_crossings")):
    for k in keys:
        if a[k] is not None and b[k] is not None:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


@pytest.mark.parametrize("recipe", ["ground", "c2"])
@pytest.mark.parametrize("case", TC.CASES)
def test_traverse_matches_the_reference(steppers, golden, math, case, recipe):
    g = golden("traverse")
    if case == "rough":
        import hashlib
        assert hashlib.sha256(TC.nodes("rough").tobytes()).hexdigest() == str(g["rough_nodes_sha"])
    k = f"{case}_{recipe}_"
    ref = {name: g[k + name] for name in ("index", "length", "n_steps", "n_crossings")}
    st = steppers[case]
    assert st.media == ref["length"].shape[0]
    t = st.traverse(g[k + "position"].copy(), g[k + "direction"], float(g[k + "ceiling"]))
    assert_bar(t, ref, f"{case} {recipe} {math}", OUTSIDE.get((f"{case}_{recipe}", math), ()))
    s = st.trace_stats()
    assert s["rays"] == t["index"].shape[0] and s["steps"] == int(t["n_steps"].sum())
    assert s["capped"] == 0
    if recipe == "c2":  # the rays that start above the ceiling (or outside the data): no step
        first = -16 if case == "two" else -32   # (flat layers hold the rays off the tile)
        assert (t["n_steps"][first:] == 0).all()
        assert np.array_equal(t["position"][first:], g[k + "position"][first:])


def c2_rays(st, n, lat0, lon0, seed=0x5EED2026):
    lat, lon, az, el = synth.uniform_rays(n, (lat0, lat0 + 1), (lon0, lon0 + 1), seed=seed)
    pos, di = st.position(lat, lon, 500.0)
    assert (di >= 0).all()
    return pos, TA.ecef_from_horizontal(lat, lon, az, el)


@pytest.mark.parametrize("size", ["hgt3601", "rough1201"])
def test_traverse_full_size_every_ray(math, size, tmp_path):
    """2e5 rays of the C2 recipe with a 2000 m ceiling, every one against the CPU checker"""
    from oracle import ffi as O
    n = 200000
    if size == "hgt3601":
        m = TA.Map.load(synth.write_hgt(str(tmp_path), 45, 3, synth.HGT_N))
        geo = O.OracleGeometry(grids=[O.hgt_grid(45, 3, synth.srtm_like_nodes(45, 3))],
                               layers=[[(O.MAP, 0, 0.0)]])
    else:
        m = TA.Map.load(TC.write_tile(tmp_path, "rough"))
        geo = TC.oracle_geometry("rough")
    st = TA.Stepper()
    st.add_map(m, 0.0)
    try:
        pos, d = c2_rays(st, n, 45, 3)
        ref = TC.check(geo, pos, d, 2000.0)
        t = st.traverse(pos.copy(), d, 2000.0)
        assert_bar(t, ref, f"{size} {math}", OUTSIDE[(size, math)])
        assert (t["n_crossings"] > 1).sum() > n // 10   # lines of sight through several media
    finally:
        st.destroy()
        m.destroy()


def test_traverse_paged_stack(tmp_path):
    """a stack with a hole and room for 2 of its 8 tiles: the rays page tiles in, generation by
    generation; STRICT gives the bits of the resident run, FAST stays within the bar"""
    d = str(tmp_path / "grid")
    tiles = [(la, lo) for la in (44, 45, 46) for lo in (3, 4, 5) if (la, lo) != (45, 4)]
    for la, lo in tiles:
        synth.write_hgt(d, la, lo, 1201)
    full, paged = TA.Stack(d, 0), TA.Stack(d, 2)
    full.load()
    sf, sp = TA.Stepper(), TA.Stepper()
    sf.add_stack(full, 0.0)
    sp.add_stack(paged, 0.0)
    try:
        rng = np.random.default_rng(5)
        n = 3000
        lat, lon = rng.uniform(44.1, 46.9, n), rng.uniform(3.1, 5.9, n)
        az, el = rng.uniform(0, 360, n), rng.uniform(-8.0, 3.0, n)
        p0, d0 = sf.position(lat, lon, 300.0)
        keep = d0 == 0
        p0 = p0[keep]
        dire = TA.ecef_from_horizontal(lat, lon, az, el)[keep]
        for math in ("strict", "fast"):
            TA.set_math(math)
            paged.clear()
            t0 = sf.traverse(p0.copy(), dire, 2000.0)
            t1 = sp.traverse(p0.copy(), dire, 2000.0)
            assert sp.rounds > 1 and paged.resident <= 2
            s1 = sp.trace_stats()
            assert s1["rays"] == p0.shape[0] and s1["steps"] == int(t1["n_steps"].sum())
            if math == "strict":
                same_bits(t0, t1)
            else:
                assert_bar(t1, t0, "paged fast")   # (no ray of this batch outside the bar)
            lat1, lon1, _ = TA.ecef_to_geodetic(t1["position"])
            moved = (np.floor(lat1) != np.floor(lat[keep])) | (np.floor(lon1) != np.floor(lon[keep]))
            assert moved.sum() > 50
    finally:
        TA.set_math("fast")
        for o in (sf, sp, full, paged):
            o.destroy()


def test_traverse_outputs_sizes_spaces_and_stops(steppers, golden, math):
    import torch
    st = steppers["rough"]
    g = golden("traverse")
    pos = np.concatenate([g["rough_c2_position"], g["rough_ground_position"]] * 40)
    d = np.concatenate([g["rough_c2_direction"], g["rough_ground_direction"]] * 40)
    n = pos.shape[0]   # 80 000
    ceiling = 2400.0
    full = st.traverse(pos.copy(), d, ceiling)
    # optional outputs: asking for fewer changes no bit of the rest
    for want in ((), ("length",), ("n_steps",), ("n_crossings",), ("length", "n_crossings")):
        t = st.traverse(pos.copy(), d, ceiling, want=want)
        same_bits(full, t)
        for k in ("length", "n_steps", "n_crossings"):
            assert (t[k] is None) == (k not in want)
    # odd batch sizes: the same bits as one large batch
    at = 0
    for size in (1, 255, 257, 65537, n - 1 - 255 - 257 - 65537):
        t = st.traverse(pos[at:at + size].copy(), d[at:at + size], ceiling)
        sub = dict(full, length=full["length"][:, at:at + size])
        for k in ("position", "index", "n_steps", "n_crossings"):
            sub[k] = full[k][at:at + size]
        same_bits(t, sub)
        at += size
    assert at == n
    # numpy (HOST) and torch (DEVICE): the same bits
    tp, td = torch.tensor(pos, device="cuda"), torch.tensor(d, device="cuda")
    t = st.traverse(tp, td, ceiling)
    torch.cuda.synchronize()
    same_bits(full, {k: (v.cpu().numpy() if v is not None else None) for k, v in t.items()})
    assert tuple(t["length"].shape) == (st.media, n)
    # trace_stats: the summed outputs
    st.traverse(pos.copy(), d, ceiling, max_steps=40)
    capped = st.traverse(pos.copy(), d, np.inf, max_steps=40)
    s = st.trace_stats()
    assert s["rays"] == n and s["steps"] == int(capped["n_steps"].sum())
    assert s["capped"] == int(((capped["n_steps"] == 40) & (capped["index"][:, 0] >= 0)).sum()) > 0
    assert s["samples"] >= n + s["steps"]
    # max_steps = 0: the origin's sample, nothing moves
    z = st.traverse(pos.copy(), d, ceiling, max_steps=0)
    assert (z["n_steps"] == 0).all() and (z["length"] == 0).all() and np.array_equal(z["position"], pos)
    # starting at or above the ceiling: no step, the index of the origin's sample
    low = st.traverse(pos.copy(), d, -1e9)
    assert (low["n_steps"] == 0).all() and np.array_equal(low["index"], z["index"])
    # altitude_max = inf: until the data ends (or max_steps)
    inf = st.traverse(pos.copy(), d)
    assert (inf["index"][:, 0] == -1).all()
    assert (inf["n_steps"] >= full["n_steps"]).all()


def test_rock_length_example(tmp_path):
    exe = str(tmp_path / "rock_length")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "rock_length.c"), "-o", exe,
                           "-L" + os.path.dirname(TA.library_path()), "-lturtle_amd",
                           "-Wl,-rpath," + os.path.dirname(TA.library_path()), "-lm"])
    tile = synth.write_hgt(str(tmp_path), 45, 3, 1201)
    out = subprocess.run([exe, tile], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = [l for l in out.stdout.splitlines() if l.startswith("azimuth")]
    assert len(lines) >= 4
    assert any(float(l.split()[-2]) > 0 for l in lines)   # some line of sight through rock
