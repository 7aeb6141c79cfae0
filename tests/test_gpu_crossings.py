"""turtle_stepper_crossings_n on the GPU: traverse_n's lines of sight with every crossing point,
against the reference's loop (tests/golden/crossings.npz) and the CPU checker
(tests/c/crossings_loop.c).

The bar, in both arithmetics: the same crossing count and media pairs, every distance within 1e-6
of the ray's total path, every point within 1e-6 x the total path (metres).  With no allowance:
position, index, length, n_steps and n_crossings are the bits of traverse_n."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import turtle_amd as TA
from turtle_amd import synth

import crossings_cases as CC
import traverse_cases as TC
from test_gpu_traverse import OUTSIDE as TRAVERSE_OUTSIDE

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR = 1e-6
KEYS = ("position", "index", "length", "n_steps", "n_crossings")

# The rays outside the bar, by name: each one is a ray of test_gpu_traverse.py's
# OUTSIDE for the same case and mode, which decides an ulp differently from the reference and then
# finds one more or one fewer pair of crossings.
OUTSIDE = {
    ("rough1201", "strict"): [158589, 198254],
    ("rough1201", "fast"): [100054, 158589],
}


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
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def outside_bar(t, ref, total):
    """the rays whose recorded crossings miss the bar against `ref` (ragged, cut to the same
    capacity): another count, another media pair, a distance or a point off by more than
    BAR x the ray's total path"""
    got = CC.ragged(t)
    bad = t["n_crossings"] != ref["n_crossings"]
    n = bad.shape[0]
    kept_g, kept_r = np.diff(got["offset"]), np.diff(ref["offset"])
    same = ~bad & (kept_g == kept_r)
    bad |= kept_g != kept_r
    rg = np.repeat(np.arange(n), kept_g)
    rr = np.repeat(np.arange(n), kept_r)
    gi, ri = same[rg], same[rr]
    ray = rg[gi]
    err = np.zeros(n)
    e = np.maximum(np.abs(got["distance"][gi] - ref["distance"][ri]),
                   np.linalg.norm(got["point"][gi] - ref["point"][ri], axis=1))
    np.maximum.at(err, ray, e)
    mismatch = np.zeros(n, dtype=bool)
    np.logical_or.at(mismatch, ray, (got["media"][gi] != ref["media"][ri]).any(axis=1))
    bad |= mismatch | (err > BAR * np.maximum(total, 1e-300))
    return np.flatnonzero(bad)


def assert_outside(ids, key, math):
    named = OUTSIDE.get((key, math), [])
    assert ids.tolist() == sorted(named), f"{key} {math}: rays outside the bar {ids.tolist()}"
    assert set(named) <= set(TRAVERSE_OUTSIDE.get((key, math), []))


def invariants(t, strict_origin=None):
    """what holds on every ray, whatever the reference says"""
    cap = t["distance"].shape[0]
    count = t["n_crossings"]
    kept = np.minimum(count, cap)
    slot = np.arange(cap)[:, None]
    on = slot < kept[None, :]
    # distances strictly increase; each crossing starts in the medium the last one entered
    both = on[1:] & on[:-1]
    assert (t["distance"][1:] > t["distance"][:-1])[both].all()
    assert (t["media"][1:, :, 0] == t["media"][:-1, :, 1])[both].all()
    # the slots past the recorded ones are zero
    assert (t["distance"][~on] == 0).all() and (t["point"][~on] == 0).all() and (t["media"][~on] == 0).all()
    if strict_origin is not None:   # (step_n is always strict)
        has = kept > 0
        assert np.array_equal(t["media"][0, has, 0], strict_origin[has])
    # a ray that left the data: its last crossing entered -1, at its final position
    left = (t["index"][:, 0] == -1) & (count > 0) & (count <= cap)
    r = np.flatnonzero(left)
    last = kept[r] - 1
    assert (t["media"][last, r, 1] == -1).all()
    assert np.array_equal(t["point"][last, r], t["position"][r])
    # ... and its path summed per medium is the last recorded distance
    total = t["length"].sum(axis=0)[r]
    assert np.allclose(t["distance"][last, r], total, rtol=1e-11, atol=0)
    # no other crossing enters -1
    assert not ((t["media"][:, :, 1] == -1) & on & (slot != (kept - 1)[None, :])).any()
    return int(left.sum())


@pytest.mark.parametrize("recipe", ["ground", "c2"])
@pytest.mark.parametrize("case", TC.CASES)
def test_crossings_match_the_reference(steppers, golden, math, case, recipe):
    g, x = golden("traverse"), golden("crossings")
    k = f"{case}_{recipe}_"
    ref = {name: x[k + name] for name in ("offset", "point", "distance", "media")}
    ref["n_crossings"] = g[k + "n_crossings"]
    capacity = int(g[k + "n_crossings"].max()) + 1
    st = steppers[case]
    args = (g[k + "direction"], float(g[k + "ceiling"]))
    t = st.crossings(g[k + "position"].copy(), *args, capacity=capacity)
    assert_outside(outside_bar(t, ref, g[k + "length"].sum(axis=0)), f"{case}_{recipe}", math)
    # the bits of traverse_n, and its statistics
    s = st.trace_stats()
    same_bits(st.traverse(g[k + "position"].copy(), *args), t)
    assert st.trace_stats() == s and s["rays"] == t["index"].shape[0]
    origin = st.step(g[k + "position"].copy())["index"][:, 0] if math == "strict" else None
    invariants(t, origin)


def c2_rays(st, n, lat0, lon0, seed=0x5EED2026):
    lat, lon, az, el = synth.uniform_rays(n, (lat0, lat0 + 1), (lon0, lon0 + 1), seed=seed)
    pos, di = st.position(lat, lon, 500.0)
    assert (di >= 0).all()
    return pos, TA.ecef_from_horizontal(lat, lon, az, el)


@pytest.mark.parametrize("size", ["hgt3601", "rough1201"])
def test_crossings_full_size(math, size, tmp_path):
    """2e5 rays of the C2 recipe with a 2000 m ceiling: the bits of traverse_n, every crossing
    against the CPU checker, the invariants, and (single-layer sin.cos tile) every rock / air
    crossing on the ground"""
    from oracle import ffi as O
    n, capacity = 200000, 32
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
        t = st.crossings(pos.copy(), d, 2000.0, capacity=capacity)
        same_bits(st.traverse(pos.copy(), d, 2000.0), t)
        ref = CC.check(geo, pos, d, 2000.0)
        cut = CC.first(ref, capacity)
        cut["n_crossings"] = ref["n_crossings"]
        assert_outside(outside_bar(t, cut, ref["length"].sum(axis=0)), size, math)
        origin = st.step(pos.copy())["index"][:, 0] if math == "strict" else None
        assert invariants(t, origin) > n // 100
        assert (t["n_crossings"] > 1).sum() > n // 10
        if size == "hgt3601":   # rock (0) / air (1): within 1e-6 m of the ground
            on = np.arange(capacity)[:, None] < np.minimum(t["n_crossings"], capacity)[None, :]
            pair = t["media"][on]
            ground = ((pair[:, 0] == 0) & (pair[:, 1] == 1)) | ((pair[:, 0] == 1) & (pair[:, 1] == 0))
            p = t["point"][on][ground]
            assert p.shape[0] > n // 2
            TA.set_math("strict")
            lat, lon, alt = TA.ecef_to_geodetic(p)
            TA.set_math(math)
            z, inside = m.elevation(lon, lat)
            assert inside.all()
            assert np.abs(alt - z).max() < 1e-6
    finally:
        st.destroy()
        m.destroy()


def test_crossings_paged_stack(tmp_path):
    """a 2 x 2 stack with room for 1 tile: the rays page tiles in, generation by generation; the
    bits of traverse_n on the same stepper, and in STRICT those of the resident stack"""
    d = str(tmp_path / "grid")
    for la, lo in ((45, 3), (45, 4), (46, 3), (46, 4)):
        synth.write_hgt(d, la, lo, 1201)
    full, paged = TA.Stack(d, 0), TA.Stack(d, 1)
    full.load()
    sf, sp = TA.Stepper(), TA.Stepper()
    sf.add_stack(full, 0.0)
    sp.add_stack(paged, 0.0)
    try:
        rng = np.random.default_rng(9)
        n = 3000
        lat, lon = rng.uniform(45.1, 46.9, n), rng.uniform(3.1, 4.9, n)
        az, el = rng.uniform(0, 360, n), rng.uniform(-8.0, 3.0, n)
        p0, _ = sf.position(lat, lon, 300.0)
        dire = TA.ecef_from_horizontal(lat, lon, az, el)
        for math in ("strict", "fast"):
            TA.set_math(math)
            paged.clear()
            t1 = sp.crossings(p0.copy(), dire, 2000.0, capacity=16)
            assert sp.rounds > 1 and paged.resident <= 1
            s1 = sp.trace_stats()
            assert s1["rays"] == n and s1["steps"] == int(t1["n_steps"].sum())
            paged.clear()
            same_bits(sp.traverse(p0.copy(), dire, 2000.0), t1)
            assert (t1["n_crossings"] > 0).sum() > 100
            if math == "strict":
                t0 = sf.crossings(p0.copy(), dire, 2000.0, capacity=16)
                same_bits(t0, t1, KEYS + ("point", "distance", "media"))
                invariants(t1, sf.step(p0.copy())["index"][:, 0])
            else:
                invariants(t1)
    finally:
        TA.set_math("fast")
        for o in (sf, sp, full, paged):
            o.destroy()


def test_crossings_overflow(steppers, golden):
    """capacity 1 and 4 on the rough tile: the true counts, the first slots of a larger run, and
    zeros past them (in arrays that held something else)"""
    st = steppers["rough"]
    g = golden("traverse")
    pos = np.concatenate([g["rough_c2_position"], g["rough_ground_position"]])
    d = np.concatenate([g["rough_c2_direction"], g["rough_ground_direction"]])
    n = pos.shape[0]
    big = st.crossings(pos.copy(), d, 2400.0, capacity=64)
    assert (big["n_crossings"] > 4).sum() > 100
    L = TA.lib()
    for capacity in (1, 4):
        t = st.crossings(pos.copy(), d, 2400.0, capacity=capacity)
        same_bits(big, t)
        for k in ("point", "distance", "media"):
            assert np.array_equal(t[k], big[k][:capacity]), (capacity, k)
        # the raw call over arrays full of garbage: the same slots, the same zeros
        out = dict(position=pos.copy(), index=np.empty((n, 2), np.int32), n_crossings=np.empty(n, np.int32),
                   point=np.full((capacity, n, 3), np.nan), distance=np.full((capacity, n), -7.0),
                   media=np.full((capacity, n, 2), -9, np.int32))
        p = {k: v.ctypes.data_as(C.c_void_p) for k, v in out.items()}
        dp = np.ascontiguousarray(d).ctypes.data_as(C.c_void_p)
        assert L.turtle_stepper_crossings_n(st.h, C.c_long(n), p["position"], dp, C.c_double(2400.0),
                                            1000000, p["index"], None, None, p["n_crossings"], capacity,
                                            p["point"], p["distance"], p["media"], TA.HOST) == 0
        for k in ("position", "index", "n_crossings", "point", "distance", "media"):
            assert np.array_equal(out[k], t[k]), (capacity, k)


def test_crossings_outputs_sizes_and_spaces(steppers, golden, math):
    import torch
    st = steppers["two"]
    g = golden("traverse")
    pos = np.concatenate([g["two_c2_position"], g["two_ground_position"]] * 3)
    d = np.concatenate([g["two_c2_direction"], g["two_ground_direction"]] * 3)
    n = pos.shape[0]   # 6000
    ceiling = 2000.0
    full = st.crossings(pos.copy(), d, ceiling, capacity=8)
    rec = ("point", "distance", "media")
    # optional outputs: asking for fewer changes no bit of the rest
    for want in ((), ("length",), ("n_steps",), ("point",), ("distance", "media")):
        t = st.crossings(pos.copy(), d, ceiling, capacity=8, want=want)
        same_bits(full, t, KEYS + rec)
        for k in ("length", "n_steps") + rec:
            assert (t[k] is None) == (k not in want)
    # capacity 0: traverse_n with the counts
    zero = st.crossings(pos.copy(), d, ceiling, capacity=0, want=("length", "n_steps"))
    same_bits(st.traverse(pos.copy(), d, ceiling), zero)
    same_bits(full, zero)
    # batch sizes that are not multiples of 64: the same bits as one batch
    at = 0
    for size in (1, 63, 65, 1000, n - 1129):
        t = st.crossings(pos[at:at + size].copy(), d[at:at + size], ceiling, capacity=8)
        sub = {k: full[k][at:at + size] for k in ("position", "index", "n_steps", "n_crossings")}
        sub.update(length=full["length"][:, at:at + size], point=full["point"][:, at:at + size],
                   distance=full["distance"][:, at:at + size], media=full["media"][:, at:at + size])
        same_bits(t, sub, KEYS + rec)
        at += size
    assert at == n
    # numpy (HOST) and torch (DEVICE): the same bits
    tp, td = torch.tensor(pos, device="cuda"), torch.tensor(d, device="cuda")
    t = st.crossings(tp, td, ceiling, capacity=8)
    torch.cuda.synchronize()
    same_bits(full, {k: v.cpu().numpy() for k, v in t.items()}, KEYS + rec)
    assert tuple(t["point"].shape) == (8, n, 3) and tuple(t["media"].shape) == (8, n, 2)
    # stops at max_steps and at the ceiling are not crossings
    capped = st.crossings(pos.copy(), d, ceiling, max_steps=5, capacity=8)
    same_bits(st.traverse(pos.copy(), d, ceiling, max_steps=5), capped)
    invariants(full)
    invariants(capped)
    assert (capped["n_crossings"] <= full["n_crossings"]).all()
    assert (capped["n_crossings"] < full["n_crossings"]).any()


def test_exit_points_example(tmp_path):
    exe = str(tmp_path / "exit_points")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "exit_points.c"), "-o", exe,
                           "-L" + os.path.dirname(TA.library_path()), "-lturtle_amd",
                           "-Wl,-rpath," + os.path.dirname(TA.library_path()), "-lm"])
    tile = TC.write_tile(tmp_path, "rough")
    out = subprocess.run([exe, tile], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    lat0, lon0 = (float(v) for v in lines[0].split()[1:3])
    rows = [l.split() for l in lines if l.startswith("ray")]
    assert len(rows) > 20 and any(r[10] == "exit" and r[11] != "none" for r in rows)
    # the same fan through the binding
    TA.set_math("fast")
    m = TA.Map.load(tile)
    st = TA.Stepper()
    st.add_map(m, 0.0)
    try:
        r = np.arange(216)
        az, el = 360.0 * (r % 36) / 36, 25.0 * (r // 36) / 6
        lat, lon = np.full(216, lat0), np.full(216, lon0)
        pos, _ = st.position(lat, lon, np.full(216, 0.5))
        t = st.crossings(pos, TA.ecef_from_horizontal(lat, lon, az, el), 2000.0, capacity=64)
        for row in rows:
            ray = int(row[1])
            kept = min(int(t["n_crossings"][ray]), 64)
            media = t["media"][:kept, ray]
            entry = int(np.flatnonzero(media[:, 1] == 0)[0])
            la, lo, al = TA.ecef_to_geodetic(t["point"][entry, ray][None])
            assert abs(float(row[7]) - la[0]) < 1e-8 and abs(float(row[8]) - lo[0]) < 1e-8
            assert abs(float(row[9]) - al[0]) < 1e-3
            leave = np.flatnonzero(media[:, 0] == 0)
            if row[11] != "none":
                la, lo, al = TA.ecef_to_geodetic(t["point"][leave[-1], ray][None])
                assert abs(float(row[11]) - la[0]) < 1e-8 and abs(float(row[12]) - lo[0]) < 1e-8
                assert abs(float(row[13]) - al[0]) < 1e-3
            else:
                assert leave.size == 0 or leave[-1] <= entry
    finally:
        st.destroy()
        m.destroy()
