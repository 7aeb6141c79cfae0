"""turtle_map_resample on the GPU: maps filled from a stack or from another map, against the
reference's loop (tests/golden/resample.npz) and the CPU checker (tests/resample_cases.py).

The bar: every code equal.  A code that differs is classified mechanically: it may only be a node
whose checker value (z - z0)/dz lies within 1e-6 of a half-integer, where the last ulp of OCML's
projection trig can decide the rounding, and every such node is named in HALFWAY.  There are
none."""
import ctypes as C
import os
import struct
import subprocess
import time
import zlib

import numpy as np
import pytest

import turtle_amd as TA
from turtle_amd import synth

import resample_cases as RC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALFWAY = {}  # case -> [(ix, iy), ...] whose code may differ by the rounding of a half-integer
D = C.c_double


@pytest.fixture(scope="module")
def tiles(tmp_path_factory):
    base = tmp_path_factory.mktemp("resample")
    return {which: RC.tile_dir(base, which) for which in ("ground", "void")}


def case_map(case, codes=None):
    nx, ny, x, y, z, proj, _ = RC.CASES[case]
    out = TA.Map.create(shape=(ny, nx), x=x, y=y, z=z, projection=proj)
    m = RC.meta(case)
    codes = RC.sentinel(nx, ny) if codes is None else codes
    fill = TA.lib().turtle_map_fill
    for iy in range(ny):
        for ix in range(nx):
            assert fill(out.h, ix, iy, D(m["z0"] + int(codes[iy, ix]) * m["dz"])) == 0
    return out


def node_codes(mp, m, signed=False):
    """the codes through turtle_map_node"""
    node = TA.lib().turtle_map_node
    z = D()
    out = np.empty((m["ny"], m["nx"]), dtype=np.float64)
    for iy in range(m["ny"]):
        for ix in range(m["nx"]):
            assert node(mp.h, ix, iy, None, None, C.byref(z)) == 0
            out[iy, ix] = z.value
    if signed:
        return out.astype(np.int16).view(np.uint16)
    return np.rint((out - m["z0"]) / m["dz"]).astype(np.uint16)


def dump_codes(mp, path):
    """the codes through turtle_map_dump (a PNG of filter-0 rows, north first: dump.c)"""
    mp.dump(str(path))
    raw = open(str(path), "rb").read()
    at, idat, head = 8, b"", None
    while at < len(raw):
        n, kind = struct.unpack(">I4s", raw[at:at + 8])
        if kind == b"IHDR":
            head = struct.unpack(">II", raw[at + 8:at + 16])
        elif kind == b"IDAT":
            idat += raw[at + 8:at + 8 + n]
        at += 12 + n
    w, h = head
    rows = np.frombuffer(zlib.decompress(idat), dtype=np.uint8).reshape(h, 1 + 2 * w)
    assert not rows[:, 0].any()
    return rows[:, 1:].copy().view(">u2").astype(np.uint16)[::-1]


def checker(case, g):
    m = RC.meta(case)
    if m["source"] in ("stack", "void"):
        geo = RC.ground_oracle() if m["source"] == "stack" else RC.void_oracle()
        z, inside = RC.check(m, stack=geo)
    else:
        sm = RC.meta(m["source"])
        z, inside = RC.check(m, source=RC.map_oracle(sm, g[f"{m['source']}_codes"]), source_meta=sm)
    return z, inside


def assert_codes(case, got, want, z, inside, m):
    diff = np.argwhere(got != want)
    named = set(HALFWAY.get(case, []))
    half = RC.halfway(z, m["z0"], m["dz"]) & inside
    for iy, ix in diff:
        assert half[iy, ix], f"{case}: node ({ix}, {iy}) differs and is not a half-integer case"
    assert {(int(ix), int(iy)) for iy, ix in diff} == named, f"{case}: {len(diff)} codes differ"


@pytest.mark.parametrize("case", ["a", "b", "c", "d", "e"])
def test_golden_cases(tiles, golden, case):
    g = golden("resample")
    m = RC.meta(case)
    mp = case_map(case)
    stack, src = None, None
    try:
        if m["source"] == "stack":
            stack = TA.Stack(tiles["ground"], 0)
            outside, clamped = mp.resample(stack=stack)
        else:
            src = case_map(m["source"], g[f"{m['source']}_codes"])
            outside, clamped = mp.resample(source=src)
        got = node_codes(mp, m)
        assert outside == int(g[f"{case}_outside"].sum()) and clamped == 0
        # outside nodes keep the sentinel written before the call
        out = g[f"{case}_outside"]
        assert np.array_equal(got[out], RC.sentinel(m["nx"], m["ny"])[out])
        z, inside = checker(case, g)
        assert np.array_equal(~inside, out)
        assert_codes(case, got, g[f"{case}_codes"], z, inside, m)
    finally:
        mp.destroy()
        if stack is not None:
            stack.destroy()
        if src is not None:
            src.destroy()


def test_full_size(tmp_path):
    """a 4000^2 Lambert 93 map at 25 m over a 2 x 2 stack of 3601^2 tiles, against the checker"""
    d = str(tmp_path / "srtm")
    for la in (45, 46):
        for lo in (2, 3):
            synth.write_hgt(d, la, lo)
    n = 4000
    x0, y0 = 650000.0, 6494500.0
    m = dict(nx=n, ny=n, x0=x0, y0=y0, dx=(n - 1) * 25.0 / (n - 1), dy=(n - 1) * 25.0 / (n - 1),
             z0=0.0, dz=2000.0 / 65535, projection="Lambert 93")
    mp = TA.Map.create(shape=(n, n), x=(x0, x0 + (n - 1) * 25.0), y=(y0, y0 + (n - 1) * 25.0),
                       z=(0.0, 2000.0), projection="Lambert 93")
    stack = TA.Stack(d, 0)
    try:
        stack.load()
        mp.resample(stack=stack)  # (tiles in HBM)
        t = time.perf_counter()
        outside, clamped = mp.resample(stack=stack)
        dt = time.perf_counter() - t
        print(f"full size: {n * n} nodes in {dt * 1e3:.1f} ms, {n * n / dt:.3e} nodes/s")
        assert outside == 0 and clamped == 0
        got = dump_codes(mp, tmp_path / "full.png")
        geo = RC.mosaic([(45, 2), (45, 3), (46, 2), (46, 3)],
                        lambda la, lo: synth.srtm_like_nodes(la, lo, synth.HGT_N))
        z, inside = RC.check(m, stack=geo)
        assert inside.all()
        want, ok, _ = RC.expected(m, z, inside, np.zeros((n, n), dtype=np.uint16))
        assert ok.all()
        assert_codes("full", got, want, z, inside, m)
    finally:
        mp.destroy()
        stack.destroy()


@pytest.mark.parametrize("size", [1, 2])
def test_paged_stack_gives_the_resident_codes(tiles, tmp_path, size):
    resident = TA.Stack(tiles["ground"], 0)
    paged = TA.Stack(tiles["ground"], size)
    maps = []
    try:
        for case in ("a", "c"):
            m = RC.meta(case)
            one, two = case_map(case), case_map(case)
            maps += [one, two]
            assert one.resample(stack=resident) == two.resample(stack=paged)
            assert paged.resident <= size
            assert np.array_equal(dump_codes(one, tmp_path / "r.png"), dump_codes(two, tmp_path / "p.png"))
            assert np.array_equal(dump_codes(two, tmp_path / "p.png"), node_codes(two, m))
    finally:
        for mp in maps:
            mp.destroy()
        resident.destroy()
        paged.destroy()


def test_math_mode_changes_no_bit(tiles, golden, tmp_path):
    g = golden("resample")
    stack = TA.Stack(tiles["ground"], 0)
    out = {}
    try:
        for mode in ("strict", "fast"):
            TA.set_math(mode)
            a = case_map("a")
            a.resample(stack=stack)
            d = case_map("d")
            d.resample(source=a)
            out[mode] = (dump_codes(a, tmp_path / "a.png"), dump_codes(d, tmp_path / "d.png"))
            a.destroy()
            d.destroy()
    finally:
        TA.set_math("fast")
        stack.destroy()
    assert np.array_equal(out["strict"][0], out["fast"][0])
    assert np.array_equal(out["strict"][1], out["fast"][1])
    assert np.array_equal(out["fast"][0], g["a_codes"])


def test_span_errors_change_nothing_and_clamp(tiles, golden):
    g = golden("resample")
    m = RC.meta("f")
    mp = case_map("f")
    stack = TA.Stack(tiles["void"], 0)
    x, y = RC.nodes_xy(m)
    x, y = x.ravel(), y.ravel()
    try:
        before = node_codes(mp, m)
        z_before, in_before = mp.elevation(x, y)  # (and an HBM copy that must not change)
        with pytest.raises(TA.TurtleError) as e:
            mp.resample(stack=stack)
        assert e.value.name == "DOMAIN_ERROR" and "elevation is outside of map span" in str(e.value)
        assert np.array_equal(node_codes(mp, m), before)
        z_after, in_after = mp.elevation(x, y)
        assert np.array_equal(z_after, z_before) and np.array_equal(in_after, in_before)
        outside, clamped = mp.resample(stack=stack, clamp=True)
        assert outside == 0 and clamped == int(g["f_refused"].sum())
        got = node_codes(mp, m)
        z, inside = checker("f", g)
        want, _, _ = RC.expected(m, z, inside, before, clamp=True)
        assert np.array_equal(want, g["f_clamped_codes"])
        assert_codes("f", got, want, z, inside, m)
    finally:
        mp.destroy()
        stack.destroy()


def test_argument_errors_change_nothing(tiles):
    L = TA.lib()
    m = RC.meta("a")
    mp, src = case_map("a"), case_map("e")
    stack = TA.Stack(tiles["ground"], 0)
    try:
        before = node_codes(mp, m)

        def call(target, st, source, flags=0):
            rc = L.turtle_map_resample(target, st, source, flags, None, None)
            TA.binding._pending.clear()
            return TA.binding.RETURN_NAMES[rc]

        assert call(None, stack.h, None) == "BAD_ADDRESS"
        assert call(mp.h, None, None) == "BAD_ADDRESS"
        assert call(mp.h, stack.h, src.h) == "DOMAIN_ERROR"
        assert call(mp.h, None, mp.h) == "DOMAIN_ERROR"
        assert call(mp.h, stack.h, None, flags=4) == "DOMAIN_ERROR"
        assert np.array_equal(node_codes(mp, m), before)
    finally:
        mp.destroy()
        src.destroy()
        stack.destroy()


def test_readers_see_the_new_nodes(tiles, golden, tmp_path):
    """turtle_map_elevation_n, the host scalar path, dump / load, and a stepper that held the
    map before the call"""
    g = golden("resample")
    m = RC.meta("a")
    mp = case_map("a")
    stack = TA.Stack(tiles["ground"], 0)
    st = TA.Stepper()
    st.add_map(mp, 0.0)
    lat, lon, az, el = synth.uniform_rays(2000, (45.95, 46.15), (2.85, 3.1), seed=7)
    d = TA.ecef_from_horizontal(lat, lon, az, el)
    try:
        pos0, di = st.position(lat, lon, 300.0)
        st.trace(pos0.copy(), d)  # the stepper's tables hold the old copy now
        mp.resample(stack=stack)
        codes = g["a_codes"]
        assert np.array_equal(node_codes(mp, m), codes)
        # batch and scalar lookups against the oracle over the new codes
        rng = np.random.default_rng(3)
        x = m["x0"] + rng.random(5000) * (m["nx"] - 1) * m["dx"]
        y = m["y0"] + rng.random(5000) * (m["ny"] - 1) * m["dy"]
        zo, io = RC.map_oracle(m, codes).grid_elevation(0, x, y)
        z, inside = mp.elevation(x, y)
        assert inside.all() and np.array_equal(z, zo)
        TA.set_scalar("host")
        try:
            zs = np.array([mp.elevation_scalar(x[k], y[k])[0] for k in range(200)])
        finally:
            TA.set_scalar("device")
        assert np.array_equal(zs, zo[:200])
        # dump -> load
        path = str(tmp_path / "a.png")
        mp.dump(path)
        fresh = TA.Map.load(path)
        assert np.array_equal(node_codes(fresh, m), codes)
        # the stepper that held the map traces as one built on a fresh map of the new codes
        st2 = TA.Stepper()
        st2.add_map(fresh, 0.0)
        p1, d1 = st.position(lat, lon, 300.0)
        p2, d2 = st2.position(lat, lon, 300.0)
        assert np.array_equal(p1, p2) and np.array_equal(d1, d2)
        assert not np.array_equal(p1, pos0)  # the ground moved
        t1, t2 = st.trace(p1.copy(), d), st2.trace(p2.copy(), d)
        for k in ("index", "length", "n_steps"):
            assert np.array_equal(t1[k], t2[k]), k
        st2.destroy()
        fresh.destroy()
    finally:
        st.destroy()
        mp.destroy()
        stack.destroy()


def test_odd_shapes(tiles, tmp_path):
    geo = RC.ground_oracle()
    stack = TA.Stack(tiles["ground"], 0)
    shapes = [(1, 1, (2.6, 2.6), (45.5, 45.5), None), (1000, 1, (2.1, 3.9), (45.7, 45.7), None),
              (13, 9, (690000.0, 702000.0), (6540000.0, 6548000.0), "Lambert 93"),
              (1, 1000, (700000.0, 700000.0), (6480000.0, 6600000.0), "Lambert 93")]
    try:
        for nx, ny, x, y, proj in shapes:
            mp = TA.Map.create(shape=(ny, nx), x=x, y=y, z=(0.0, 2000.0), projection=proj)
            m = dict(nx=nx, ny=ny, x0=x[0], y0=y[0], dx=(x[1] - x[0]) / (nx - 1) if nx > 1 else 0.0,
                     dy=(y[1] - y[0]) / (ny - 1) if ny > 1 else 0.0, z0=0.0, dz=2000.0 / 65535,
                     projection=proj)
            outside, _ = mp.resample(stack=stack)
            z, inside = RC.check(m, stack=geo)
            want, _, _ = RC.expected(m, z, inside, np.zeros((ny, nx), dtype=np.uint16))
            assert outside == int((~inside).sum())
            assert_codes(f"{nx}x{ny}", node_codes(mp, m), want, z, inside, m)
            mp.destroy()
        # a signed (HGT) target loaded from a tile file: codes are (int16)z
        tile = TA.Map.load(synth.write_hgt(str(tmp_path / "one"), 45, 2, RC.N))
        meta = tile.meta()
        m = dict(nx=meta["nx"], ny=meta["ny"], x0=meta["x"][0], y0=meta["y"][0],
                 dx=1.0 / (RC.N - 1), dy=1.0 / (RC.N - 1), z0=-32767.0, dz=1.0, projection=None)
        before = node_codes(tile, m, signed=True)
        outside, clamped = tile.resample(stack=stack)
        z, inside = RC.check(m, stack=geo)
        # the tile's north-east corner node is 46N 3E: the missing tile answers there
        assert outside == int((~inside).sum()) == 1 and not inside[-1, -1] and clamped == 0
        want, _ = RC.quantise(z, m["z0"], m["dz"], signed=True)
        got = node_codes(tile, m, signed=True)
        assert np.array_equal(got, np.where(inside, want, before))
        assert not np.array_equal(got, before)
        tile.destroy()
    finally:
        stack.destroy()


def test_projection_map_example(tiles, tmp_path):
    exe = str(tmp_path / "projection_map")
    subprocess.check_call(["gcc", "-O2", "-std=c99", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "projection_map.c"), "-o", exe,
                           "-L" + os.path.dirname(TA.library_path()), "-lturtle_amd",
                           "-Wl,-rpath," + os.path.dirname(TA.library_path()), "-lm"])
    png = str(tmp_path / "pdd.png")
    out = subprocess.run([exe, tiles["ground"], png], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    assert "40401 nodes: 0 outside the data" in out.stdout
    mp = TA.Map.create(shape=(201, 201), x=(693530.7, 699530.7), y=(6515284.5, 6521284.5),
                       z=(500.0, 1500.0), projection="Lambert 93")
    stack = TA.Stack(tiles["ground"], 0)
    try:
        outside, clamped = mp.resample(stack=stack, clamp=True)
        assert f"{clamped} clamped" in out.stdout
        loaded = TA.Map.load(png)
        assert loaded.meta()["projection"] == "Lambert 93"
        assert np.array_equal(dump_codes(loaded, tmp_path / "again.png"), dump_codes(mp, tmp_path / "mine.png"))
        loaded.destroy()
    finally:
        mp.destroy()
        stack.destroy()
