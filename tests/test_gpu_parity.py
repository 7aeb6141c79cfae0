"""Parity of the HIP path (through the C ABI) with the reference.

Three checkers, in decreasing authority:
  * tests/golden/*.npz -- outputs of the real reference on stored inputs;
  * the CPU restatement (oracle/), itself pinned bit-for-bit to those;
  * size-independent properties at the BASELINE sizes (test_gpu_properties).

Bar (BASELINE.json north_star): identical medium index, path length within
1e-6 relative.  Integer/byte work (node decode, tile selection, inside flags)
is bit-exact.  Transcendentals come from OCML instead of glibc, so floating
outputs may differ in the last ulp: tolerances are written at each assert.
"""
import os

import numpy as np
import pytest

import turtle_amd as TA
from oracle import ffi as O

import amd_build as B
import terrains as T
from turtle_amd import synth

pytestmark = pytest.mark.gpu

REL = 1e-6  # the parity bar on path length


@pytest.fixture(params=["fast", "strict"])
def math(request):
    """Both arithmetic variants of the trace kernel must meet the same bar."""
    TA.set_math(request.param)
    yield request.param
    TA.set_math("fast")


def check_trace(t, ref_index, ref_length, ref_nsteps, what, allow=0):
    """identical medium; |dL|/L <= 1e-6; report grazing mismatches."""
    idx = np.asarray(t["index"])
    bad = np.flatnonzero((idx[:, 0] != ref_index[:, 0]))
    assert bad.size <= allow, f"{what}: {bad.size} rays changed medium: {bad[:10]}"
    ok = np.ones(idx.shape[0], dtype=bool)
    ok[bad] = False
    L, L0 = np.asarray(t["length"])[ok], ref_length[ok]
    rel = np.abs(L - L0) / np.maximum(np.abs(L0), 1e-300)
    rel[L0 == 0] = np.abs(L[L0 == 0])
    assert rel.max() <= REL, f"{what}: path length off by {rel.max():.3e}"
    # data index and step count: equal except where a last-ulp difference
    # moves a sample across a cell edge or a bisection bracket by one
    ds = np.abs(np.asarray(t["n_steps"])[ok] - ref_nsteps[ok])
    # (logged on C2: 3 rays of a million; the allowance is a ten-thousandth of the rays, at least one)
    assert (ds <= 1).all() and (ds != 0).sum() <= max(1, int(1e-4 * ds.size)), \
        f"{what}: step counts differ on {int((ds != 0).sum())} rays of {ds.size}"
    return rel.max()


def test_fast_transform_accuracy(golden):
    """The fast-math ECEF->geodetic of the trace kernel, exposed through
    turtle_ecef_to_geodetic_n: a few ulp from the reference everywhere (both
    branches of the latitude formula, poles, axis, 100 km up, 10 km down)."""
    g = golden("ecef")
    TA.set_math("fast")
    try:
        la, lo, al = TA.ecef_to_geodetic(g["ecef_all"])
    finally:
        TA.set_math("fast")
    ok = np.isfinite(g["to_alt"])
    dlat = np.abs(la - g["to_lat"])[ok]
    dlon = np.abs(lo - g["to_lon"])[ok]
    dalt = np.abs(al - g["to_alt"])[ok]
    print(f"fast transform: max |dlat| {dlat.max():.2e} deg, |dlon| {dlon.max():.2e} deg, "
          f"|dalt| {dalt.max():.2e} m")
    assert dlat.max() < 5e-14 and dalt.max() < 6e-9
    # longitude is ill-conditioned only within ~1e-300 m of the axis
    far = np.hypot(g["ecef_all"][:, 0], g["ecef_all"][:, 1])[ok] > 1e-3
    assert dlon[far].max() < 1e-13  # 2-3 ulp at |lon| ~ 180
    assert la[-7] == 90.0 and lo[-7] == 0.0 and la[-6] == -90.0  # exact poles


def test_ecef_known_answers(golden):
    TA.set_math("strict")
    g = golden("ecef")
    e = TA.ecef_from_geodetic(g["lat"], g["lon"], g["alt"])
    # sin/cos of OCML vs glibc: 1-2 ulp of 6.4e6 m
    assert np.abs(e - g["ecef"]).max() < 5e-9
    la, lo, al = TA.ecef_to_geodetic(g["ecef_all"])
    assert np.abs(la - g["to_lat"]).max() < 1e-13 * 90
    assert np.abs(lo - g["to_lon"]).max() < 1e-13 * 180
    assert np.abs(al - g["to_alt"]).max() < 5e-9
    # exact special cases [ref ecef.c:77-84]: the last rows of ecef_all
    assert la[-7] == 90.0 and lo[-7] == 0.0 and la[-6] == -90.0
    assert al[-7] == g["to_alt"][-7] and al[-5] == g["to_alt"][-5]
    d = TA.ecef_from_horizontal(g["lat"], g["lon"], g["az"], g["el"])
    assert np.abs(d - g["direction"]).max() < 1e-15 * 4
    az, el = TA.ecef_to_horizontal(g["lat"], g["lon"], g["dir_scaled"])
    daz = np.abs(az - g["to_az"])
    daz = np.minimum(daz, 360 - daz)
    # azimuth is ill-conditioned near the zenith/nadir: scale by 1/cos(el)
    assert (daz * np.cos(np.radians(g["to_el"])) < 1e-11).all()
    # asin near +-1 amplifies an ulp of its argument by 1/cos(el)
    assert (np.abs(el - g["to_el"]) * np.maximum(np.cos(np.radians(g["to_el"])), 1e-8)
            < 1e-11).all()
    assert az[5] == 0.0 and el[5] == 0.0  # null direction: untouched
    TA.set_math("fast")


def test_ecef_reference_assertions():
    """tests/test-turtle.c:582-625 through the SCALAR drop-in calls."""
    from turtle_amd import binding as Bn
    p = Bn.scalar_ecef_from_geodetic(45.5, 3.5, 1000.0)
    la, lo, al = Bn.scalar_ecef_to_geodetic(p)
    assert abs(la - 45.5) < 1e-8 and abs(lo - 3.5) < 1e-8 and abs(al - 1000) < 1e-8
    la, lo, al = Bn.scalar_ecef_to_geodetic([0.0, 0.0, 6356752.3142 + 1000.0])
    assert la == 90.0 and lo == 0.0 and abs(al - 1000.0) < 1e-9
    p = Bn.scalar_ecef_from_geodetic(0.0, 90.0, 1000.0)
    la, lo, al = Bn.scalar_ecef_to_geodetic(p)
    assert la == 0.0 and lo == 90.0 and abs(al - 1000) < 1e-8


def test_bilinear_bit_exact(golden):
    g = golden("bilinear")
    m = B.c1_map()
    z, inside = m.elevation(g["x"], g["y"])
    assert np.array_equal(inside, g["inside"])
    ok = inside == 1
    assert np.array_equal(z[ok], g["z"][ok])  # +,-,*,/ only: bit-exact
    for ix, iy, xyz in zip(g["node_ix"], g["node_iy"], g["node_xyz"]):
        assert m.node(int(ix), int(iy)) == tuple(xyz)
    # scalar drop-in: outside leaves *elevation untouched; inside==NULL raises
    zz, ii = m.elevation_scalar(3.5, 45.5)
    k = 0
    assert ii == 1
    zz, ii = m.elevation_scalar(2.0, 45.5)
    assert ii == 0 and zz == -12345.0
    with pytest.raises(TA.TurtleError) as e:
        m.elevation_scalar(2.0, 45.5, want_inside=False)
    assert e.value.name == "DOMAIN_ERROR" and "point is outside of map" in str(e.value)
    m.destroy()


def test_c1_traces(golden, math):
    g = golden("c1_traces")
    m = B.c1_map()
    st = B.c1_stepper(m)
    pos, di = st.position(g["lat"], g["lon"], 500.0)
    assert (di == 0).all() and np.abs(pos - g["position"]).max() < 5e-9
    t = st.trace(g["position"].copy(), g["direction"])
    check_trace(t, g["r0_index"], g["r0_length"], g["r0_n_steps"], "C1 vs reference range=0")
    # the reference's default (local_range = 1) differs from it by ~1e-9 only
    check_trace(t, g["r1_index"], g["r1_length"], g["r1_n_steps"], "C1 vs reference range=1")
    # end points: rays that skim the ground for thousands of steps amplify any
    # 1e-9 m difference in a sample (libm vs OCML already gives 6e-6 m in strict
    # arithmetic); 5e-5 m over paths of kilometres is 1e-8 relative, the bar is 1e-6
    assert np.abs(t["position"] - g["r0_position"]).max() < (5e-5 if math == "fast" else 1e-5)
    s = st.trace_stats()
    assert s["rays"] == 1000 and s["steps"] == int(np.sum(t["n_steps"])) and s["capped"] == 0
    assert 1.0 < s["samples"] / s["steps"] < 1.2  # ~1.05 samples per step
    st.destroy()
    m.destroy()


def test_c1_per_step_records(golden):
    """G7: every step of 16 rays (position, ds, index) against the reference."""
    g = golden("steps")
    m = B.c1_map()
    st = B.c1_stepper(m)
    rec = g["record"]
    pos = g["position"].copy()
    direction = g["direction"]
    alive = np.ones(16, dtype=bool)
    for k in range(1, int(rec[:, 1].max()) + 1):
        rows = rec[rec[:, 1] == k]
        rays = rows[:, 0].astype(int)
        o = st.step(pos[rays].copy(), direction[rays])
        assert np.array_equal(o["index"], rows[:, 6:8].astype(np.int32))
        assert np.abs(o["step"] - rows[:, 5]).max() <= 1e-6 * np.abs(rows[:, 5]).max()
        assert np.abs(o["position"] - rows[:, 2:5]).max() < 1e-5
        pos[rays] = o["position"]
    st.destroy()
    m.destroy()


def test_hgt_tile_traces(golden, tmp_path, math):
    g = golden("hgt_traces")
    m = B.hgt_tile(tmp_path)
    for ix, iy, z in zip(g["node_ix"][:64], g["node_iy"][:64], g["node_z"][:64]):
        assert m.node(int(ix), int(iy))[2] == z
    z, inside = m.elevation(g["qx"], g["qy"])
    assert np.array_equal(inside, g["qin"])
    assert np.array_equal(z[inside == 1], g["qz"][inside == 1])
    st = TA.Stepper()
    st.add_map(m, 0.0)
    pos, di = st.position(g["lat"], g["lon"], 500.0)
    assert np.abs(pos - g["position"]).max() < 5e-9
    t = st.trace(g["position"].copy(), g["direction"])
    worst = check_trace(t, g["r0_index"], g["r0_length"], g["r0_n_steps"],
                        "3601^2 tile vs reference")
    print(f"hgt 10k rays: worst relative path-length difference {worst:.2e}")
    st.destroy()
    m.destroy()


def test_scalar_calls_on_the_host_agree_with_the_kernels(golden, tmp_path):
    """turtle_amd_scalar_set(HOST): the drop-in scalar functions answered by the host restatement
    (csrc/scalar.c) give what the kernels give -- the strict kernels to the last ulp of OCML's
    trig, the fast ones at the parity bar -- over a map, two layers with a geoid, and a stack
    that pages; and the batch calls do not care about the option."""
    g = golden("c1_traces")
    m = B.c1_map()
    st = B.c1_stepper(m)
    sel = slice(0, 200)
    pos, d = g["position"][sel], g["direction"][sel]
    TA.set_math("strict")
    ref = st.trace(pos.copy(), d)
    try:
        TA.set_scalar("host")
        assert TA.get_scalar() == "host"
        again = st.trace(pos.copy(), d)          # a batch call: still the kernels
        for key in ("index", "n_steps", "length", "position"):
            assert np.array_equal(again[key], ref[key])
        for r in range(200):
            o = st.step_scalar(pos[r])
            medium, p, total, k = o["index"][0], o["position"], 0.0, 0
            while True:
                o = st.step_scalar(p, d[r])
                p, total, k = o["position"], total + o["step"], k + 1
                if o["index"][0] != medium or k >= 100000:
                    break
            assert o["index"][0] == ref["index"][r, 0] and k == ref["n_steps"][r]
            assert abs(total - ref["length"][r]) <= 1e-9 * ref["length"][r]
            assert np.abs(p - ref["position"][r]).max() < 1e-5
        # the reference's golden values, through the public scalar entry points
        p0, di = st.position_scalar(g["lat"][0], g["lon"][0], 500.0)
        assert np.array_equal(p0, g["position"][0]) and di == 0
        z, inside = m.elevation_scalar(3.5, 45.5)
        zk, ik = m.elevation(np.array([3.5]), np.array([45.5]))
        assert inside == 1 and z == zk[0]
    finally:
        TA.set_scalar("device")
        TA.set_math("fast")
    st.destroy()
    m.destroy()


def test_outputs_not_asked_for_change_nothing(math):
    """A caller that wants no path lengths or step counts gets the same media and end points, to
    the bit, from the same kernels (the trace's own counters say so) as one that wants them."""
    m = TA.Map.create(T.c1_nodes(), T.C1_X, T.C1_Y, T.C1_Z)
    st = B.c1_stepper(m)
    lat, lon, az, el = synth.uniform_rays(20000, T.C1_Y, T.C1_X, seed=77)
    pos, _ = st.position(lat, lon, 500.0)
    d = TA.ecef_from_horizontal(lat, lon, az, el)
    full = st.trace(pos.copy(), d)
    stats = st.trace_stats()
    for want in ((), ("length",), ("n_steps",)):
        t = st.trace(pos.copy(), d, want=want)
        assert t["length"] is None or np.array_equal(t["length"], full["length"])
        assert t["n_steps"] is None or np.array_equal(t["n_steps"], full["n_steps"])
        assert np.array_equal(t["index"], full["index"]) and np.array_equal(t["position"], full["position"])
        assert st.trace_stats() == stats, (want, st.trace_stats(), stats)
    st.destroy()
    m.destroy()


def test_c3_seams_of_full_size_tiles(golden, tmp_path, math):
    """C3's shape at full tile size: a stack of 3601^2 tiles, rays that start
    within 0.01 degree of a seam and cross it, run along it or leave through the rim --
    against the REFERENCE's own trace (G11), no ray set apart."""
    g = golden("c3_seam")
    stack = B.mosaic(tmp_path, [tuple(t) for t in g["tiles"]], synth.HGT_N)
    st = TA.Stepper()
    st.add_stack(stack, 0.0)
    pos, di = st.position(g["lat"], g["lon"], 300.0)
    assert (di == 0).all() and np.abs(pos - g["position"]).max() < 5e-9
    t = st.trace(g["position"].copy(), g["direction"])
    check_trace(t, g["t_index"], g["t_length"], g["t_n_steps"], "2x2 mosaic of 3601^2 tiles")
    assert np.abs(t["position"] - g["t_position"]).max() < 1e-5  # (paths of up to 20 km)
    # the same through a stack that pages: two tiles resident at a time
    paged = TA.Stack(str(tmp_path / "mosaic"), 2)
    sp = TA.Stepper()
    sp.add_stack(paged, 0.0)
    tp = sp.trace(g["position"].copy(), g["direction"])
    check_trace(tp, g["t_index"], g["t_length"], g["t_n_steps"], "the same, two tiles resident")
    assert sp.rounds > 1 and paged.resident <= 2
    sp.destroy()
    paged.destroy()
    st.destroy()
    stack.destroy()


def test_stack_directory(golden, tmp_path, math):
    g = golden("stack")
    n = int(g["n"])
    stack = B.mosaic(tmp_path, [tuple(t) for t in g["tiles"]], n)
    z, inside = stack.elevation(g["lat"], g["lon"])
    assert np.array_equal(inside, g["inside"])
    assert np.array_equal(z, g["z"])  # bit-exact, incl. 0 for outside/missing
    # scalar drop-in: missing tile with inside==NULL raises PATH_ERROR
    zz, ii = stack.elevation_scalar(46.5, 4.5)
    assert ii == 0 and zz == 0.0
    with pytest.raises(TA.TurtleError) as e:
        stack.elevation_scalar(46.5, 4.5, want_inside=False)
    assert e.value.name == "PATH_ERROR" and "missing elevation data" in str(e.value)
    st = TA.Stepper()
    st.add_stack(stack, 0.0)
    pos, di = st.position(g["ray_lat"], g["ray_lon"], 300.0)
    assert (di == 0).all() and np.abs(pos - g["position"]).max() < 5e-9
    t = st.trace(g["position"].copy(), g["direction"])
    check_trace(t, g["t_index"], g["t_length"], g["t_n_steps"], "2x2 mosaic")
    st.destroy()
    stack.destroy()
    one = B.mosaic(tmp_path / "one", [(45, 3)], n)
    z1, in1 = one.elevation(g["lat1"], g["lon1"])
    assert np.array_equal(in1, g["in1"]) and np.array_equal(z1, g["z1"])
    one.destroy()


def test_stack_rim_and_seams(tmp_path, math):
    """Samples hugging the mosaic's rim and the seams between its tiles, from both
    sides, 1e-12 to 1e-4 degree away (1e-7 m to 10 m): the stepper's answer --
    inside or not, which elevation -- is the reference's.  This is where a ray
    leaving the mosaic is bisected, and where the fast lookup hands over to the
    exact one (device.hip: kSeamGuard, kRimGuard)."""
    tiles = [(45, 3), (45, 4), (46, 3), (46, 4)]
    n = 1201  # the .hgt reader knows two sizes [ref io/hgt.c:98-104]
    stack = B.mosaic(tmp_path, tiles, n)
    geo = T.mosaic_oracle(tiles, n, 45, 3, 2, 2)
    st = TA.Stepper()
    st.add_stack(stack, 0.0)
    eps = np.array([1e-12, 1e-11, 1e-10, 1e-9, 1e-8, 1e-7, 1e-6, 1e-5, 1e-4])
    off = np.concatenate([-eps[::-1], eps])
    edges = np.array([45.0, 46.0, 47.0])
    along = np.linspace(45.03, 46.97, 23)
    lat, lon = [], []
    for e in edges:
        for o in off:
            lat += [np.full(along.size, e + o), along]          # horizontal line at lat = e + o
            lon += [along - 42.0, np.full(along.size, e - 42.0 + o)]  # vertical at lon = e - 42 + o
    lat, lon = np.concatenate(lat), np.concatenate(lon)
    # the corners too: both coordinates on an edge at once
    cl, co = np.meshgrid(edges, edges - 42.0)
    for o1 in off[::4]:
        for o2 in off[::4]:
            lat, lon = np.concatenate([lat, (cl + o1).ravel()]), np.concatenate([lon, (co + o2).ravel()])
    pos = O.ecef_from_geodetic(lat, lon, np.full(lat.size, 2500.0))
    mine = st.step(pos.copy(), None)
    ref = geo.step(pos)
    assert np.array_equal(mine["index"], ref["index"])
    inside = ref["index"][:, 0] >= 0
    assert inside.sum() > 0.4 * lat.size and (~inside).sum() > 0.2 * lat.size
    assert np.abs(mine["elevation"][inside] - ref["elevation"][inside]).max() < 1e-9
    # and one step from there: a ray that has left keeps answering "outside"
    d = TA.isotropic(lat.size, 7, 0, device=False)
    mine2 = st.step(mine["position"], d, resume=mine)
    ref2 = geo.step(ref["position"], d)
    same = mine2["index"][:, 0] == ref2["index"][:, 0]
    assert (~same).sum() == 0, np.flatnonzero(~same)[:10]
    ok = same & (ref2["index"][:, 0] >= 0)
    assert np.abs(mine2["step"][ok] - ref2["step"][ok]).max() < 1e-6 * ref2["step"][ok].max()
    st.destroy()
    stack.destroy()


@pytest.mark.parametrize("name", ["nogeoid", "geoid"])
def test_layers_offsets_flat_geoid(golden, name, math):
    g = golden("layers")
    m = B.c1_map()
    geoid = B.geoid_map(g["geoid_nodes"]) if name == "geoid" else None
    st = B.two_layer_stepper(m, geoid)
    P, D, Oq = g[name + "_P"], g[name + "_D"], g[name + "_O"]
    for slope in (0.4, 2.0):
        st.slope = slope
        for has_dir in (0, 1):
            sel = (Oq[:, 2] == slope) & (Oq[:, 1] == has_dir)
            if math == "fast":
                # start points placed EXACTLY on a surface (height == the other
                # layer's offset) are classified by the last ulp of the
                # altitude: only reference-order arithmetic reproduces that bit
                on_surface = ((Oq[:, 15] == 1) & (Oq[:, 16] == -0.5)) | \
                             ((Oq[:, 15] == 0) & (Oq[:, 16] == 0.5))
                sel &= ~on_surface
            ref = Oq[sel]
            o = st.step(P[sel].copy(), D[sel] if has_dir else None)
            assert np.array_equal(o["index"], ref[:, 12:14].astype(np.int32))
            assert np.abs(o["latitude"] - ref[:, 6]).max() < 1e-11
            assert np.abs(o["longitude"] - ref[:, 7]).max() < 1e-11
            # after a located boundary the end point sits anywhere in the 1e-8 m bracket
            assert np.abs(o["altitude"] - ref[:, 8]).max() < (5e-9 if math == "strict" else 3e-8)
            e = o["elevation"]
            big = np.abs(ref[:, 9:11]) > 1e300  # +-DBL_MAX sentinels: exact
            assert np.array_equal(e[big], ref[:, 9:11][big])
            assert np.abs(e[~big] - ref[:, 9:11][~big]).max() < 1e-9
            # the bisection stops at a 1e-8 m bracket; points placed exactly ON a
            # surface (height == layer offset) bracket it from whichever side a
            # last-ulp altitude difference puts them, so steps agree to a few
            # bracket widths there, and to 1e-6 relative everywhere else
            tol = np.maximum(1e-6 * np.abs(ref[:, 11]), 2e-8 if math == "strict" else 1e-7)
            assert (np.abs(o["step"] - ref[:, 11]) <= tol).all()
            assert np.abs(o["position"] - ref[:, 3:6]).max() < 1e-7
    st.slope = 0.4
    t = st.trace(g[name + "_tpos"].copy(), g[name + "_tdir"])
    check_trace(t, g[name + "_t_index"], g[name + "_t_length"], g[name + "_t_n_steps"],
                f"two layers ({name})")
    # continue through the next medium.  The rays now sit within 1e-8 m of the
    # boundary the bisection located, so -- like the reference, whose next step
    # starts from its cached sample -- the medium is carried over, not re-derived
    t2 = st.trace(g[name + "_t_position"].copy(), g[name + "_tdir"],
                  resume_index=g[name + "_t_index"])
    check_trace(t2, g[name + "_t2_index"], g[name + "_t2_length"], g[name + "_t2_n_steps"],
                f"two layers, second medium ({name})")
    if math == "strict":
        # reference-order arithmetic gives a bit-identical altitude, so even a
        # fresh start on the boundary re-derives the same medium
        t3 = st.trace(g[name + "_t_position"].copy(), g[name + "_tdir"])
        check_trace(t3, g[name + "_t2_index"], g[name + "_t2_length"],
                    g[name + "_t2_n_steps"], f"two layers, fresh restart ({name})")
    st.destroy()
    m.destroy()
    if geoid is not None:
        geoid.destroy()


def test_reference_stepper_layer_assertions():
    """tests/test-turtle.c:255-409 re-expressed with geodetic data, through the
    SCALAR drop-in entry points (turtle_stepper_step / _position)."""
    DBL_MAX = np.finfo(np.float64).max
    FLT_EPSILON = float(np.finfo(np.float32).eps)
    m = B.c1_map()
    st = B.two_layer_stepper(m)
    lat0, lon0 = 45.756546, 3.4485671
    values = np.zeros((2, 2))
    for i in range(2):
        p, di = st.position_scalar(lat0, lon0, -0.25, i)
        assert di == 0
        o = st.step_scalar(p, None)
        assert o["index"][0] == i and o["index"][1] == 0
        values[0][i] = o["altitude"]
        p, di = st.position_scalar(40.0, 10.0, -0.25, i)
        assert di == 1  # only the flat data holds that point
        o = st.step_scalar(p, None)
        assert o["index"][0] == i and o["index"][1] == 1
        values[1][i] = o["altitude"]
    off = (-0.5, 0.0)
    for i in range(2):
        assert abs((values[i][0] - off[0]) - (values[i][1] - off[1])) < FLT_EPSILON
    slope = st.slope
    assert slope == 0.4 and st.resolution == 1e-2 and st.range == 1.0
    p, di = st.position_scalar(lat0, lon0, 0.5, 1)
    o = st.step_scalar(p, None)  # above the top layer
    assert o["index"][0] == 2 and o["elevation"][1] == DBL_MAX
    assert abs(o["elevation"][0] - (values[0][1] + 0.25)) < FLT_EPSILON
    assert abs(o["step"] - 0.5 * slope) < FLT_EPSILON
    p, di = st.position_scalar(lat0, lon0, -0.1, 1)
    o = st.step_scalar(p, None)  # between the two surfaces
    assert list(o["index"]) == [1, 0]
    assert abs(o["elevation"][0] - (values[0][0] + 0.25)) < FLT_EPSILON
    assert abs(o["elevation"][1] - (values[0][1] + 0.25)) < FLT_EPSILON
    assert abs(o["step"] - 0.1 * slope) < FLT_EPSILON
    p, di = st.position_scalar(lat0, lon0, -0.5, 0)
    o = st.step_scalar(p, None)  # below everything
    assert list(o["index"]) == [0, 0] and o["elevation"][0] == -DBL_MAX
    assert abs(o["step"] - 0.5 * slope) < FLT_EPSILON
    # boundary location: vertical ray from 0.1 m below the top surface
    p, di = st.position_scalar(lat0, lon0, -0.1, 1)
    up = TA.ecef_from_horizontal([lat0], [lon0], [0.0], [90.0])[0]
    st.slope = 2.0
    o = st.step_scalar(p, up)
    assert list(o["index"]) == [2, 0]
    assert abs(o["altitude"] - (values[0][1] + 0.25)) < 1e-5 and abs(o["step"] - 0.1) < 1e-5
    o2 = st.step_scalar(o["position"], up)  # next step from the boundary
    assert list(o2["index"]) == [2, 0] and abs(o2["step"] - st.resolution) < 1e-5
    # idempotent sampling: two dir=NULL calls are bit-identical [ref :822-838]
    a, b = st.step_scalar(p, None), st.step_scalar(p, None)
    for k in ("latitude", "longitude", "altitude", "step"):
        assert a[k] == b[k]
    assert np.array_equal(a["elevation"], b["elevation"])
    st.destroy()
    m.destroy()


def test_reference_stepper_exit_and_outside(tmp_path):
    """tests/test-turtle.c:852-858, :872-883, :923-931 re-expressed."""
    m = B.c1_map()
    st = TA.Stepper()
    st.add_map(m, 0.0)
    p, di = st.position_scalar(45.0, 90.0, 0.0, 0, initial=(1.0, 2.0, 3.0))
    assert di == -1 and list(p) == [1.0, 2.0, 3.0]  # untouched
    with pytest.raises(TA.TurtleError) as e:
        st.position_scalar(45.0, 90.0, 0.0, 0, want_index=False)
    assert e.value.name == "DOMAIN_ERROR" and "no valid data" in str(e.value)
    with pytest.raises(TA.TurtleError):
        st.position_scalar(45.5, 3.5, 0.0, 3)  # no such layer
    # horizontal ray leaves the map in < 100000 steps with index[0] < 0
    p, di = st.position_scalar(45.5, 3.5, -0.5, 0)
    d = TA.ecef_from_horizontal([45.5], [3.5], [0.0], [0.0])[0]
    t = st.trace(p[None, :].copy(), d[None, :], max_steps=100000)
    assert t["index"][0, 0] == 1  # first it surfaces (medium 0 -> 1)
    # it now sits on the surface it located: carry the medium over, as the
    # reference's cached sample does, instead of re-deriving it there
    t = st.trace(t["position"], d[None, :], max_steps=100000, resume_index=t["index"])
    assert t["index"][0, 0] == -1 and t["n_steps"][0] < 100000
    # far away: index = {-1, -1}, elevation = {0, 0}, step 0
    far = t["position"][0] + d * 1e6
    o = st.step_scalar(far, None)
    assert list(o["index"]) == [-1, -1] and list(o["elevation"]) == [0.0, 0.0]
    assert o["step"] == 0.0
    with pytest.raises(TA.TurtleError) as e:
        st.step_scalar(far, None, want_index=False)
    assert e.value.name == "DOMAIN_ERROR"
    st.destroy()
    m.destroy()


def test_resume_flag_matches_fresh_sample():
    m = B.c1_map()
    st = B.c1_stepper(m)
    lat, lon, az, el = TA.synth.uniform_rays(512, T.C1_Y, T.C1_X, seed=11)
    pos, _ = st.position(lat, lon, 400.0)
    d = TA.ecef_from_horizontal(lat, lon, az, el)
    a = st.step(pos.copy(), None)            # sample only
    b = st.step(pos.copy(), d)               # fresh: samples the start itself
    c = st.step(pos.copy(), d, resume=a)     # resumes from the returned sample
    for k in ("position", "altitude", "elevation", "index", "step"):
        assert np.array_equal(np.asarray(b[k]), np.asarray(c[k])), k
    st.destroy()
    m.destroy()


def test_tally_exact():
    rng = np.random.default_rng(5)
    n = 100000
    index = np.stack([rng.integers(-1, 3, n), np.zeros(n, dtype=np.int64)], 1).astype(np.int32)
    length = rng.uniform(0, 70000, n)
    length[:5] = [0.0, 65536.0, 65535.999, np.nan, -1.0]
    hits, hist = TA.tally(index, length, 3, 1024, 65536.0)
    assert np.array_equal(hits, np.bincount(index[:, 0] + 1, minlength=4))
    t = length * (1024 / 65536.0)
    b = np.full(n, 1024)
    okk = (t >= 0) & (t < 1024)
    b[okk] = t[okk].astype(np.int64)
    assert np.array_equal(hist, np.bincount(b, minlength=1025))
    hits2, hist2 = TA.tally(index, length, 3, 1024, 65536.0, hits, hist)  # accumulates
    assert hits2.sum() == 2 * n and hist2.sum() == 2 * n


def test_oracle_agrees_on_fresh_rays(math):
    """Seeded rays that are NOT in the fixtures: GPU vs the CPU restatement."""
    geo = T.c1_oracle()
    m = B.c1_map()
    st = B.c1_stepper(m)
    lat, lon, az, el = TA.synth.uniform_rays(4096, T.C1_Y, T.C1_X, seed=77)
    pos0, _ = geo.position(lat, lon, 500.0)
    d = O.ecef_from_horizontal(lat, lon, az, el)
    ref = geo.trace(pos0, d, threads=4)
    t = st.trace(pos0.copy(), d)
    check_trace(t, ref["index"], ref["length"], ref["n_steps"], "fresh rays vs oracle")
    # max_steps cap and zero-step edge cases
    t = st.trace(pos0.copy(), d, max_steps=7)
    r7 = geo.trace(pos0, d, max_steps=7)
    assert np.array_equal(t["n_steps"], r7["n_steps"]) and np.array_equal(t["index"], r7["index"])
    t = st.trace(pos0[:3].copy(), d[:3], max_steps=0)
    assert (t["n_steps"] == 0).all() and (t["index"][:, 0] == 1).all()
    e = st.trace(np.zeros((0, 3)), np.zeros((0, 3)))  # empty batch
    assert e["index"].shape == (0, 2)
    st.destroy()
    m.destroy()


def test_degenerate_inputs(math):
    """What no harness should send and some will: NaN and infinite coordinates, the
    centre of the Earth, the poles, a point 10^9 m away, zero / NaN / non-unit /
    reversed directions -- and batches that do not fill a wave.  Same answers as
    the reference's arithmetic (the CPU restatement), and every call returns."""
    geo = T.c1_oracle()
    m = B.c1_map()
    st = B.c1_stepper(m)
    n = 12
    lat, lon = np.full(n, 45.5), np.full(n, 3.5)
    pos, _ = geo.position(lat, lon, 500.0)
    d = O.ecef_from_horizontal(lat, lon, np.full(n, 30.0), np.full(n, -5.0))
    pos[1, 0] = np.nan
    pos[2, 1] = np.inf
    pos[3] = 0.0
    pos[4] = (0.0, 0.0, 6.4e6)
    pos[5] = (1e9, 1e9, 1e9)
    pos[10] = (0.0, 0.0, -6.4e6)
    d[6] = 0.0
    d[7, 2] = np.nan
    d[8] *= 1e6
    d[9] *= -1.0
    with np.errstate(all="ignore"):
        r0, r1 = geo.step(pos.copy()), geo.step(pos.copy(), d)
        rt = geo.trace(pos.copy(), d, max_steps=600)   # beyond 512: the per-ray lines too
    g0, g1 = st.step(pos.copy(), None), st.step(pos.copy(), d)
    gt = st.trace(pos.copy(), d, max_steps=600)
    assert np.array_equal(g0["index"], r0["index"]) and np.array_equal(g1["index"], r1["index"])
    assert np.array_equal(gt["index"], rt["index"]), (gt["index"], rt["index"])
    assert np.array_equal(gt["n_steps"], rt["n_steps"]), (gt["n_steps"], rt["n_steps"])
    ok = np.isfinite(r1["step"])
    assert np.array_equal(np.isfinite(g1["step"]), ok)
    assert np.abs(g1["step"][ok] - r1["step"][ok]).max() <= 1e-6 * np.abs(r1["step"][ok]).max()
    ok = np.isfinite(rt["length"])
    assert np.array_equal(np.isfinite(gt["length"]), ok)
    assert (np.abs(gt["length"][ok] - rt["length"][ok]) <= 1e-6 * np.maximum(rt["length"][ok], 1e-3)).all()
    # ragged batches: one ray, a wave less one, a wave, a wave and one, a block and one
    lat, lon, az, el = TA.synth.uniform_rays(257, T.C1_Y, T.C1_X, seed=5)
    p0, _ = geo.position(lat, lon, 300.0)
    dd = O.ecef_from_horizontal(lat, lon, az, el)
    ref = geo.trace(p0, dd, threads=2)
    for k in (1, 63, 64, 65, 257):
        t = st.trace(p0[:k].copy(), dd[:k])
        check_trace(t, ref["index"][:k], ref["length"][:k], ref["n_steps"][:k], f"{k} rays")
        s1 = st.step(p0[:k].copy(), dd[:k])
        o1 = geo.step(p0[:k].copy(), dd[:k])
        assert np.array_equal(s1["index"], o1["index"])
        assert np.abs(s1["step"] - o1["step"]).max() <= 1e-6 * o1["step"].max()
    st.destroy()
    m.destroy()


@pytest.mark.parametrize("where", ["south-west", "north-80", "equator-dateline"])
def test_long_rays_other_quadrants(where, math):
    """Grazing rays (thousands of steps: the fast trace's second phase, where
    coordinates come from the per-ray series) on maps in the other hemispheres, at
    high latitude and next to the date line, against the CPU restatement."""
    x, y = {"south-west": ((-71.0, -70.0), (-34.0, -33.0)),
            "north-80": ((15.0, 17.0), (79.5, 80.0)),
            "equator-dateline": ((178.9, 179.85), (-0.5, 0.5))}[where]
    nodes = T.c1_nodes()
    geo = O.OracleGeometry(grids=[O.default_grid(nodes, x, y, T.C1_Z)], layers=[[(O.MAP, 0, 0.0)]])
    m = TA.Map.create(nodes, x, y, T.C1_Z)
    st = B.c1_stepper(m)
    rng = np.random.default_rng(5)
    n = 1500
    lat = rng.uniform(y[0] + 0.2 * (y[1] - y[0]), y[1] - 0.2 * (y[1] - y[0]), n)
    lon = rng.uniform(x[0] + 0.2 * (x[1] - x[0]), x[1] - 0.2 * (x[1] - x[0]), n)
    az = rng.uniform(0.0, 360.0, n)
    el = rng.uniform(-3.0, 1.0, n)          # shallow: long paths close to the ground
    pos0, di = geo.position(lat, lon, 30.0)
    assert (di == 0).all()
    d = O.ecef_from_horizontal(lat, lon, az, el)
    ref = geo.trace(pos0, d, threads=4)
    t = st.trace(pos0.copy(), d)
    assert (ref["n_steps"] > 512).sum() > 50, "the recipe no longer reaches the second phase"
    # Zero tolerance, with ONE kind of ray set apart and named: a ray that never
    # reaches a boundary and stops at the cap (max_steps = 100 000; south-west has
    # one, ray 904: el = -0.795 deg, 28 951 m).  Its "path length" is no distance to
    # an intersection but the sum of 1e5 clearance-sized steps along the ground,
    # each fed by the sample before it: a 1e-9 m difference in one sample grows to
    # centimetres (the STRICT arithmetic, which differs from the reference by OCML's
    # last ulp in sin/cos only, ends 2.5e-2 m = 8.7e-7 off on it; FAST 4.5e-2 m =
    # 1.6e-6; round 2's kernels the same to the digit).  For such a ray the bar is:
    # same medium, same (capped) step count, 1e-5 on the sum.
    rel = np.abs(t["length"] - ref["length"]) / np.maximum(ref["length"], 1e-300)
    capped = ref["n_steps"] >= 100000
    assert capped.sum() <= 1 and np.array_equal(t["n_steps"][capped], ref["n_steps"][capped])
    assert np.array_equal(t["index"][capped], ref["index"][capped]) and (rel[capped] < 1e-5).all()
    grazing = ((t["index"][:, 0] != ref["index"][:, 0]) | (rel > REL)) & ~capped
    assert grazing.sum() == 0, f"{where}: {int(grazing.sum())} rays off the bar"
    ok = ~grazing
    assert (np.abs(t["n_steps"] - ref["n_steps"])[ok] <= 1).all()
    print(f"{where}: {int((ref['n_steps'] > 512).sum())} rays beyond 512 steps (max "
          f"{int(ref['n_steps'].max())}), {int(grazing.sum())} grazing, the others: worst relative "
          f"path-length difference {rel[ok].max():.2e}, beyond 1e-8: {int((rel[ok] > 1e-8).sum())}")
    st.destroy()
    m.destroy()


def test_philox_and_isotropic_bitwise():
    import philox_ref as P
    for seed, stream, first in ((0, 0, 0), (0x5EED2026, 7, 123456789012), (2 ** 64 - 1, 2 ** 40 + 3, 5)):
        w = TA.philox(1000, seed, stream, first)
        assert np.array_equal(w, P.blocks(1000, seed, stream, first))
    assert [hex(int(v)) for v in TA.philox(1, 0, 0, 0)[0]] == \
        ["0x6627e8d5", "0xe169c58d", "0xbc57ac4c", "0x9b00dbd8"]  # Random123 KAT
    d = TA.isotropic(4096, 0x5EED2026, 11, 100, device=False)
    ref = P.isotropic(4096, 0x5EED2026, 11, 100)
    assert np.abs(d - ref).max() < 1e-15  # sin, cos of 2 pi u: own polynomials vs numpy of the rounded 2 pi u
    assert np.abs(np.linalg.norm(d, axis=1) - 1).max() < 1e-15


def test_scattering_walk_against_oracle(math):
    """Config C5 in small: every ray takes K single steps, each in a fresh
    isotropic direction; the GPU carries its sample over between steps
    (TURTLE_AMD_STEP_RESUME), the oracle re-samples every start point."""
    geo = T.c1_oracle()
    m = B.c1_map()
    st = B.c1_stepper(m)
    n, K = 3000, 40
    lat, lon, az, el = TA.synth.uniform_rays(n, T.C1_Y, T.C1_X, seed=55)
    pos, _ = st.position(lat, lon, 30.0)
    ref_pos = pos.copy()
    state = st.step(pos, None)
    total, ref_total = np.zeros(n), np.zeros(n)
    flips = 0
    for k in range(K):
        d = TA.isotropic(n, 99, k, device=False)
        state = st.step(state["position"], d, resume=state)
        o = geo.step(ref_pos, d)
        ref_pos = o["position"]
        same = state["index"][:, 0] == o["index"][:, 0]
        flips += int((~same).sum())
        # a ray whose medium differs has diverged for good: re-synchronise it so
        # that later steps keep testing the arithmetic, and count it
        if not same.all():
            bad = np.flatnonzero(~same)
            state["position"][bad] = ref_pos[bad]
            fresh = st.step(ref_pos[bad].copy(), None)
            for key in ("altitude", "elevation", "index", "latitude", "longitude"):
                state[key][bad] = fresh[key]
        ok = same & (o["index"][:, 0] >= 0)
        assert np.abs(state["step"][ok] - o["step"][ok]).max() <= \
            max(1e-6 * o["step"][ok].max(), 1e-7)
        assert np.abs(state["position"][same] - ref_pos[same]).max() < 1e-6
        total += state["step"]
        ref_total += o["step"]
    # crossing the surface at random angles 120 000 times: a handful of rays may
    # be classified differently when they land within 1e-9 m of it
    assert flips == 0, flips
    st.destroy()
    m.destroy()


def test_scatter_n_is_the_step_loop(math, tmp_path):
    """turtle_stepper_scatter_n (a ray's whole walk in one kernel, directions drawn and
    sums kept there) against the loop over turtle_amd_isotropic_n +
    turtle_stepper_step_n with TURTLE_AMD_STEP_RESUME: bit for bit in strict
    arithmetic; in fast arithmetic the loop bisects a crossing on the ray's line and
    the walk by the closed form (1e-9 m apart: a ray that lands on the other side of a
    surface by that much diverges, and is counted).  On a map and through a stack with
    a hole (whose tiles come in while the first walk runs: that one goes generation
    by generation, in rounds); in one call and in two; numpy arrays and torch tensors."""
    import torch
    m = B.c1_map()
    stack = B.mosaic(tmp_path, [(45, 3), (45, 4), (46, 3)], 1201)
    for terrain, box, add in ((m, (T.C1_Y, T.C1_X), "add_map"),
                              (stack, ((45.0, 47.0), (3.0, 5.0)), "add_stack")):
        st = TA.Stepper()
        getattr(st, add)(terrain, 0.0)
        n, K = 5000, 24
        lat, lon, _, _ = TA.synth.uniform_rays(n, box[0], box[1], seed=8)
        pos, di = st.position(lat, lon, 20.0)
        pos = pos[di == 0]
        n = pos.shape[0]
        state = st.step(pos.copy(), None)
        total, moved = np.zeros(n), np.zeros(n, dtype=np.int32)
        for k in range(K):
            inside = state["index"][:, 0] >= 0
            d = TA.isotropic(n, 4242, k, first_ray=17, device=False)
            state = st.step(state["position"], d, resume=state)
            moved += inside
            total += np.where(inside, state["step"], 0.0)
        w = st.scatter(pos.copy(), 4242, K, first_ray=17)
        s = st.trace_stats()
        assert s["steps"] == int(w["steps"].sum())
        if math == "strict":
            assert np.array_equal(w["position"], state["position"])
            assert np.array_equal(w["index"], state["index"])
            assert np.array_equal(w["steps"], moved) and np.array_equal(w["length"], total)
            inside = state["index"][:, 0] >= 0
            assert np.array_equal(w["altitude"][inside], state["altitude"][inside])
        else:
            same = (w["index"][:, 0] == state["index"][:, 0]) & (w["steps"] == moved)
            assert (~same).sum() == 0, int((~same).sum())
            assert np.abs(w["position"][same] - state["position"][same]).max() < 1e-6
            assert np.abs(w["length"][same] - total[same]).max() < 1e-6
        w2 = st.scatter(pos.copy(), 4242, 10, first_ray=17)
        w2 = st.scatter(None, 4242, K - 10, first_ray=17, first_step=10, state=w2)
        wd = st.scatter(torch.as_tensor(pos, device="cuda"), 4242, K, first_ray=17)
        TA.synchronize()      # device arrays: the call returns once its launches are queued
        for got in (w2, {k: v.cpu().numpy() for k, v in wd.items()}):
            for key in ("position", "index", "steps", "length"):
                assert np.array_equal(got[key], w[key]), key
        st.destroy()
    m.destroy()
    stack.destroy()


def test_walk_n_is_the_step_loop_with_less_state(math, tmp_path):
    """turtle_stepper_walk_n (round 4): a walk's steps with ONE double of state a ray between the
    calls -- the tentative length of its next step -- where turtle_stepper_step_n with
    TURTLE_AMD_STEP_RESUME hands altitude and two elevations back and forth.  The same function of
    the same sample, evaluated when the sample is taken instead of when the next step begins:
    positions, step lengths and media equal bit for bit, step after step, in both arithmetics;
    over one map and through a stack with a hole whose rim rays leave by; numpy and device arrays."""
    import torch
    m = B.c1_map()
    stack = B.mosaic(tmp_path, [(45, 3), (45, 4), (46, 3)], 1201)
    for terrain, box, add, height in ((m, (T.C1_Y, T.C1_X), "add_map", 20.0),
                                      (stack, ((45.0, 47.0), (3.0, 5.0)), "add_stack", 3000.0)):
        st = TA.Stepper()
        getattr(st, add)(terrain, 0.0)
        n, K = 4000, 20
        lat, lon, _, _ = TA.synth.uniform_rays(n, box[0], box[1], seed=12)
        pos, di = st.position(lat, lon, height)
        pos = pos[di == 0]
        n = pos.shape[0]
        a = st.step(pos.copy(), None)
        b = st.walk(pos.copy())
        bd = st.walk(torch.as_tensor(pos, device="cuda").clone())
        assert np.array_equal(a["index"], b["index"]) and np.array_equal(a["step"], b["next"])
        left = 0
        for k in range(K):
            d = TA.isotropic(n, 31, k, first_ray=3, device=False)
            a = st.step(a["position"], d, resume=a)
            b = st.walk(None, d, state=b)
            bd = st.walk(None, torch.as_tensor(d, device="cuda"), state=bd)
            TA.synchronize()
            for got in (b, {k_: v.cpu().numpy() for k_, v in bd.items()}):
                assert np.array_equal(got["position"], a["position"]), k
                assert np.array_equal(got["index"], a["index"]), k
                assert np.array_equal(got["step"], a["step"]), k
            left = int((a["index"][:, 0] < 0).sum())
        if add == "add_stack":
            assert left > 20           # rays did leave, and then took no further step
        st.destroy()
    m.destroy()
    stack.destroy()


def test_gradient_bit_exact(golden, tmp_path):
    """turtle_map_gradient / turtle_stack_gradient [ref map.c:280-392,
    stack.c:364-388]: +,-,*,/ only, so bit-exact, slip at map.c:353 included."""
    g = golden("gradient")
    m = TA.Map.create(g["nodes"], T.C1_X, T.C1_Y, T.C1_Z)
    gx, gy, inside = m.gradient(g["x"], g["y"], fill=-7.0)
    assert np.array_equal(inside, g["inside"])
    assert np.array_equal(gx, g["gx"]) and np.array_equal(gy, g["gy"])
    m.destroy()
    stack = B.mosaic(tmp_path, [(45, 3), (45, 4), (46, 3)], 1201)
    glat, glon, sin = stack.gradient(g["lat"], g["lon"], fill=-7.0)
    assert np.array_equal(sin, g["sinside"])
    assert np.array_equal(glat, g["glat"]) and np.array_equal(glon, g["glon"])
    stack.destroy()


def test_projections(golden):
    """turtle_projection_project/unproject [ref projection.c:192-448]: OCML's
    log/tan/pow/exp/sinh/atanh against glibc's, a few ulp of 1e7 m."""
    g = golden("projection")
    for k, name in enumerate(g["names"]):
        p = TA.Projection(str(name))
        x, y = p.project(g[f"p{k}_lat"], g[f"p{k}_lon"])
        assert np.abs(x - g[f"p{k}_x"]).max() < 2e-8 and np.abs(y - g[f"p{k}_y"]).max() < 2e-8, name
        la, lo = p.unproject(g[f"p{k}_x"], g[f"p{k}_y"])
        assert np.abs(la - g[f"p{k}_ulat"]).max() < 1e-12, name
        assert np.abs(lo - g[f"p{k}_ulon"]).max() < 1e-12, name
        xs, ys = p.project_scalar(float(g[f"p{k}_lat"][0]), float(g[f"p{k}_lon"][0]))
        assert xs == x[0] and ys == y[0]  # the scalar drop-in is the n = 1 batch
        p.destroy()


@pytest.mark.parametrize("name", ["nogeoid", "geoid"])
def test_projected_map_under_the_stepper(golden, name, math):
    """A UTM map + a flat sea under one layer [ref stepper.c:65-83, :243-248]."""
    g = golden("projection")
    m = TA.Map.create(g["nodes"], (495000.0, 497000.0), (5066000.0, 5068000.0), (0.0, 1000.0),
                      projection="UTM 31N")
    geoid = B.geoid_map(g["geoid_nodes"]) if name == "geoid" else None
    st = TA.Stepper()
    if geoid is not None:
        st.geoid_set(geoid)
    st.add_flat(-5.0)
    st.add_map(m, 0.0)
    pos, di = st.position(g[name + "_lat"], g[name + "_lon"], 150.0)
    assert np.array_equal(di, g[name + "_di"]) and np.abs(pos - g[name + "_pos"]).max() < 5e-8
    o = st.step(g[name + "_pos"][::4].copy(), None)
    rows = g[name + "_rows"]
    assert np.array_equal(o["index"], rows[:, 6:8].astype(np.int32))
    assert np.abs(o["altitude"] - rows[:, 2]).max() < 5e-9
    big = np.abs(rows[:, 3:5]) > 1e300
    assert np.abs(o["elevation"][~big] - rows[:, 3:5][~big]).max() < 1e-7
    assert np.abs(o["step"] - rows[:, 5]).max() < 1e-7
    t = st.trace(g[name + "_pos"].copy(), g[name + "_dir"])
    check_trace(t, g[name + "_t_index"], g[name + "_t_length"], g[name + "_t_n_steps"],
                f"UTM map ({name})")
    st.destroy()
    m.destroy()
    if geoid is not None:
        geoid.destroy()


def test_geotiff_map_elevation(golden):
    """A GeoTIFF written by the reference, read natively, looked up on the GPU:
    bit-exact against what the reference computed from the same file."""
    import os
    g = golden("geotiff")
    m = TA.Map.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                                 "geotiff_utm.tif"))
    z, inside = m.elevation(g["qx"], g["qy"])
    assert np.array_equal(inside, g["qin"])
    assert np.array_equal(z[inside == 1], g["qz"][inside == 1])
    m.destroy()


def test_png_map_elevation_and_stepper(golden):
    """The reference's own map file format, read natively: bit-exact lookups,
    and the projected map works under a stepper (the set-up of
    examples/example-stepper.c: flat + projected map)."""
    import os
    g = golden("png")
    m = TA.Map.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                                 "map_utm.png"))
    z, inside = m.elevation(g["qx"], g["qy"])
    assert np.array_equal(inside, g["qin"])
    assert np.array_equal(z[inside == 1], g["qz"][inside == 1])
    st = TA.Stepper()
    st.add_flat(0.0)
    st.add_map(m, 0.0)
    p = TA.Projection("UTM 31N")
    lat, lon = p.unproject(np.array([496000.0]), np.array([5067000.0]))
    pos, di = st.position(lat, lon, 10.0)
    o = st.step(pos, None)
    assert di[0] == 0 and o["index"][0, 0] == 1
    zc, _ = m.elevation(np.array([496000.0]), np.array([5067000.0]))
    # the UTM series pair is only inverse to ~1 mm [ref projection.c:377-448],
    # so the stepper looks the map up a millimetre away from (496000, 5067000)
    assert abs(o["elevation"][0, 0] - zc[0]) < 1e-2
    assert abs(o["altitude"][0] - o["elevation"][0, 0] - 10.0) < 1e-8
    p.destroy()
    st.destroy()
    m.destroy()


def test_reference_hgt_test_as_written(tmp_path):
    """The reference's test_io_hgt [ref tests/test-turtle.c:1049-1089] re-expressed: a 3601^2 tile of
    -1 / +1 written as the reference's test writes it (file order, big-endian), every node with
    k % 100 == 0 or k % 101 == 0 read back through turtle_map_node, then turtle_map_fill(0, 0, 10)
    and turtle_map_elevation(3, 45) == 10 -- through the kernel (the HBM copy of a map that was
    filled is made again) and on the host; and a batch of points against the bilinear of the
    checkerboard, bit for bit."""
    n = 3601
    k = np.arange(n * n, dtype=np.int64).reshape(n, n)
    z_file = np.where(k % 2 == 0, -1, 1).astype(">i2")
    path = os.path.join(str(tmp_path), "N45E003.hgt")
    z_file.tofile(path)
    m = TA.Map.load(path)
    pick = np.flatnonzero(((k % 100) == 0) | ((k % 101) == 0))[::37]      # a tenth of a percent of the reference's nodes
    for kk in pick:
        i, j = divmod(int(kk), n)
        _, _, z = m.node(j, i)
        assert z == (-1.0 if kk % 2 == 0 else 1.0), (i, j, z)
    # bilinear over the checkerboard, on the device: memory rows run south -> north
    z_mem = z_file[::-1, :].astype(np.float64)
    rng = np.random.default_rng(11)
    x, y = rng.uniform(3.0, 4.0, 20000), rng.uniform(45.0, 46.0, 20000)
    got, inside = m.elevation(x, y)
    hx, hy = (x - 3.0) / (1.0 / (n - 1)), (y - 45.0) / (1.0 / (n - 1))
    ix, iy = np.minimum(hx.astype(int), n - 2), np.minimum(hy.astype(int), n - 2)
    fx, fy = hx - ix, hy - iy
    want = (z_mem[iy, ix] * (1 - fx) * (1 - fy) + z_mem[iy + 1, ix] * (1 - fx) * fy +
            z_mem[iy, ix + 1] * fx * (1 - fy) + z_mem[iy + 1, ix + 1] * fx * fy)     # [ref map.c:272-273]
    assert inside.all() and np.array_equal(got, want)
    m.fill(0, 0, 10.0)
    z, inside = m.elevation_scalar(3.0, 45.0)
    assert inside and z == 10.0
    TA.set_scalar("host")
    try:
        z, inside = m.elevation_scalar(3.0, 45.0)
    finally:
        TA.set_scalar("device")
    assert inside and z == 10.0
    got2, _ = m.elevation(x, y)
    far = (ix > 0) | (iy > 0)
    assert np.array_equal(got2[far], want[far])         # only the cell of node (0, 0) changed
    m.destroy()


def test_plain_c_caller(tmp_path):
    """examples/trace_rays.c: a C99 program against include/turtle.h, built
    with gcc only and linked to libturtle_amd.so -- the scalar drop-in loop and
    one trace_n call agree (the program checks; we check its exit code)."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(tmp_path, "trace_rays")
    lib = os.path.join(root, "turtle_amd")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "examples", "trace_rays.c"), "-L" + lib,
                           "-lturtle_amd", "-lm", "-Wl,-rpath," + lib, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout[-600:], out.stderr[-300:])
    assert out.returncode == 0 and "0 disagreements" in out.stdout


def test_unmodified_reference_loop_and_the_environment_switch(tmp_path):
    """examples/reference_loop.c uses nothing but the reference's own header and keeps its
    per-ray loop of scalar calls.  Relinked, source unchanged: a launch a call by default; with
    TURTLE_AMD_SCALAR=host in the environment the same binary is answered on the host (the
    same media and step counts, path lengths within 1e-9) at a cost of the reference's order."""
    import os
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(tmp_path, "reference_loop")
    lib = os.path.join(root, "turtle_amd")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "examples", "reference_loop.c"), "-L" + lib,
                           "-lturtle_amd", "-lm", "-Wl,-rpath," + lib, "-o", exe])
    rows, cost = {}, {}
    for where in ("device", "host"):
        env = {k: v for k, v in os.environ.items() if k != "TURTLE_AMD_SCALAR"}
        if where == "host":
            env["TURTLE_AMD_SCALAR"] = "host"
        out = subprocess.run([exe, "12"], capture_output=True, text=True, timeout=300, env=env)
        assert out.returncode == 0, out.stderr[-500:]
        rows[where] = re.findall(r"ray (\d+): medium (-?\d+) -> (-?\d+) after (\d+) steps, (\S+) m", out.stdout)
        cost[where] = float(re.search(r"(\d+) ns a call", out.stdout).group(1))
    assert len(rows["host"]) == 12 and len(rows["device"]) == 12
    for a, b in zip(rows["device"], rows["host"]):
        assert a[:4] == b[:4], (a, b)
        assert abs(float(a[4]) - float(b[4])) <= 1e-9 * float(b[4]), (a, b)
    print(f"scalar calls: {cost['device']:.0f} ns on the device, {cost['host']:.0f} ns on the host")
    assert cost["host"] < 5000 < cost["device"]


def test_c_host_with_threads_and_rccl(tmp_path):
    """examples/multi_gpu_tally.c: a C host, one thread per GPU over a shared map,
    the tally reduced with ncclAllReduce(ncclUint64) over RCCL; on this one-GPU box
    it runs with one rank (communicator of one) and checks its own sums."""
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(tmp_path, "multi_gpu_tally")
    lib = os.path.join(root, "turtle_amd")
    subprocess.check_call(["gcc", "-std=gnu99", "-Wall", "-D__HIP_PLATFORM_AMD__",
                           "-I" + os.path.join(root, "include"), "-I/opt/rocm/include",
                           os.path.join(root, "examples", "multi_gpu_tally.c"), "-L" + lib,
                           "-lturtle_amd", "-L/opt/rocm/lib", "-lrccl", "-lamdhip64", "-lpthread", "-lm",
                           "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    out = subprocess.run([exe, "1", "100000"], capture_output=True, text=True, timeout=300)
    print(out.stdout[-400:], out.stderr[-400:])
    assert out.returncode == 0 and "reduced tally == one-GPU tally" in out.stdout


def test_two_ranks_share_the_gpu_through_bench(tmp_path):
    """The N > 1 path of bench.py itself on this one-GPU box: two ranks over gloo
    (RCCL needs a GPU per rank) trace their blocks and all-reduce the tally; one
    rank tracing both blocks (--blocks 2) gets the same tally, to the bit."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    common = ["--rays", "150000", "--steps", "2", "--warmup", "1", "--no-cpu", "--workload", "c2",
              "--also", "none"]
    env = dict(os.environ, TURTLE_BENCH_BACKEND="gloo", MASTER_ADDR="127.0.0.1")
    two = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
                          "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29517",
                          os.path.join(root, "bench.py"), "--gpus", "2"] + common,
                         capture_output=True, text=True, timeout=600, env=env, cwd=root)
    one = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--blocks", "2"]
                         + common, capture_output=True, text=True, timeout=600, cwd=root)
    lines = []
    for out in (two, one):
        rows = [l for l in out.stdout.splitlines() if l.startswith("{")]
        # the full record of the workload ("leg"), then the line the driver parses: the LAST one
        assert out.returncode == 0 and len(rows) == 2, (out.stdout[-500:], out.stderr[-1500:])
        assert json.loads(rows[0])["leg"] == "c2" and len(rows[-1]) < 6000
        lines.append(json.loads(rows[-1]))
        assert lines[-1]["kernel"]["ms"] <= lines[-1]["ms_per_step"]
        assert lines[-1]["in_flight"]["batches"] == 3 and lines[-1]["config"]["in_flight"] == 1
    assert lines[0]["backend"] == "gloo" and lines[0]["comm_world_size"] == 2
    assert lines[0]["n_gpus"] == 2 and lines[1]["n_gpus"] == 1
    assert lines[0]["tally"] == lines[1]["tally"]
    assert sum(lines[0]["tally"]["hits"]) == 300000
    assert lines[0]["kernel"]["steps_per_launch"] * 2 > lines[1]["kernel"]["steps_per_launch"] > 0
    # and `python bench.py --gpus 2` by itself, as the driver calls it: it starts its two
    # ranks as a child job and relays rank 0's line and the exit code
    own = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2"] + common,
                         capture_output=True, text=True, timeout=600, cwd=root,
                         env={k: v for k, v in env.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")})
    rows = [l for l in own.stdout.splitlines() if l.startswith("{")]
    assert own.returncode == 0 and len(rows) == 2, (own.stdout[-500:], own.stderr[-1500:])
    assert json.loads(rows[-1])["n_gpus"] == 2 and json.loads(rows[-1])["tally"] == lines[0]["tally"]
    bad = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--workload", "nope"],
                         capture_output=True, text=True, timeout=120, cwd=root)
    assert bad.returncode != 0


def test_bench_dumps_what_its_last_timed_step_computed(tmp_path):
    """bench.py --dump-outputs: --steps passes timed, and the arrays of the last one written as
    float64 .npy -- the tally in the result line is theirs, and they agree with the CPU oracle"""
    import hashlib
    import json
    import subprocess
    import sys
    from turtle_amd import sharding
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = tmp_path / "outputs"
    n = 60000
    run = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--workload", "c2",
                          "--rays", str(n), "--steps", "3", "--warmup", "1", "--no-cpu", "--also", "none",
                          "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, cwd=root)
    rows = [l for l in run.stdout.splitlines() if l.startswith("{")]
    assert run.returncode == 0 and len(rows) == 2, (run.stdout[-500:], run.stderr[-1500:])
    line, record = json.loads(rows[-1]), json.loads(rows[0])
    assert line["steps"] == 3 and record["steps"] == 3 and line["ms_per_step"] > 0
    assert record["outputs"]["rays"] == n and "ray" not in record["outputs"]["files"]
    got = {name: np.load(out / (name + ".npy")) for name in ("position", "index", "length", "n_steps", "tally")}
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["position"].shape == (n, 3) and got["index"].shape == (n, 2) and got["length"].shape == (n,)
    tally = got["tally"].astype(np.int64)
    assert hashlib.sha256(tally.tobytes()).hexdigest()[:16] == line["tally"]["sha256"]
    hits, _, steps, _ = sharding.tally_layout(2, 1024)
    assert tally[steps] == got["n_steps"].sum() and tally[hits].sum() == n
    # bench.py's C2 rays set up as it does, their first ones traced by the oracle
    m = 2000
    lat, lon, az, el = (v[:m] for v in sharding.rank_rays(n, 0, (45.0, 46.0), (3.0, 4.0)))
    tile = B.hgt_tile(tmp_path)
    st = B.c1_stepper(tile)
    pos, _ = st.position(lat, lon, 500.0)
    d = TA.ecef_from_horizontal(lat, lon, az, el)
    st.destroy()
    tile.destroy()
    _, geo = T.hgt_oracle(45, 3)
    ref = geo.trace(pos, d, local_range=0.0, threads=8)
    assert np.array_equal(got["index"][:m], ref["index"])
    assert (np.abs(got["length"][:m] - ref["length"]) <= 1e-6 * np.abs(ref["length"])).all()


@pytest.mark.parametrize("fmt", ["hgt", "tif"])
def test_scatter_over_a_stack_against_the_oracle(math, tmp_path, fmt):
    """Config C5 in small, on its real kind of terrain: a walk of 64 generations over a
    3 x 3 mosaic with a hole (seams, the rim, rays that leave), every step against the
    CPU restatement's single steps, directions from the library's Philox.  The tiles as
    SRTM ships them (.hgt) and as ASTER-GDEM2 does, the terrain BASELINE names for C5:
    GeoTIFF, int16 (the reference reads those files as it reads the .hgt ones:
    tests/golden/check_geotiff_tiles_with_reference.py)."""
    tiles = [(la, lo) for la in (45, 46, 47) for lo in (3, 4, 5) if (la, lo) != (46, 4)]
    stack = B.mosaic(tmp_path, tiles, 1201, fmt)
    stack.load()
    geo = T.mosaic_oracle(tiles, 1201, 45, 3, 3, 3)
    rng = np.random.default_rng(9)
    qlat, qlon = rng.uniform(44.9, 48.1, 4096), rng.uniform(2.9, 6.1, 4096)
    z, inside = stack.elevation(qlat, qlon)
    zo, io = geo.stack_elevation(0, qlat, qlon)
    assert np.array_equal(inside, io) and np.array_equal(z, zo)   # tile selection and bilinear: bit-exact
    st = TA.Stepper()
    st.add_stack(stack, 0.0)
    n, K = 6000, 64
    lat, lon, _, _ = TA.synth.uniform_rays(n, (45.0, 48.0), (3.0, 6.0), seed=21, margin=0.02)
    height = np.where(np.arange(n) % 4 == 0, 30000.0, 60.0)   # high ones take 10 km steps: they leave
    pos, di = st.position(lat, lon, height)
    pos = pos[di == 0]
    n = pos.shape[0]
    w = st.scatter(pos.copy(), 777, K, first_ray=5)
    ref_pos, total = pos.copy(), np.zeros(n)
    o = geo.step(ref_pos)
    alive = o["index"][:, 0] >= 0
    steps = np.zeros(n, dtype=np.int32)
    for k in range(K):
        d = TA.isotropic(n, 777, k, first_ray=5, device=False)
        o = geo.step(ref_pos, d)
        ref_pos = np.where(alive[:, None], o["position"], ref_pos)
        total += np.where(alive, o["step"], 0.0)
        steps += alive
        alive &= o["index"][:, 0] >= 0
    ref_medium = np.where(alive, o["index"][:, 0], -1)
    same = (w["index"][:, 0] == ref_medium) & (w["steps"] == steps)
    # a ray that lands on the other side of a surface by 1e-9 m has diverged for good
    assert (~same).sum() == 0, int((~same).sum())
    assert np.abs(w["position"][same] - ref_pos[same]).max() < 1e-5
    rel = np.abs(w["length"][same] - total[same]) / np.maximum(total[same], 1e-300)
    assert rel.max() <= REL, rel.max()
    assert (steps < K).sum() > 20          # rays did leave: through the hole and the rim
    st.destroy()
    stack.destroy()
