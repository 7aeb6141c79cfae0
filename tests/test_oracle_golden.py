"""Pin the CPU restatement (oracle/) against the reference's own outputs.

tests/golden/*.npz were produced by tests/golden/generate.py driving the real
reference library.  The restatement follows the reference expression by
expression, so on the same libm it must agree BIT FOR BIT at local_range = 0
and 1; the asserts below are exact unless a comment says otherwise.
"""
import numpy as np

from oracle import ffi as O
import terrains as T
from turtle_amd import synth


def eq(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def test_g1_ecef(golden):
    g = golden("ecef")
    assert eq(O.ecef_from_geodetic(g["lat"], g["lon"], g["alt"]), g["ecef"])
    la, lo, al = O.ecef_to_geodetic(g["ecef_all"])
    assert eq(la, g["to_lat"]) and eq(lo, g["to_lon"]) and eq(al, g["to_alt"])
    assert eq(O.ecef_from_horizontal(g["lat"], g["lon"], g["az"], g["el"]), g["direction"])
    az, el = O.ecef_to_horizontal(g["lat"], g["lon"], g["dir_scaled"])
    assert eq(az, g["to_az"]) and eq(el, g["to_el"])


def test_g1_reference_test_ecef_assertions():
    """tests/test-turtle.c:582-625 re-expressed."""
    p = O.ecef_from_geodetic([45.5], [3.5], [1000.0])
    la, lo, al = O.ecef_to_geodetic(p)
    assert abs(la[0] - 45.5) < 1e-8 and abs(lo[0] - 3.5) < 1e-8 and abs(al[0] - 1000) < 1e-8
    d = O.ecef_from_horizontal([45.5], [3.5], [60.0], [30.0])
    az, el = O.ecef_to_horizontal([45.5], [3.5], d)
    assert abs(az[0] - 60) < 1e-8 and abs(el[0] - 30) < 1e-8
    for lat, lon in ((90.0, 0.0), (-90.0, 0.0), (0.0, 90.0)):
        p = O.ecef_from_geodetic([lat], [lon], [1000.0])
        la, lo, al = O.ecef_to_geodetic(p)
        if abs(lat) == 90:
            # cos(pi/2) is 6e-17, not 0: the reference test passes because
            # its check is ck_assert_double_eq on the *rounded* result
            assert abs(la[0] - lat) < 1e-9 and abs(al[0] - 1000) < 1e-8
        else:
            assert la[0] == lat and lo[0] == lon and abs(al[0] - 1000) < 1e-8


def test_g2_bilinear(golden):
    g = golden("bilinear")
    assert T.sha(T.c1_nodes()) == str(g["nodes_sha"])
    geo = T.c1_oracle()
    z, inside = geo.grid_elevation(0, g["x"], g["y"])
    assert eq(inside, g["inside"])
    ok = inside == 1
    assert eq(z[ok], g["z"][ok])
    for ix, iy, xyz in zip(g["node_ix"], g["node_iy"], g["node_xyz"]):
        v = O.lib().orc_grid_node(O.C.byref(geo.grids[0]), int(ix), int(iy))
        assert v == xyz[2]


def _check_trace(t, g, prefix):
    assert eq(t["index"], g[prefix + "_index"])
    assert eq(t["n_steps"], g[prefix + "_n_steps"])
    assert eq(t["length"], g[prefix + "_length"])
    assert eq(t["position"], g[prefix + "_position"])


def test_g3_c1_traces(golden):
    g = golden("c1_traces")
    geo = T.c1_oracle()
    pos, di = geo.position(g["lat"], g["lon"], 500.0)
    assert eq(pos, g["position"]) and (di == 0).all()
    assert eq(O.ecef_from_horizontal(g["lat"], g["lon"], g["az"], g["el"]), g["direction"])
    for prefix, rng in (("r0", 0.0), ("r1", 1.0)):
        t = geo.trace(g["position"], g["direction"], local_range=rng)
        _check_trace(t, g, prefix)
    assert 300 < g["r0_n_steps"].mean() < 500  # ~393 steps/ray


def test_g3_threads_do_not_change_results(golden):
    g = golden("c1_traces")
    geo = T.c1_oracle()
    t = geo.trace(g["position"], g["direction"], local_range=0.0, threads=4)
    _check_trace(t, g, "r0")


def test_g7_per_step_records(golden):
    g = golden("steps")
    geo = T.c1_oracle()
    rec = g["record"]
    # replay each ray one turtle_stepper_step at a time (orc_step_n: fresh
    # history per call, exact transform)
    for r in range(g["position"].shape[0]):
        rows = rec[rec[:, 0] == r]
        pos = g["position"][r].copy()
        for row in rows:
            o = geo.step(pos[None, :], g["direction"][r][None, :])
            assert eq(o["position"][0], row[2:5])
            assert o["step"][0] == row[5]
            assert eq(o["index"][0], row[6:8].astype(np.int32))
            pos = o["position"][0]


def test_g4_hgt_tile(golden):
    g = golden("hgt_traces")
    nodes, geo = T.hgt_oracle()
    assert T.sha(nodes) == str(g["nodes_sha"])
    for ix, iy, z in zip(g["node_ix"], g["node_iy"], g["node_z"]):
        assert O.lib().orc_grid_node(O.C.byref(geo.grids[0]), int(ix), int(iy)) == z
    z, inside = geo.grid_elevation(0, g["qx"], g["qy"])
    assert eq(inside, g["qin"])
    assert eq(z[inside == 1], g["qz"][inside == 1])
    pos, di = geo.position(g["lat"], g["lon"], 500.0)
    assert eq(pos, g["position"])
    for prefix, rng in (("r0", 0.0), ("r1", 1.0)):
        t = geo.trace(g["position"], g["direction"], local_range=rng, threads=4)
        _check_trace(t, g, prefix)


def test_g11_c3_seam_full_size_tiles(golden):
    """C3's shape at full tile size: rays across the seams of a 2x2 mosaic of 3601^2 tiles, the
    restatement against the reference's own trace, bit for bit."""
    g = golden("c3_seam")
    tiles = [tuple(t) for t in g["tiles"]]
    assert T.sha(synth.srtm_like_nodes(45, 3)) == str(g["nodes_sha"])
    geo = T.mosaic_oracle(tiles, synth.HGT_N, 45, 3, 2, 2)
    pos, di = geo.position(g["lat"], g["lon"], 300.0)
    assert eq(pos, g["position"]) and (di == 0).all()
    t = geo.trace(g["position"], g["direction"], threads=4)
    _check_trace(t, g, "t")
    # the rays do what the fixture is for: they end in another tile than they started in
    lat1, lon1, _ = O.ecef_to_geodetic(t["position"])
    moved = (np.floor(lat1) != np.floor(g["lat"])) | (np.floor(lon1) != np.floor(g["lon"]))
    assert moved.sum() > 300 and (t["index"][:, 0] == -1).any()


def test_g5_stack(golden):
    g = golden("stack")
    n = int(g["n"])
    geo = T.mosaic_oracle([tuple(t) for t in g["tiles"]], n, 45, 3, 2, 2)
    z, inside = geo.stack_elevation(0, g["lat"], g["lon"])
    assert eq(inside, g["inside"])
    assert eq(z, g["z"])
    one = T.mosaic_oracle([(45, 3)], n, 45, 3, 1, 1)
    z1, in1 = one.stack_elevation(0, g["lat1"], g["lon1"])
    assert eq(in1, g["in1"]) and eq(z1, g["z1"])
    # SURVEY 8c probe facts: (45.5,3.5) in, (45,3) in, (46,4) OUT, (46.0000001,3.5) out
    assert list(in1[:4]) == [1, 1, 0, 0]
    pos, di = geo.position(g["ray_lat"], g["ray_lon"], 300.0)
    assert eq(pos, g["position"])
    t = geo.trace(g["position"], g["direction"])
    _check_trace(t, g, "t")
    assert (t["index"][:, 0] == -1).any() and (t["index"][:, 0] == 0).any()


def test_g6_layers(golden):
    g = golden("layers")
    for name, geoid_nodes in (("nogeoid", None), ("geoid", g["geoid_nodes"])):
        geo = T.c1_oracle(layers=T.two_layer_spec(), geoid_nodes=geoid_nodes)
        P, D, Oq = g[name + "_P"], g[name + "_D"], g[name + "_O"]
        for slope in (0.4, 2.0):
            for has_dir in (0, 1):
                sel = (Oq[:, 2] == slope) & (Oq[:, 1] == has_dir)
                o = geo.step(P[sel], D[sel] if has_dir else None, slope=slope)
                ref = Oq[sel]
                assert (ref[:, 0] == 0).all()
                assert eq(o["position"], ref[:, 3:6])
                assert eq(o["latitude"], ref[:, 6]) and eq(o["longitude"], ref[:, 7])
                assert eq(o["altitude"], ref[:, 8])
                assert eq(o["elevation"], ref[:, 9:11])
                assert eq(o["step"], ref[:, 11])
                assert eq(o["index"], ref[:, 12:14].astype(np.int32))
        # stepper_position on both layers, incl. the data index it reports
        t = geo.trace(g[name + "_tpos"], g[name + "_tdir"])
        _check_trace(t, g, name + "_t")
        t2 = geo.trace(t["position"], g[name + "_tdir"])
        _check_trace(t2, g, name + "_t2")


def test_g8_gradient(golden):
    """turtle_map_gradient incl. the slip at map.c:353 (13 rows of the fixture)."""
    g = golden("gradient")
    geo = O.OracleGeometry(grids=[O.default_grid(g["nodes"], T.C1_X, T.C1_Y, T.C1_Z)],
                           layers=[[(O.MAP, 0, 0.0)]])
    gx, gy, inside = geo.grid_gradient(0, g["x"], g["y"])
    assert eq(inside, g["inside"]) and eq(gx, g["gx"]) and eq(gy, g["gy"])
    assert ((g["gy"] == -7.0) & (g["inside"] == 1)).sum() > 0  # the slip is exercised


UTM_X, UTM_Y, UTM_Z = (495000.0, 497000.0), (5066000.0, 5068000.0), (0.0, 1000.0)


def utm_oracle(g, with_geoid):
    grids = [O.default_grid(g["nodes"], UTM_X, UTM_Y, UTM_Z, projection="UTM 31N")]
    geoid = -1
    if with_geoid:
        grids.append(O.default_grid(g["geoid_nodes"], (0.0, 360.0), (-90.0, 90.0), (-40.0, 40.0)))
        geoid = 1
    return O.OracleGeometry(grids=grids, layers=[[(O.FLAT, 0, -5.0), (O.MAP, 0, 0.0)]],
                            geoid=geoid)


def test_g9_projections(golden):
    """projection.c forward/inverse for the six Lambert variants and UTM."""
    g = golden("projection")
    for k, name in enumerate(g["names"]):
        x, y = O.project(str(name), g[f"p{k}_lat"], g[f"p{k}_lon"])
        assert eq(x, g[f"p{k}_x"]) and eq(y, g[f"p{k}_y"]), name
        la, lo = O.unproject(str(name), g[f"p{k}_x"], g[f"p{k}_y"])
        assert eq(la, g[f"p{k}_ulat"]) and eq(lo, g[f"p{k}_ulon"]), name
        assert np.abs(la - g[f"p{k}_lat"]).max() < 1e-7  # it is a projection pair


def test_g9_projected_map_in_the_stepper(golden):
    """stepper.c:65-83, :243-248, :304-311: a UTM map under the stepper."""
    g = golden("projection")
    for name in ("nogeoid", "geoid"):
        geo = utm_oracle(g, name == "geoid")
        pos, di = geo.position(g[name + "_lat"], g[name + "_lon"], 150.0)
        assert eq(pos, g[name + "_pos"]) and eq(di, g[name + "_di"])
        o = geo.step(g[name + "_pos"][::4])
        rows = g[name + "_rows"]
        assert eq(o["latitude"], rows[:, 0]) and eq(o["longitude"], rows[:, 1])
        assert eq(o["altitude"], rows[:, 2]) and eq(o["elevation"], rows[:, 3:5])
        assert eq(o["step"], rows[:, 5]) and eq(o["index"], rows[:, 6:8].astype(np.int32))
        t = geo.trace(g[name + "_pos"], g[name + "_dir"])
        _check_trace(t, g, name + "_t")


def test_g12_rough_and_void_ground(golden):
    """Traces, single steps and deep ECEF -> geodetic over rough and void ground (tests/rough_cases.py):
    the restatement against the reference, bit for bit -- the values stored in rough.npz, and the
    origins, directions and positions against the sha256 of the reference's"""
    import rough_cases as RC
    g = golden("rough")
    for case in RC.CASES:
        assert RC.sha(RC.nodes(case)) == str(g[f"{case}_nodes_sha"])
        geo = RC.oracle_geometry(case)
        for recipe in RC.recipes(case):
            k = f"{case}_{recipe}_"
            pos, d = RC.oracle_rays(case, recipe)
            assert RC.sha(pos) == str(g[k + "origin_sha"]) and RC.sha(d) == str(g[k + "direction_sha"])
            t = geo.trace(pos, d, max_steps=1000000, threads=4)
            assert eq(t["index"], g[k + "index"].astype(np.int32)), k
            assert eq(t["n_steps"], g[k + "n_steps"]) and eq(t["length"], g[k + "length"]), k
            assert RC.sha(t["position"]) == str(g[k + "position_sha"]), k
        pos, d = RC.oracle_rays(case, "ground")
        ds, index, position = RC.oracle_step_records(geo, pos[:RC.STEP_RAYS], d[:RC.STEP_RAYS])
        assert RC.sha(ds) == str(g[f"{case}_steps_ds_sha"])
        assert eq(index, g[f"{case}_steps_index"].astype(np.int32))
        assert RC.sha(position) == str(g[f"{case}_steps_position_sha"])
    # the void tile: rays that start in a void (32 km below the ellipsoid) and rays that end in one
    lat, lon, _ = O.ecef_to_geodetic(RC.oracle_rays("void", "c2")[0])
    z, _ = RC.oracle_geometry("void").grid_elevation(0, lon, lat)
    assert (z < -30000).sum() >= 10
    assert all((g[f"void_edge{k}_index"][:, 0] == 0).sum() > 30 for k in range(len(RC.VOID_BLOCKS)))
    e, geodetic = RC.deep_transforms(O.ecef_from_geodetic, O.ecef_to_geodetic)
    assert RC.sha(e) == str(g["deep_ecef_sha"]) and RC.sha(geodetic) == str(g["deep_geodetic_sha"])
    assert (geodetic[2] < -25e3 + 1).all() and (geodetic[2] > -40e3 - 1).all()


def test_g14_composite_geometries(golden):
    """Traces at both local ranges, lines of sight through every medium, and position and single
    steps hugging every rim, over composite geometries (tests/composite_cases.py: a stack beside
    maps and flats, overlapping maps, layers without data, a geoid): the restatement against the
    reference (composite.npz), bit for bit, NaN for NaN"""
    import composite_cases as CC
    import traverse_cases as TC
    g = golden("composite")
    lat, lon = CC.utm_footprint()       # the UTM map lies inside tile (0N, 11E)
    assert (lat > 0.0).all() and (lat < 1.0).all() and (lon > 11.0).all() and (lon < 12.0).all()
    for case in CC.CASES:
        assert CC.nodes_sha(case) == str(g[f"{case}_nodes_sha"])
        geo = CC.oracle_geometry(case)
        pos, d, _ = CC.graze(case, geo, CC.GOLDEN_RAYS)
        assert CC.sha(pos) == str(g[f"{case}_graze_origin_sha"])
        assert CC.sha(d) == str(g[f"{case}_graze_direction_sha"])
        for tag, local_range in (("r1", 1.0), ("r0", 0.0)):
            k = f"{case}_{tag}_"
            t = geo.trace(pos, d, max_steps=CC.GRAZE_MAX_STEPS, local_range=local_range, threads=4)
            assert eq(t["index"], g[k + "index"].astype(np.int32)), k
            assert eq(t["n_steps"], g[k + "n_steps"]) and eq(t["length"], g[k + "length"]), k
            assert eq(t["position"], g[k + "position"]), k
        pos, d = CC.sight(case, CC.GOLDEN_RAYS)
        k = f"{case}_sight_"
        assert CC.sha(pos) == str(g[k + "origin_sha"]) and CC.sha(d) == str(g[k + "direction_sha"])
        t = TC.check(geo, pos, d, CC.CEILING, max_steps=CC.SIGHT_MAX_STEPS, threads=4)
        assert eq(t["index"], g[k + "index"].astype(np.int32)), k
        assert eq(t["length"], g[k + "length"]) and eq(t["n_steps"], g[k + "n_steps"]), k
        assert eq(t["n_crossings"], g[k + "n_crossings"]), k
        k = f"{case}_rim_"
        lat, lon, _ = CC.rim_points(case)
        assert CC.sha(np.stack([lat, lon])) == str(g[k + "points_sha"])
        both = set()
        for layer in range(len(CC.RECIPES[case][1]) - 1):
            p, di = geo.position(lat, lon, 100.0, layer=layer)
            assert eq(di, g[k + f"data{layer}"].astype(np.int32)), (k, layer)
            assert eq(p[di >= 0], g[k + f"position{layer}"][di >= 0]), (k, layer)
            both |= set(np.unique(di))
        assert len(both) >= 3           # the points do hug rims: more than one data answers
        start = O.ecef_from_geodetic(lat, lon, np.full(lat.size, 2500.0))
        assert CC.sha(start) == str(g[k + "start_sha"])
        o, rows = geo.step(start), g[k + "step"]
        assert eq(o["latitude"], rows[:, 0]) and eq(o["longitude"], rows[:, 1]) and eq(o["altitude"], rows[:, 2])
        assert eq(o["elevation"], rows[:, 3:5]) and eq(o["index"], rows[:, 5:7].astype(np.int32)), k


def test_g15_slope_and_resolution(golden):
    """Traces at slope and resolution other than the defaults (tests/params_cases.py: the reference
    example's slope 1, slope 2 and 0.1, resolutions of 1e-3, 0.25 and 1 m) over the smooth and the
    rough tile: the restatement against the reference (params.npz), bit for bit"""
    import params_cases as PC
    import traverse_cases as TC
    g = golden("params")
    assert T.sha(TC.nodes("rough")) == str(g["rough_nodes_sha"])
    for case in PC.CASES:
        geo = TC.oracle_geometry(case)
        for recipe in PC.RECIPES:
            pos, d = g[f"{case}_{recipe}_position"], g[f"{case}_{recipe}_direction"]
            if recipe != "c2":          # the stored rays are the recipe's
                lat, lon, height, az, el = PC.draws(case, recipe)
                assert eq(geo.position(lat, lon, height)[0], pos)
                assert eq(O.ecef_from_horizontal(lat, lon, az, el), d)
            for name in PC.settings(case):
                slope, resolution = PC.SETTINGS[name]
                k = f"{case}_{recipe}_{name}_"
                t = geo.trace(pos, d, max_steps=PC.MAX_STEPS, slope=slope, resolution=resolution, threads=4)
                assert eq(t["index"], g[k + "index"].astype(np.int32)), k
                assert eq(t["n_steps"], g[k + "n_steps"]) and eq(t["length"], g[k + "length"]), k
                assert (t["n_steps"] < PC.MAX_STEPS).all(), k
    assert "rough_c2_steep_index" not in g
