"""Which rays count at slope and resolution other than the defaults (tests/params_cases.py): the
mask of ill-conditioned rays, computed by the CPU restatement alone, stays under its caps for every
batch the GPU tests (tests/test_gpu_params.py) hold to the bar, and those batches exercise what they
are for.  No GPU."""
import numpy as np
import pytest

import params_cases as PC
import traverse_cases as TC


def test_checkers_take_slope_and_resolution(golden):
    """the keyword arguments of the four CPU checkers reach their C loops: traverse's loop with no
    ceiling is the trace of params.npz where a ray's first change of medium is its last (it leaves
    the data), and the defaults are what they were"""
    import advance_cases as AC
    import advance_exp_cases as AE
    import crossings_cases as CR
    g = golden("params")
    geo = TC.oracle_geometry("hgt")
    pos, d = g["hgt_ground_position"][:200], g["hgt_ground_direction"][:200]
    for name in ("example", "coarse"):
        slope, resolution = PC.SETTINGS[name]
        k = f"hgt_ground_{name}_"
        left = g[k + "index"][:200, 0] == -1
        assert left.sum() > 100
        t = TC.check(geo, pos, d, slope=slope, resolution=resolution)
        c = CR.check(geo, pos, d, slope=slope, resolution=resolution)
        rho = AC.DENSITY[2]
        a = AC.check(geo, pos, d, rho, np.full(200, np.inf), slope=slope, resolution=resolution)
        e = AE.check(geo, pos, d, rho, AE.SCALE_HEIGHT[2], np.full(200, np.inf), slope=slope,
                     resolution=resolution)
        for got in (t, c, a, e):
            assert np.array_equal(got["n_steps"][left], g[k + "n_steps"][:200][left])
        assert np.array_equal(t["length"][1][left], g[k + "length"][:200][left])
        assert np.array_equal(a["distance"][left], g[k + "length"][:200][left])
        assert not np.array_equal(t["n_steps"], TC.check(geo, pos, d)["n_steps"])
    assert np.array_equal(TC.check(geo, pos, d, slope=0.4, resolution=1e-2)["length"],
                          TC.check(geo, pos, d)["length"])


def traced_cells(golden):
    """every batch test_gpu_params.py traces to a first change of medium: (key, geometry, origins,
    directions, case, setting)"""
    g = golden("params")
    for case in PC.CASES:
        geo = TC.oracle_geometry(case)
        for name in PC.settings(case):
            pos = np.concatenate([g[f"{case}_{r}_position"] for r in PC.RECIPES])
            d = np.concatenate([g[f"{case}_{r}_direction"] for r in PC.RECIPES])
            yield (case, name), geo, pos, d, case, name
    geo = PC.stack_oracle()
    pos, d = PC.stack_rays()
    for name in PC.SETTINGS:
        yield ("stack", name), geo, pos, d, "stack", name


def test_masks_stay_under_their_caps(golden):
    """The mask over the full perturbation set (+-2e-9 m and +-1e-8 m along two seeded unit vectors:
    eight retraces) for every traced batch, recipe by recipe, and for every line-of-sight batch.

    Observed (masked rays of 1000 a recipe, ground / c2 / graze; of 2000 on the stack):
      hgt    every setting 0 / 0 / 0
      rough  example 1 / 12 / 18, mixed 1 / 11 / 18, fine, coarse and slow 0 / 0 / 0
      stack  fine 2, every other setting 0
      lines of sight ("hgt" and "two" at example, fine and coarse; ground and c2): 0 everywhere
    Every traced batch has rays beyond 32 steps, and beyond 512 but on the rough tile at slope 1
    (hgt: 38 .. 2268 of 3000; the longest ray takes 59 403 steps, at `slow`)."""
    for key, geo, pos, d, case, name in traced_cells(golden):
        slope, resolution = PC.SETTINGS[name]
        bad, base = PC.trace_mask(key, geo, pos, d, slope, resolution)
        n = PC.RAYS if case != "stack" else pos.shape[0]
        counts = [int(bad[i:i + n].sum()) for i in range(0, pos.shape[0], n)]
        print(f"{case:5s} {name:7s}: masked {counts}, beyond 32 steps {int((base['n_steps'] > 32).sum())}, "
              f"beyond 512 {int((base['n_steps'] > 512).sum())}, max {int(base['n_steps'].max())}")
        assert max(counts) <= PC.cap(case, name) * n, (key, counts)
        assert (base["n_steps"] < PC.MAX_STEPS).all(), key
        # the first pass, the hand-over and the lined pass all have rays
        assert (base["n_steps"] > 32).sum() > 50, key
        if case != "rough":
            assert (base["n_steps"] > 512).sum() > 10, key
    g = golden("traverse")
    for case in PC.SIGHT_CASES:
        geo = TC.oracle_geometry(case)
        for recipe in ("ground", "c2"):
            pos, d, ceiling = PC.sight_rays(case, recipe, g)
            for name in PC.SIGHT_SETTINGS:
                slope, resolution = PC.SETTINGS[name]
                bad, base = PC.traverse_mask((case, recipe, name), geo, pos, d, ceiling, slope, resolution)
                print(f"sight {case:3s} {recipe:6s} {name:7s}: masked {int(bad.sum())}, crossings max "
                      f"{int(base['n_crossings'].max())}, steps max {int(base['n_steps'].max())}")
                assert bad.sum() <= PC.cap(case, name) * bad.size, (case, recipe, name, int(bad.sum()))
    for recipe in ("ground", "c2"):          # traverse.npz's own "two" rays, where the mask allows
        pos, d, ceiling = PC.sight_rays("two", recipe, g, shallow=True)
        for name in PC.SHALLOW_SETTINGS:
            slope, resolution = PC.SETTINGS[name]
            bad, base = PC.traverse_mask(("two shallow", recipe, name), TC.oracle_geometry("two"), pos, d, ceiling,
                                         slope, resolution)
            print(f"sight two (the fixture's rays) {recipe:6s} {name:7s}: masked {int(bad.sum())}, crossings max "
                  f"{int(base['n_crossings'].max())}")
            assert bad.sum() <= PC.cap("two", name) * bad.size and base["n_crossings"].max() > 3
    # the generic step machine's batches (composite_cases' "layers")
    import composite_cases as CO
    geo = CO.oracle_geometry(PC.GENERIC_CASE)
    gpos, gd, _ = CO.graze(PC.GENERIC_CASE, geo)
    spos, sd = PC.generic_sight()
    assert spos.shape[0] > 1500
    for name in PC.GENERIC_SETTINGS:
        slope, resolution = PC.SETTINGS[name]
        bad, base = PC.trace_mask(("generic", name), geo, gpos, gd, slope, resolution)
        sbad, sbase = PC.traverse_mask(("generic sight", name), geo, spos, sd, CO.CEILING, slope, resolution,
                                       max_steps=CO.SIGHT_MAX_STEPS)
        print(f"generic {name:7s}: graze masked {int(bad.sum())} of {bad.size}, beyond 512 steps "
              f"{int((base['n_steps'] > 512).sum())}; sight masked {int(sbad.sum())} of {sbad.size}")
        assert bad.sum() <= 0.005 * bad.size and sbad.sum() <= 0.005 * sbad.size
        assert (base["n_steps"] > 512).sum() > 300 and (base["n_steps"] < PC.MAX_STEPS).all()
        assert (sbase["n_steps"] < CO.SIGHT_MAX_STEPS).all()


def test_edge_batches_and_named_rays(golden):
    """The edge batches (params_cases.EDGES) do what they are for in the restatement: no ray takes
    more than the 600 steps, at slope and resolution 0 every live ray ends at the cap with length 0,
    at a resolution of 1e-9 m rays reach the ground before the cap.  And every ray
    test_gpu_params.py names outside the bar is one the wider reference-only set flags and the mask
    does not."""
    import terrains as T
    geo = T.c1_oracle()
    for edge, (slope, resolution) in PC.EDGES.items():
        for pos, d in PC.edge_batches():
            with np.errstate(all="ignore"):
                base = geo.trace(pos.copy(), d, max_steps=PC.EDGE_MAX_STEPS, slope=slope, resolution=resolution)
            assert (base["n_steps"] <= PC.EDGE_MAX_STEPS).all()
            live = base["index"][:, 0] >= 0
            if edge == "no step at all":
                assert live.any() and (base["n_steps"][live] == PC.EDGE_MAX_STEPS).all()
                assert (base["length"][live] == 0).all()
            if edge == "resolution below the bracket" and pos.shape[0] == 65:
                assert ((base["index"][:, 0] == 0) & (base["n_steps"] > 400)).sum() >= 5
    g = golden("params")
    for what, rays in PC.OUTSIDE.items():
        _, case, name, _ = what.split()
        pos = np.concatenate([g[f"{case}_{r}_position"] for r in PC.RECIPES])[rays]
        d = np.concatenate([g[f"{case}_{r}_direction"] for r in PC.RECIPES])[rays]
        run = PC.trace_run(TC.oracle_geometry(case), d, *PC.SETTINGS[name])
        assert not PC.ill_conditioned(run, pos)[0].any(), what
        assert PC.ill_conditioned(run, pos, PC.wider_offsets())[0].all(), what


def test_the_mask_flags_what_moves():
    """ill_conditioned() on a made-up loop: a ray whose step count, index or length depends on the
    origin's last digits is flagged, one that moves by less than 1e-7 of its path is not"""
    pos = np.zeros((5, 3))

    def run(p):
        shift = p[0, 0] + p[0, 1] + p[0, 2]
        moved = shift != 0
        return dict(index=np.array([[0, 0], [0, 0], [int(moved) - 1, 0], [0, 0], [0, 0]], dtype=np.int32),
                    n_steps=np.array([3, 3 + int(moved), 3, 3, 3], dtype=np.int32),
                    length=np.array([10.0, 10.0, 10.0, 10.0 + 2e-6 * moved, 10.0 + 5e-7 * moved]))

    bad, base = PC.ill_conditioned(run, pos)
    assert bad.tolist() == [False, True, True, True, False]
    assert base["n_steps"].tolist() == [3] * 5
    off = PC.offsets()
    assert off.shape == (8, 3)
    assert np.allclose(np.linalg.norm(off, axis=1), [PC.TAU0] * 4 + [PC.BRACKET] * 4, rtol=1e-12)
    assert np.array_equal(off[0], -off[1]) and np.array_equal(off[6], -off[7])
