"""Stacks of compressed GeoTIFF tiles on the GPU: the kernels and the paging see the nodes of the
same tiles written uncompressed, so every answer is the same bit for bit -- no tolerance.  (The
decoders themselves are pinned on the host, against libtiff's output: test_tiff_compressed.py.)"""

import numpy as np
import pytest

import turtle_amd as TA
from turtle_amd import synth

import tiff_cases as TC

pytestmark = pytest.mark.gpu

# how each tile of a 2 x 2 stack is written: the issue's mix (zlib streams from the standard
# library), and one with the LZW and PackBits writers of tiff_cases.py
MIXES = {
    "deflate": (dict(compression=TC.DEFLATE, predictor=2, rows_per_strip=8),
                dict(compression=TC.DEFLATE_OLD, rows_per_strip=1),
                dict(compression=TC.DEFLATE, predictor=2, order="MM"),
                dict(compression=TC.NONE, rows_per_strip=16)),
    "lzw_packbits": (dict(compression=TC.LZW, predictor=2, rows_per_strip=8),
                     dict(compression=TC.PACKBITS, rows_per_strip=5),
                     dict(compression=TC.LZW, order="MM", rows_per_strip=1),
                     dict(compression=TC.LZW, predictor=2)),
}


def _tile_nodes(la, lo, n):
    nodes = synth.rough_nodes(n, seed=1 + 7 * la + lo, amplitude=600, noise=40)
    return synth.with_voids(nodes, [(n // 2, n // 2 + 3, n // 3, n // 3 + 4)]) if (la + lo) % 2 else nodes


def _write_stack(directory, tiles, n, how):
    for k, (la, lo) in enumerate(tiles):
        TC.write_tile(directory, la, lo, _tile_nodes(la, lo, n), **how[k % len(how)])
    return directory


RESIDENT_TILES = [(45, 3), (45, 4), (46, 3), (46, 4)]


@pytest.fixture(scope="module")
def resident_raw(tmp_path_factory):
    return _write_stack(str(tmp_path_factory.mktemp("tif") / "raw"), RESIDENT_TILES, 121,
                        (dict(compression=TC.NONE),))


@pytest.mark.parametrize("mix", sorted(MIXES))
def test_resident_stack_of_compressed_tiles(tmp_path, resident_raw, mix):
    d = _write_stack(str(tmp_path / mix), RESIDENT_TILES, 121, MIXES[mix])
    raw, packed = TA.Stack(resident_raw, 0), TA.Stack(d, 0)
    raw.load(), packed.load()
    assert raw.resident == 4 and packed.resident == 4
    rng = np.random.default_rng(11)
    n = 4096
    lat, lon = rng.uniform(44.95, 47.05, n), rng.uniform(2.95, 5.05, n)
    lat[:256] = np.round(lat[:256])              # on the seams, and on the stack's edges
    lon[256:512] = np.round(lon[256:512])
    z0, in0 = raw.elevation(lat, lon)
    z1, in1 = packed.elevation(lat, lon)
    assert in0.sum() > 3000 and np.array_equal(in0, in1) and np.array_equal(z0, z1)
    s0, s1 = TA.Stepper(), TA.Stepper()
    s0.add_stack(raw, 0.0), s1.add_stack(packed, 0.0)
    la, lo, az, el = synth.uniform_rays(2048, (45.0, 47.0), (3.0, 5.0), seed=5)
    p0, d0 = s0.position(la, lo, 300.0)
    p1, d1 = s1.position(la, lo, 300.0)
    assert np.array_equal(p0, p1) and np.array_equal(d0, d1) and (d0 == 0).all()
    dirs = TA.ecef_from_horizontal(la, lo, az, el)
    try:
        for math in ("strict", "fast"):
            TA.set_math(math)
            a, b = s0.trace(p0.copy(), dirs), s1.trace(p0.copy(), dirs)
            assert int(a["n_steps"].sum()) > 2048
            for key in ("position", "index", "length", "n_steps"):
                assert np.array_equal(a[key], b[key]), (math, key)
    finally:
        TA.set_math("fast")
    for o in (s0, s1, raw, packed):
        o.destroy()


PAGED_TILES = [(la, lo) for la in range(40, 44) for lo in range(5, 10)]     # 4 x 5 = 20 tiles
PAGED_HOW = MIXES["deflate"][:3] + MIXES["lzw_packbits"]


@pytest.fixture(scope="module")
def paged_dirs(tmp_path_factory):
    root = tmp_path_factory.mktemp("paged")
    return (_write_stack(str(root / "raw"), PAGED_TILES, 65, (dict(compression=TC.NONE),)),
            _write_stack(str(root / "packed"), PAGED_TILES, 65, PAGED_HOW))


@pytest.mark.parametrize("math", ["strict", "fast"])
def test_paged_stack_of_compressed_tiles(paged_dirs, math):
    """20 tiles through a stack that keeps one: the crew decodes bands of compressed tiles into
    the staging buffers, round after round.  STRICT arithmetic is where a paged trace promises the
    bits of a resident one whatever the order its tiles came in: there the compressed
    stack gives the uncompressed one's bits, paged and resident.  In FAST a ray that waited for a
    tile carries on along a new line, and how many rounds a batch takes depends on when staging
    buffers come free (50 and 56 rounds were seen for these two stacks in one run), so two paged
    runs agree to the 1e-9 of tests/test_gpu_paging.py, index and step count exactly."""
    raw, packed = TA.Stack(paged_dirs[0], 1), TA.Stack(paged_dirs[1], 1)
    full = TA.Stack(paged_dirs[0], 0)
    full.load()
    steppers = [TA.Stepper() for _ in range(3)]
    for st, stack in zip(steppers, (raw, packed, full)):
        st.add_stack(stack, 0.0)
    la, lo, az, el = synth.uniform_rays(2048, (40.0, 44.0), (5.0, 10.0), seed=9, margin=0.02,
                                        el_range=(-12.0, 2.0))
    p, di = steppers[2].position(la, lo, 400.0)
    assert (di == 0).all()
    assert len({(int(a), int(b)) for a, b in zip(np.floor(la), np.floor(lo))}) == 20
    dirs = TA.ecef_from_horizontal(la, lo, az, el)
    TA.set_math(math)
    try:
        a = steppers[0].trace(p.copy(), dirs)
        b = steppers[1].trace(p.copy(), dirs)
        assert steppers[1].rounds > 1 and steppers[0].rounds > 1
        assert packed.resident <= 1
        if math == "strict":
            c = steppers[2].trace(p.copy(), dirs)
            for key in ("position", "index", "length", "n_steps"):
                assert np.array_equal(a[key], b[key]) and np.array_equal(c[key], b[key]), key
        else:
            assert np.array_equal(a["index"], b["index"]) and np.array_equal(a["n_steps"], b["n_steps"])
            rel = np.abs(a["length"] - b["length"]) / np.maximum(a["length"], 1e-300)
            assert rel.max() < 1e-9 and np.abs(a["position"] - b["position"]).max() < 1e-5
        lat1, lon1, _ = TA.ecef_to_geodetic(b["position"])
        assert ((np.floor(lat1) != np.floor(la)) | (np.floor(lon1) != np.floor(lo))).sum() > 50
    finally:
        TA.set_math("fast")
    for o in steppers + [raw, packed, full]:
        o.destroy()


def test_host_scalar_reads_a_compressed_tile_again(paged_dirs):
    """A tile that comes back from a staging buffer has no host copy of its nodes: the host scalar
    path reads the (compressed) file when it first needs them, and answers as the device does"""
    full, small = TA.Stack(paged_dirs[0], 0), TA.Stack(paged_dirs[1], 1)
    full.load()
    rng = np.random.default_rng(3)
    boxes = {"a": (40, 5), "b": (40, 6), "c": (41, 5)}      # Deflate + predictor 2, 32946, big-endian LZW
    pts = {k: (rng.uniform(la + 0.01, la + 0.99, 500), rng.uniform(lo + 0.01, lo + 0.99, 500))
           for k, (la, lo) in boxes.items()}
    for k in "abcabacbca":
        z0, in0 = full.elevation(*pts[k])
        z1, in1 = small.elevation(*pts[k])
        assert in0.all() and np.array_equal(in0, in1) and np.array_equal(z0, z1), k
        TA.set_scalar("host")
        try:
            zs = [small.elevation_scalar(float(pts[k][0][i]), float(pts[k][1][i]))[0] for i in range(8)]
        finally:
            TA.set_scalar("device")
        assert zs == list(z0[:8]), k
    full.destroy()
    small.destroy()
