"""Compressed GeoTIFF-16 tiles in the native reader (turtle_amd/csrc/tiff.c): LZW, Deflate and
PackBits strips, the horizontal predictor, either byte order [ref io/geotiff16.c:165-258 reads
them all through libtiff].

The fixtures under tests/golden come from libtiff's ENCODERS (Pillow; see
generate_tiff_compressed.py, which also had the reference read every one of them); what Pillow
cannot write comes from the writers of tiff_cases.py, which the same script had libtiff and the
reference read.  Host side only: no GPU."""
import ctypes as C
import os
import zlib

import numpy as np
import pytest

import turtle_amd as TA
from turtle_amd import binding

import tiff_cases as TC

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = ("lzw_p2_r8", "lzw_p1_r1", "deflate_p2_r16", "packbits_r5", "lzw_full_table")


def fixture_path(name):
    return os.path.join(HERE, "golden", name + ".tif")


def fixture_nodes(g, name):
    return g["lzw_full_table"] if name == "lzw_full_table" else g["terrain"]


def nodes_of(m, nx, ny):
    """every node of a map, [row south->north]"""
    return np.array([[m.node(ix, iy)[2] for ix in range(nx)] for iy in range(ny)])


def load_nodes(path, shape):
    m = TA.Map.load(path)
    try:
        meta = m.meta()
        assert (meta["ny"], meta["nx"]) == tuple(shape)
        return nodes_of(m, meta["nx"], meta["ny"])
    finally:
        m.destroy()


@pytest.fixture(scope="module")
def terrain(golden):
    """the 53 x 37 nodes of the fixtures: noise, and a block of voids where the predictor wraps"""
    z = golden("tiff_compressed")["terrain"]
    assert z.shape == (37, 53) and (z == -32768).sum() == 12
    return z


@pytest.mark.parametrize("name", FIXTURES)
def test_fixtures_from_libtiff_load(golden, name):
    """every node and the meta data of files that libtiff wrote"""
    g = golden("tiff_compressed")
    m = TA.Map.load(fixture_path(name))
    meta = m.meta()
    nodes = fixture_nodes(g, name)
    ny, nx = nodes.shape
    assert (meta["nx"], meta["ny"]) == (nx, ny)
    assert meta["x"] == tuple(g[name + "_x"]) and meta["y"] == tuple(g[name + "_y"])
    assert meta["z"] == tuple(g[name + "_z"])
    assert meta["encoding"] == "tif" and meta["projection"] is None
    assert np.array_equal(nodes_of(m, nx, ny), nodes)
    m.destroy()


@pytest.mark.parametrize("order", ["II", "MM"])
@pytest.mark.parametrize("predictor", [1, 2])
@pytest.mark.parametrize("compression", [TC.DEFLATE, TC.DEFLATE_OLD])
def test_deflate_writer_of_our_own(tmp_path, terrain, order, predictor, compression):
    """zlib streams from the standard library: both byte orders (big-endian with the predictor
    and voids is where adding before swapping shows), both Deflate tags, strips of 1, 7 and all
    rows, an odd width (53)"""
    for rps in (1, 7, None):
        p = TC.write_tiff(str(tmp_path / f"d_{rps}.tif"), terrain, order=order, compression=compression,
                          predictor=predictor, rows_per_strip=rps, x0=3.0, y_top=46.0, dx=0.5, dy=0.25)
        m = TA.Map.load(p)
        assert m.meta()["x"] == (3.0, 3.0 + 52 * 0.5) and m.meta()["y"] == (46.0 - 36 * 0.25, 46.0)
        assert np.array_equal(nodes_of(m, 53, 37), terrain), rps
        m.destroy()


@pytest.mark.parametrize("order", ["II", "MM"])
@pytest.mark.parametrize("compression,predictor", [(TC.LZW, 1), (TC.LZW, 2), (TC.PACKBITS, 1)])
def test_lzw_and_packbits_in_both_byte_orders(tmp_path, terrain, compression, predictor, order):
    """(big-endian LZW and PackBits files: not among the fixtures, Pillow writes little-endian)"""
    for rps in (1, 7, None):
        p = TC.write_tiff(str(tmp_path / "t.tif"), terrain, order=order, compression=compression,
                          predictor=predictor, rows_per_strip=rps)
        assert np.array_equal(load_nodes(p, terrain.shape), terrain), rps


@pytest.mark.parametrize("order", ["II", "MM"])
def test_two_strips_with_short_offsets_and_counts_in_the_directory(tmp_path, terrain, order):
    """two SHORTs share a directory entry's value field, the first strip's in its first bytes"""
    small = terrain[:6, :9]

    for compression in (TC.NONE, TC.DEFLATE):
        raw = TC.tiff_bytes(small, order=order, compression=compression, rows_per_strip=3, inline_shorts=True)
        p = str(tmp_path / "s.tif")
        with open(p, "wb") as f:
            f.write(raw)
        assert np.array_equal(load_nodes(p, small.shape), small), compression


def test_predictor_tag_without_a_codec_that_knows_it(tmp_path, terrain):
    """libtiff has the predictor for LZW and Deflate only: with PackBits or no compression the
    tag is ignored (and an uncompressed file reads as it always did)"""
    for compression in (TC.NONE, TC.PACKBITS):
        p = TC.write_tiff(str(tmp_path / "t.tif"), terrain, compression=compression, rows_per_strip=5,
                          tags=((317, 3, 2),))
        assert np.array_equal(load_nodes(p, terrain.shape), terrain)


# ---- row bands ---------------------------------------------------------------------------------

def _read_rows(path, m, iy0, iy1):
    L = TA.lib()
    L.tamd_tiff_read_rows.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_int]
    return L.tamd_tiff_read_rows(os.fsencode(path), m.h, iy0, iy1)


@pytest.mark.parametrize("name,rows_per_strip", [("lzw_p2_r8", 8), ("deflate_p2_r16", 16), ("packbits_r5", 5),
                                                 ("lzw_p1_r1", 1), ("own_mm_whole", 37)])
def test_row_ranges_that_start_and_end_inside_strips(tmp_path, terrain, name, rows_per_strip):
    """tamd_tiff_read_rows, the reader of the page-in crew's bands: rows iy0 .. iy1 - 1 of the
    file go to their places, no other row is touched, and bands that tile the map give the
    whole-file read"""
    if name == "own_mm_whole":
        path = TC.write_tiff(str(tmp_path / "w.tif"), terrain, order="MM", predictor=2)
    else:
        path = fixture_path(name)
    ny, nx = terrain.shape
    blank = TC.write_tiff(str(tmp_path / "blank.tif"), np.full_like(terrain, 7), compression=TC.NONE)
    for iy0, iy1 in ((0, 1), (3, 11), (8, 24), (13, 14), (30, 37), (0, 37), (5, 5)):
        m = TA.Map.load(blank)
        assert _read_rows(path, m, iy0, iy1) == 0
        want = np.full_like(terrain, 7)
        want[iy0:iy1] = terrain[iy0:iy1]
        assert np.array_equal(nodes_of(m, nx, ny), want), (iy0, iy1)
        m.destroy()
    m = TA.Map.load(blank)
    for iy0 in range(0, ny, 8):             # the crew's bands: whole blocks of 8 rows
        assert _read_rows(path, m, iy0, min(iy0 + 8, ny)) == 0
    assert np.array_equal(nodes_of(m, nx, ny), terrain)
    assert _read_rows(path, m, 30, 38) != 0 and _read_rows(path, m, -1, 4) != 0   # outside the file
    m.destroy()


class _TileJob(C.Structure):
    _fields_ = [("path", C.c_char_p), ("staged", C.c_void_p), ("staged_bytes", C.c_size_t),
                ("cached", C.c_int), ("map", C.c_void_p), ("rc", C.c_int)]


def _blocked(nodes):
    """the HBM layout (internal.h): blocks of 8 x 8 nodes, block rows south -> north, zero padded"""
    ny, nx = nodes.shape
    nby, nbx = (ny + 7) // 8, (nx + 7) // 8
    padded = np.zeros((nby * 8, nbx * 8), dtype=np.uint16)
    padded[:ny, :nx] = nodes.view(np.uint16)
    return padded.reshape(nby, 8, nbx, 8).transpose(0, 2, 1, 3).ravel()


def test_page_in_crew_decodes_compressed_tiles_in_bands(tmp_path, golden):
    """tamd_tiles_decode, the host half of a stack's page-in (worker threads, bands of rows,
    nodes laid out in a staging buffer): files of many strips, of fewer strips than the crew
    would cut bands, and of one strip, side by side with a raw one"""
    g = golden("tiff_compressed")
    big = g["lzw_full_table"]                                   # 96 x 64
    files = [(fixture_path("lzw_full_table"), big),             # one strip: one band
             (fixture_path("lzw_p2_r8"), g["terrain"]),
             (TC.write_tiff(str(tmp_path / "a.tif"), big, order="MM", predictor=2, rows_per_strip=24), big),
             (TC.write_tiff(str(tmp_path / "b.tif"), big, compression=TC.LZW, predictor=2, rows_per_strip=1), big),
             (TC.write_tiff(str(tmp_path / "c.tif"), big, compression=TC.PACKBITS, rows_per_strip=9), big),
             (TC.write_tiff(str(tmp_path / "d.tif"), big, compression=TC.NONE, rows_per_strip=5), big)]
    L = TA.lib()
    L.tamd_tiles_decode.restype = None
    L.tamd_blocked_bytes.restype = C.c_size_t
    for n in (len(files), 1):               # 1 tile: the crew cuts it in as many bands as it has threads
        jobs = (_TileJob * n)()
        buffers = []
        for k in range(n):
            ny, nx = files[k][1].shape
            size = L.tamd_blocked_bytes(nx, ny)
            assert size == _blocked(files[k][1]).nbytes
            buffers.append(np.full(size // 2, 0xABCD, dtype=np.uint16))
            jobs[k].path = os.fsencode(files[k][0])
            jobs[k].staged, jobs[k].staged_bytes = buffers[k].ctypes.data, size
        L.tamd_tiles_decode(jobs, n)
        for k in range(n):
            assert jobs[k].rc == 0 and jobs[k].map, files[k][0]
            ny, nx = files[k][1].shape
            m = TA.Map(C.c_void_p(jobs[k].map))
            assert np.array_equal(nodes_of(m, nx, ny), files[k][1]), files[k][0]
            assert np.array_equal(buffers[k], _blocked(files[k][1])), files[k][0]
            m.destroy()
    # a tile with a damaged strip: BAD_FORMAT for that tile, the others come in
    bad = TC.write_tiff(str(tmp_path / "bad.tif"), big, rows_per_strip=8,
                        mangle=lambda chunks: chunks[:3] + [chunks[3][:len(chunks[3]) // 2]] + chunks[4:])
    jobs = (_TileJob * 2)()
    jobs[0].path, jobs[1].path = os.fsencode(bad), os.fsencode(files[0][0])
    L.tamd_tiles_decode(jobs, 2)
    assert jobs[0].rc == binding.RETURN_NAMES.index("BAD_FORMAT") and not jobs[0].map
    assert jobs[1].rc == 0
    m = TA.Map(C.c_void_p(jobs[1].map))
    assert np.array_equal(nodes_of(m, 96, 64), big)
    m.destroy()


# ---- refusals ----------------------------------------------------------------------------------

def _refused(path):
    with pytest.raises(TA.TurtleError) as e:
        TA.Map.load(path)
    assert e.value.name == "BAD_FORMAT", str(e.value)
    return str(e.value)


def test_headers_that_are_refused(tmp_path, terrain):
    p = str(tmp_path / "t.tif")
    for how in (dict(compression=7, codec=TC.NONE),                  # JPEG
                dict(compression=50000, codec=TC.DEFLATE),           # ZSTD
                dict(compression=TC.DEFLATE, predictor=3),           # floating point predictor
                dict(compression=TC.LZW, tags=((317, 3, 3),)),
                dict(compression=TC.DEFLATE, tags=((266, 3, 2),)),   # FillOrder 2
                dict(compression=TC.NONE, tags=((266, 3, 2),)),
                dict(compression=TC.DEFLATE, counts=False),          # no StripByteCounts
                dict(compression=TC.LZW, counts=False, rows_per_strip=5),
                dict(compression=TC.DEFLATE, tags=((322, 3, 16),))):  # tiled
        message = _refused(TC.write_tiff(p, terrain, **how))
        assert "missing data" not in message, how    # refused from the header, before any strip is read

    # as many byte counts as there are not strips
    def fewer(entries):
        typ, n, at = entries[279]
        entries[279] = (typ, n - 1, at)
    _refused(TC.write_tiff(p, terrain, rows_per_strip=5, edit=fewer))

    # a strip that ends beyond the end of the file: its count, or its offset
    def long_count(entries):
        entries[279] = (4, 1, 1 << 20)
    assert "missing data" not in _refused(TC.write_tiff(p, terrain, edit=long_count))

    def far_offset(entries):
        entries[273] = (4, 1, 0xFFFFFFF0)
    assert "missing data" not in _refused(TC.write_tiff(p, terrain, edit=far_offset))
    raw = TC.tiff_bytes(terrain, rows_per_strip=4)
    # ... and BigTIFF's version number
    with open(p, "wb") as f:
        f.write(raw[:2] + b"\x2b\x00" + raw[4:])
    _refused(p)
    # the same files, uncompressed and without byte counts, load as they always did
    ok = TC.write_tiff(p, terrain, compression=TC.NONE, counts=False, rows_per_strip=5)
    assert np.array_equal(load_nodes(ok, terrain.shape), terrain)


def test_damaged_strips_are_missing_data(tmp_path, terrain):
    p = str(tmp_path / "t.tif")

    def halve(which):
        return lambda chunks: [c[:len(c) // 2] if k == which else c for k, c in enumerate(chunks)]

    for compression in (TC.DEFLATE, TC.LZW, TC.PACKBITS):
        for rps, which in ((None, 0), (8, 2)):
            message = _refused(TC.write_tiff(p, terrain, compression=compression, rows_per_strip=rps,
                                             mangle=halve(which)))
            assert "missing data when reading file" in message
    # a strip that holds FEWER rows than the directory says (encoded from a shorter image)
    short = zlib.compress(terrain[::-1][:30].astype("<i2").tobytes())
    assert "missing data" in _refused(TC.write_tiff(p, terrain, mangle=lambda c: [short]))
    # PackBits that would run beyond its rows: all but the last 4 bytes of the strip, then a run
    # of 128 or a literal of 128 (and, for comparison, the 4 bytes that do fit)
    rows = terrain[::-1].astype("<i2").tobytes()
    body = TC.encode_strip(rows[:-106], TC.PACKBITS, 106) + bytes([101]) + rows[-106:-4]
    for tail, fits in ((bytes([0x81, 0x55]), False), (bytes([127]) + bytes(128), False), (bytes([3]) + rows[-4:], True)):
        path = TC.write_tiff(p, terrain, compression=TC.PACKBITS, mangle=lambda c: [body + tail])
        if fits:
            assert np.array_equal(load_nodes(path, terrain.shape), terrain)
        else:
            assert "missing data" in _refused(path)
    # LZW: raw samples under the tag, the LSB-first variant of old writers (its Clear reads as
    # code 0 or 1), a stream that never clears, EOI too early
    first = TC.lzw_encode(terrain[::-1].astype("<i2").tobytes())
    for stream in (terrain[::-1].astype("<i2").tobytes(), bytes([0x00, 0x01]) + first[2:],
                   first[2:], bytes([0x80, 0x40, 0x40])):
        assert "missing data" in _refused(TC.write_tiff(p, terrain, compression=TC.LZW, mangle=lambda c: [stream]))
    # trailing input after a full strip is ignored
    ok = TC.write_tiff(p, terrain, compression=TC.LZW, rows_per_strip=8, mangle=lambda c: [x + b"\xff\x00\x81" for x in c])
    assert np.array_equal(load_nodes(ok, terrain.shape), terrain)


@pytest.mark.parametrize("name", ["lzw_full_table", "lzw_p2_r8", "deflate_p2_r16", "packbits_r5"])
def test_flipped_bytes_never_overrun(tmp_path, golden, name):
    """one byte of strip data flipped, at many places in turn: BAD_FORMAT, or a map of the right
    size (which the sanitizer build of scripts/asan_cpu.sh watches for overruns)"""
    raw = bytearray(open(fixture_path(name), "rb").read())
    g = fixture_nodes(golden("tiff_compressed"), name)
    strips = TC.strips_of(bytes(raw))
    spots = [offset + k for offset, count in strips for k in range(count)]
    p = str(tmp_path / "flipped.tif")
    for k in range(40):
        where = spots[(k * 2654435761) % len(spots)]
        damaged = bytearray(raw)
        damaged[where] ^= 1 << (k % 8) if k % 3 else 0xFF
        with open(p, "wb") as f:
            f.write(damaged)
        try:
            m = TA.Map.load(p)
        except TA.TurtleError as e:
            assert e.name == "BAD_FORMAT"
            continue
        assert (m.meta()["ny"], m.meta()["nx"]) == g.shape
        m.node(g.shape[1] - 1, g.shape[0] - 1)
        m.destroy()
