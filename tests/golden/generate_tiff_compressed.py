#!/usr/bin/env python3
"""Compressed GeoTIFF-16 fixtures from an encoder that is not ours: Pillow, whose TIFF writer
is libtiff (build container only; Pillow is not a test dependency).

  lzw_p2_r8.tif        LZW, predictor 2, 8 rows a strip        53 x 37 nodes
  lzw_p1_r1.tif        LZW, no predictor, 1 row a strip
  deflate_p2_r16.tif   Deflate (8), predictor 2, 16 rows a strip
  packbits_r5.tif      PackBits, 5 rows a strip
  lzw_full_table.tif   LZW, one strip of 96 x 64 noisy nodes: the encoder fills its table and
                       clears it in mid-strip (counted below, from the code stream)
  tiff_compressed.npz  the nodes (south -> north; `terrain` for the four 53 x 37 files) and the
                       meta data turtle_map_meta must give

Every file is read back through libtiff (Pillow) and, where oracle/_ref is built, through the
reference's turtle_map_load, whose dlopen("libtiff.so") needs the symlink generate_files.py
makes too.  The encoders of tests/tiff_cases.py are checked here as well: libtiff must read what
they write.
"""
import glob
import os
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.dirname(os.path.abspath(__file__))

X0, Y_TOP, DX, DY = 495000.0, 5068000.0, 10.0, 10.0
FILES = (("lzw_p2_r8", "tiff_lzw", 2, 8), ("lzw_p1_r1", "tiff_lzw", 1, 1),
         ("deflate_p2_r16", "tiff_adobe_deflate", 2, 16), ("packbits_r5", "packbits", 1, 5))


def reexec_with_links():
    d = tempfile.mkdtemp(prefix="turtle_links_")
    hits = sorted(glob.glob("/usr/lib/x86_64-linux-gnu/libtiff*.so.*"))
    if hits:
        os.symlink(hits[0], os.path.join(d, "libtiff.so"))
    env = dict(os.environ, LD_LIBRARY_PATH=d + ":" + os.environ.get("LD_LIBRARY_PATH", ""),
               TURTLE_LINKS_READY="1")
    sys.exit(subprocess.call([sys.executable, os.path.abspath(__file__)], env=env))


def terrain():
    """53 x 37 nodes, south -> north: smooth ground, +-20 m of noise a node, a block of voids"""
    rng = np.random.Generator(np.random.Philox(317))
    x, y = np.arange(53, dtype=np.float64), np.arange(37, dtype=np.float64)
    z = 900.0 + 500.0 * np.sin(x / 9.0)[None, :] * np.cos(y / 7.0)[:, None] + 6.0 * y[:, None]
    z = np.rint(z).astype(np.int64) + rng.integers(-20, 21, z.shape)
    z = z.astype(np.int16)
    z[20:23, 30:34] = -32768            # the predictor's differences wrap here
    return z


def noisy():
    """96 x 64 nodes of noise over a slope: ~12 KB that LZW cannot shrink, in one strip"""
    rng = np.random.Generator(np.random.Philox(4094))
    return (1500 + 3 * np.arange(96)[None, :] + rng.integers(-3000, 3001, (64, 96))).astype(np.int16)


def save(path, nodes_s2n, compression, predictor, rows_per_strip):
    from PIL import Image
    from PIL.TiffImagePlugin import ImageFileDirectory_v2
    info = ImageFileDirectory_v2()
    info[33550] = (DX, DY, 0.0)
    info[33922] = (0.0, 0.0, 0.0, X0, Y_TOP, 0.0)
    info[278] = rows_per_strip
    if predictor != 1:
        info[317] = predictor
    image = np.ascontiguousarray(nodes_s2n[::-1]).view(np.uint16)
    Image.fromarray(image).save(path, compression=compression, tiffinfo=info)


def libtiff_nodes(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im).astype(np.uint16).view(np.int16)[::-1]


def directory(path):
    """{tag: value or offset} of a little-endian file's first directory, and the file's bytes"""
    b = open(path, "rb").read()
    assert b[:2] == b"II"
    at, = struct.unpack_from("<I", b, 4)
    n, = struct.unpack_from("<H", b, at)
    tags = {}
    for i in range(n):
        tag, typ, cnt = struct.unpack_from("<HHI", b, at + 2 + 12 * i)
        val, = struct.unpack_from("<H" if typ == 3 else "<I", b, at + 10 + 12 * i)
        tags[tag] = (typ, cnt, val)
    return tags, b


def reference_nodes(path, nx, ny):
    from oracle import ref_ffi as R
    m = R.RefMap.load(path)
    z = np.array([[m.node(ix, iy)[2] for ix in range(nx)] for iy in range(ny)])
    m.destroy()
    return z


def main():
    import tiff_cases as TC
    from oracle import ref_ffi as R
    with_reference = R.available()
    out = {"x0": X0, "y_top": Y_TOP, "dx": DX, "dy": DY}
    cases = [(name, terrain(), *how) for name, *how in FILES]
    cases.append(("lzw_full_table", noisy(), "tiff_lzw", 1, 64))
    for name, z, compression, predictor, rps in cases:
        path = os.path.join(OUT, name + ".tif")
        save(path, z, compression, predictor, rps)
        ny, nx = z.shape
        tags, raw = directory(path)
        want = {"tiff_lzw": 5, "tiff_adobe_deflate": 8, "packbits": 32773}[compression]
        assert tags[259][2] == want and tags[278][2] == rps and tags.get(317, (3, 1, 1))[2] == predictor
        assert tags[273][1] == (ny + rps - 1) // rps and os.path.getsize(path) < 20 * 1024
        assert np.array_equal(libtiff_nodes(path), z), name
        if with_reference:
            assert np.array_equal(reference_nodes(path, nx, ny), z.astype(np.float64)), (name, R.errors())
        out["terrain" if z.shape == (37, 53) else name] = z     # (four files hold the same ground)
        out[name + "_x"] = np.array([X0, X0 + (nx - 1) * DX])
        out[name + "_y"] = np.array([Y_TOP - (ny - 1) * DY, Y_TOP])
        out[name + "_z"] = np.array([-32767.0, 32768.0])
        print(name, os.path.getsize(path), "bytes,", tags[273][1], "strips",
              "(reference agrees)" if with_reference else "(no reference build here)")
    # the one-strip file: its encoder did run out of table
    tags, raw = directory(os.path.join(OUT, "lzw_full_table.tif"))
    assert tags[273][1] == 1
    codes = list(TC.lzw_codes(raw[tags[273][2]:tags[273][2] + tags[279][2]]))
    clears = codes.count(256)
    assert codes[0] == 256 and codes[-1] == 257 and clears >= 2, clears
    print("lzw_full_table:", len(codes), "codes,", clears, "Clear codes")
    np.savez_compressed(os.path.join(OUT, "tiff_compressed.npz"), **out)
    # the writers of tests/tiff_cases.py, read by libtiff: through Pillow for little-endian files
    # (Pillow swaps the samples libtiff has already brought to host order, so it misreads every
    # compressed big-endian file, ours or not), through the reference for both byte orders
    with tempfile.TemporaryDirectory() as d:
        for z in (terrain(), noisy()):
            ny, nx = z.shape
            for compression in (TC.LZW, TC.PACKBITS, TC.DEFLATE, TC.DEFLATE_OLD):
                for order in ("II", "MM"):
                    for predictor in (1, 2):
                        if predictor == 2 and compression == TC.PACKBITS:
                            continue
                        for rps in (1, 7, None):
                            p = TC.write_tiff(os.path.join(d, "t.tif"), z, order=order, compression=compression,
                                              predictor=predictor, rows_per_strip=rps)
                            case = (compression, order, predictor, rps)
                            if order == "II":
                                assert np.array_equal(libtiff_nodes(p), z), case
                            if with_reference:
                                assert np.array_equal(reference_nodes(p, nx, ny), z.astype(np.float64)), case
    print("tiff_cases writers: read back by libtiff" + (" and by the reference" if with_reference else ""))


if __name__ == "__main__":
    if os.environ.get("TURTLE_LINKS_READY") != "1":
        reexec_with_links()
    main()
