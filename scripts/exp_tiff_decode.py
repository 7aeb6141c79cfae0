#!/usr/bin/env python3
"""What reading a compressed GeoTIFF tile costs on the host (turtle_amd/csrc/tiff.c), against
libtiff on the same files.  No GPU: the decoders and the page-in crew (tiles.c) touch files and
host memory only.

One 3601 x 3601 tile (synthetic SRTM-like ground plus +-3 m of noise a node, so that the
compressors have something to do) is written by libtiff (Pillow) raw and with each codec, with
and without the horizontal predictor, and timed (best of --repeat):

  load      turtle_map_load, one thread
  crew16    16 copies of the tile through tamd_tiles_decode into staging buffers in the HBM
            layout, as a round of a paged batch brings them in (worker threads, bands of rows)
  libtiff   Pillow's Image.load() of the same file: libtiff's decoders, one thread

    python scripts/exp_tiff_decode.py [--n 3601] [--rows-per-strip 1] [--repeat 3]
"""
import argparse
import ctypes as C
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import turtle_amd as TA  # noqa: E402
from turtle_amd import synth  # noqa: E402

CASES = (("raw", "raw", 1), ("lzw", "tiff_lzw", 1), ("lzw+p2", "tiff_lzw", 2),
         ("deflate", "tiff_adobe_deflate", 1), ("deflate+p2", "tiff_adobe_deflate", 2),
         ("packbits", "packbits", 1))


class TileJob(C.Structure):
    _fields_ = [("path", C.c_char_p), ("staged", C.c_void_p), ("staged_bytes", C.c_size_t),
                ("cached", C.c_int), ("map", C.c_void_p), ("rc", C.c_int)]


def best(f, repeat):
    times = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        f()
        times.append(time.perf_counter() - t0)
    return min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=synth.HGT_N)
    ap.add_argument("--rows-per-strip", type=int, default=1,
                    help="1 is what GDAL writes for a tile this wide (strips of about 8 KB)")
    ap.add_argument("--repeat", type=int, default=3)
    args = ap.parse_args()
    from PIL import Image, features
    from PIL.TiffImagePlugin import ImageFileDirectory_v2
    Image.MAX_IMAGE_PIXELS = None
    n = args.n
    nodes = synth.srtm_like_nodes(45, 3, n).astype(np.int32)
    iy, ix = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    nodes += (synth._hash32(ix, iy, 7) % np.uint64(7)).astype(np.int32) - 3
    nodes = nodes.astype(np.int16)
    L = TA.lib()
    L.tamd_tiles_decode.restype = None
    L.tamd_blocked_bytes.restype = C.c_size_t
    size = L.tamd_blocked_bytes(n, n)
    buffers = [np.zeros(size // 2, dtype=np.uint16) for _ in range(16)]
    d = tempfile.mkdtemp(prefix="tiff_decode_")
    print(f"{n} x {n} nodes, {args.rows_per_strip} row(s) a strip, libtiff {features.version('libtiff')}, "
          f"{len(os.sched_getaffinity(0))} cores")
    print(f"{'codec':<11}{'file MB':>8}{'load ms':>9}{'crew16 ms':>10}{'a tile':>8}{'libtiff ms':>11}{'load/libtiff':>13}")
    try:
        for name, compression, predictor in CASES:
            path = os.path.join(d, name.replace("+", "_") + ".tif")
            info = ImageFileDirectory_v2()
            info[33550] = (1.0 / (n - 1), 1.0 / (n - 1), 0.0)
            info[33922] = (0.0, 0.0, 0.0, 3.0, 46.0, 0.0)
            info[278] = args.rows_per_strip
            if predictor != 1:
                info[317] = predictor
            Image.fromarray(np.ascontiguousarray(nodes[::-1]).view(np.uint16)).save(
                path, compression=compression, tiffinfo=info)
            copies = []
            for k in range(16):
                copies.append(os.path.join(d, f"copy{k:02d}_" + os.path.basename(path)))
                shutil.copyfile(path, copies[-1])

            def load():
                m = TA.Map.load(path)
                z = m.node(n // 3, n // 2)[2]
                m.destroy()
                assert z == nodes[n // 2, n // 3]

            def crew():
                jobs = (TileJob * 16)()
                for k in range(16):
                    jobs[k].path = os.fsencode(copies[k])
                    jobs[k].staged, jobs[k].staged_bytes = buffers[k].ctypes.data, size
                L.tamd_tiles_decode(jobs, 16)
                for k in range(16):
                    assert jobs[k].rc == 0
                    TA.Map(C.c_void_p(jobs[k].map)).destroy()

            def libtiff():
                with Image.open(path) as im:
                    im.load()

            t_load, t_crew, t_lib = best(load, args.repeat), best(crew, args.repeat), best(libtiff, args.repeat)
            print(f"{name:<11}{os.path.getsize(path) / 1e6:>8.1f}{1e3 * t_load:>9.1f}{1e3 * t_crew:>10.1f}"
                  f"{1e3 * t_crew / 16:>8.1f}{1e3 * t_lib:>11.1f}{t_load / t_lib:>13.2f}")
            for p in copies + [path]:
                os.remove(p)
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    main()
