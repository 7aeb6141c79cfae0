"""Writers of compressed GeoTIFF-16 tiles for the tests of turtle_amd/csrc/tiff.c: what Pillow's
libtiff cannot be made to write (big-endian files, Compression 32946, damaged strips, missing
tags), from the standard library alone.  The LZW and PackBits ENCODERS here are checked against
libtiff's decoders by tests/golden/generate_tiff_compressed.py; the library's decoders are
checked against libtiff's encoders through the fixtures that script writes."""
from __future__ import annotations

import os
import struct
import zlib

import numpy as np

NONE, LZW, DEFLATE, PACKBITS, DEFLATE_OLD = 1, 5, 8, 32773, 32946


def lzw_encode(data: bytes) -> bytes:
    """TIFF 6.0 LZW as libtiff writes it: MSB-first codes of 9 to 12 bits, a Clear (256) first and
    whenever the table is full, the width growing one code early, an EOI (257) last."""
    out = bytearray()
    acc = bits = 0

    def put(code, width):
        nonlocal acc, bits
        acc = (acc << width) | code
        bits += width
        while bits >= 8:
            bits -= 8
            out.append((acc >> bits) & 0xFF)
        acc &= (1 << bits) - 1

    table, free, width = {}, 258, 9
    put(256, width)
    prefix = None
    for byte in data:
        if prefix is None:
            prefix = byte
            continue
        key = (prefix, byte)
        if key in table:
            prefix = table[key]
            continue
        put(prefix, width)
        table[key] = free
        free += 1
        if free == 4094:            # libtiff's CODE_MAX - 1: start over
            put(256, width)
            table, free, width = {}, 258, 9
        elif free > (1 << width) - 1:
            width += 1
        prefix = byte
    if prefix is not None:
        put(prefix, width)
        # the decoder adds an entry for this code too, and may widen before the EOI
        if free + 1 > (1 << width) - 1 and width < 12:
            width += 1
    put(257, width)
    if bits:
        out.append((acc << (8 - bits)) & 0xFF)
    return bytes(out)


def packbits_encode(row: bytes) -> bytes:
    """one row (PackBits runs do not cross rows): repeats of 3 and more as runs, the rest literal"""
    out, i, n = bytearray(), 0, len(row)
    while i < n:
        j = i
        while j + 1 < n and row[j + 1] == row[i] and j - i < 127:
            j += 1
        if j - i >= 2:
            out += bytes([(256 - (j - i)) & 0xFF, row[i]])
            i = j + 1
            continue
        k = i
        while k < n and k - i < 128 and not (k + 2 < n and row[k] == row[k + 1] == row[k + 2]):
            k += 1
        out += bytes([k - i - 1]) + row[i:k]
        i = k
    return bytes(out)


def encode_strip(raw: bytes, compression: int, row_bytes: int) -> bytes:
    if compression == NONE:
        return raw
    if compression in (DEFLATE, DEFLATE_OLD):
        return zlib.compress(raw, 6)
    if compression == LZW:
        return lzw_encode(raw)
    if compression == PACKBITS:
        return b"".join(packbits_encode(raw[i:i + row_bytes]) for i in range(0, len(raw), row_bytes))
    raise ValueError(compression)


def tiff_bytes(nodes_s2n, order="II", compression=DEFLATE, predictor=1, rows_per_strip=None,
               x0=0.0, y_top=0.0, dx=1.0, dy=1.0, codec=None, counts=True, tags=(), edit=None,
               mangle=None, inline_shorts=False) -> bytes:
    """int16 nodes [row south->north] as a GeoTIFF of strips.  `codec`: the encoder to use when it
    is not the one `compression` names (a file that lies about itself); `counts=False` leaves
    StripByteCounts out; `tags`: more (tag, type, value) entries, replacing ours of the same tag;
    `mangle(list of encoded strips)`: damage done before the offsets are laid out; `edit(entries)`:
    the directory {tag: (type, count, value)} changed in place before it is written;
    `inline_shorts`: a file of two strips keeps their offsets and counts as two SHORTs in the entry."""
    e = "<" if order == "II" else ">"
    ny, nx = nodes_s2n.shape
    rps = rows_per_strip or ny
    image = np.ascontiguousarray(nodes_s2n[::-1]).astype(np.int16).view(np.uint16)
    if predictor == 2:
        image = np.concatenate([image[:, :1], (image[:, 1:] - image[:, :-1]).astype(np.uint16)], axis=1)
    image = image.astype(e + "u2")
    chunks = [encode_strip(image[r:r + rps].tobytes(), codec or compression, 2 * nx)
              for r in range(0, ny, rps)]
    if mangle is not None:
        chunks = mangle(chunks)
    data = b"".join(chunks)
    offs, at = [], 8
    for c in chunks:
        offs.append(at)
        at += len(c)
    cnts = [len(c) for c in chunks]
    base, blob = 8 + len(data), b""

    def extra(payload):
        nonlocal blob
        off = base + len(blob)
        blob += payload
        return off

    n = len(chunks)
    entries = {256: (4, 1, nx), 257: (4, 1, ny), 258: (3, 1, 16), 259: (3, 1, compression),
               262: (3, 1, 1), 277: (3, 1, 1), 278: (4, 1, rps), 339: (3, 1, 2)}
    if inline_shorts:
        assert n == 2 and at < 65536
        entries[273], entries[279] = (3, 2, tuple(offs)), (3, 2, tuple(cnts))
    else:
        entries[273] = (4, n, offs[0] if n == 1 else extra(struct.pack(e + f"{n}I", *offs)))
        if counts:
            entries[279] = (4, n, cnts[0] if n == 1 else extra(struct.pack(e + f"{n}I", *cnts)))
    if predictor != 1:
        entries[317] = (3, 1, predictor)
    entries[33550] = (12, 3, extra(struct.pack(e + "3d", dx, dy, 0.0)))
    entries[33922] = (12, 6, extra(struct.pack(e + "6d", 0, 0, 0, x0, y_top, 0)))
    for tag, typ, value in tags:
        entries[tag] = (typ, 1, value)
    if edit is not None:
        edit(entries)
    ifd = struct.pack(e + "H", len(entries))
    for tag in sorted(entries):
        typ, cnt, val = entries[tag]
        if isinstance(val, tuple):
            ifd += struct.pack(e + "HHIHH", tag, typ, cnt, *val)
        else:
            ifd += struct.pack(e + "HHIHH", tag, typ, cnt, val, 0) if typ == 3 else struct.pack(e + "HHII", tag, typ, cnt, val)
    ifd += struct.pack(e + "I", 0)
    return order.encode() + struct.pack(e + "HI", 42, base + len(blob)) + data + blob + ifd


def write_tiff(path, nodes_s2n, **how) -> str:
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "wb") as f:
        f.write(tiff_bytes(nodes_s2n, **how))
    return path


def write_tile(directory, lat0, lon0, nodes_s2n, **how) -> str:
    """a 1 x 1 degree tile of a stack, named as ASTER GDEM names its tiles"""
    from turtle_amd import synth
    step = 1.0 / (nodes_s2n.shape[0] - 1)
    return write_tiff(os.path.join(directory, synth.geotiff_name(lat0, lon0)), nodes_s2n,
                      x0=float(lon0), y_top=float(lat0 + 1), dx=step, dy=step, **how)


def strips_of(raw: bytes):
    """[(offset, byte count)] of the strips of a TIFF file, as its first directory gives them"""
    e = "<" if raw[:2] == b"II" else ">"
    at, = struct.unpack_from(e + "I", raw, 4)
    n, = struct.unpack_from(e + "H", raw, at)
    out = {}
    for i in range(n):
        tag, typ, cnt = struct.unpack_from(e + "HHI", raw, at + 2 + 12 * i)
        if tag not in (273, 279):
            continue
        code, size = ("H", 2) if typ == 3 else ("I", 4)
        where = at + 10 + 12 * i
        if cnt * size > 4:
            where, = struct.unpack_from(e + "I", raw, where)
        out[tag] = struct.unpack_from(e + f"{cnt}{code}", raw, where)
    return list(zip(out[273], out[279]))


def lzw_codes(data: bytes):
    """the codes of a TIFF LZW stream, following the decoder's table size for the widths"""
    acc = bits = 0
    width, free, fresh = 9, 258, True
    it = iter(data)
    while True:
        while bits < width:
            try:
                acc = (acc << 8) | next(it)
            except StopIteration:
                return
            bits += 8
        bits -= width
        code = (acc >> bits) & ((1 << width) - 1)
        acc &= (1 << bits) - 1
        yield code
        if code == 257:
            return
        if code == 256:
            width, free, fresh = 9, 258, True
        elif fresh:
            fresh = False
        else:
            free += 1
            if free > (1 << width) - 2 and width < 12:
                width += 1
