/*
 * tiff.c -- GeoTIFF-16 ingest without libtiff [ref src/turtle/io/geotiff16.c:
 * 165-258, which reads scan lines through a dlopen()ed libtiff].
 *
 * What is read: classic TIFF (version 42) in either byte order, one 16-bit
 * sample per pixel, in strips, with Compression (259) 1 (none: what the reference
 * itself writes), 5 (LZW: ASTER GDEM v3), 8 or 32946 (Deflate: a zlib stream per
 * strip; GDAL exports of SRTM) or 32773 (PackBits); with LZW and Deflate,
 * Predictor (317) 1 or 2 (horizontal differencing of the 16-bit samples), which
 * libtiff knows for these two codecs alone -- for the others the tag is ignored,
 * as libtiff ignores it.  The decoders are here; only zlib's inflate is borrowed,
 * as in png.c.
 *
 * What is refused, with BAD_FORMAT when the header is parsed: BigTIFF (version
 * 43), tiled files (322: the reference's scan line read fails on them too), any
 * other compression (JPEG, CCITT, LZMA, ZSTD ...), another predictor, FillOrder
 * (266) 2, other sample layouts, a compressed file without StripByteCounts (279)
 * or with as many counts as it has not strips, a strip of a compressed file that
 * ends beyond the end of the file.  A strip that does not decode to exactly its
 * rows is "missing data" (BAD_FORMAT + 100, host.h), as a short read is.
 *
 * Geo-referencing as the reference derives it: dx, dy from
 * ModelPixelScale (33550); x0 = tie point X, y0 = tie point Y + (1 - ny) dy
 * (33922) [ref geotiff16.c:205-214]; values are int16 elevations (z0 = -32767,
 * dz = 1, as [ref geotiff16.c:186-187, :230-233]); image rows run north->south
 * and are stored south->north in memory [ref geotiff16.c:246-255].
 */
#include "host.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>

enum { COMPRESSION_NONE = 1, COMPRESSION_LZW = 5, COMPRESSION_DEFLATE = 8, COMPRESSION_PACKBITS = 32773,
        COMPRESSION_DEFLATE_OLD = 32946 };

struct tiff_file {
        FILE * fid;
        int swap; /* file byte order differs from the host's */
        int little; /* the file's byte order is II */
        uint32_t width, height, rows_per_strip, n_strips;
        uint32_t bits, samples, compression, predictor, fill_order;
        uint32_t strip_offsets_at, strip_offsets_type, strip_offsets_count;
        uint32_t strip_offsets_value;
        uint32_t strip_counts_at, strip_counts_type, strip_counts_count;
        uint32_t strip_counts_value;
        /* a compressed file: where its strips are, checked against the file's size */
        uint32_t * offsets, * counts;
        double scale[3], tie[6];
        int have_scale, have_tie;
};

static uint16_t rd16(const unsigned char * b, int swap)
{
        uint16_t v;
        memcpy(&v, b, 2);
        return swap ? (uint16_t)((v >> 8) | (v << 8)) : v;
}

static uint32_t rd32(const unsigned char * b, int swap)
{
        uint32_t v;
        memcpy(&v, b, 4);
        if (swap) v = (v >> 24) | ((v >> 8) & 0xff00u) | ((v << 8) & 0xff0000u) | (v << 24);
        return v;
}

static double rd64f(const unsigned char * b, int swap)
{
        unsigned char t[8];
        int i;
        for (i = 0; i < 8; i++) t[i] = swap ? b[7 - i] : b[i];
        double v;
        memcpy(&v, t, 8);
        return v;
}

static int read_doubles(struct tiff_file * t, uint32_t offset, uint32_t count, double * out,
    uint32_t max)
{
        unsigned char buf[8];
        uint32_t i;
        if (count > max) count = max;
        if (fseek(t->fid, offset, SEEK_SET) != 0) return 1;
        for (i = 0; i < count; i++) {
                if (fread(buf, 1, 8, t->fid) != 8) return 1;
                out[i] = rd64f(buf, t->swap);
        }
        return 0;
}

/* One strip's entry of StripOffsets or StripByteCounts: inline in the directory (one LONG or
 * SHORT, two SHORTs), or in an array of SHORTs or LONGs elsewhere in the file */
struct strip_table {
        uint32_t at, type, count, value;
};

static int strip_entry(struct tiff_file * t, const struct strip_table * table, uint32_t strip, uint32_t * entry)
{
        if (table->count == 1) {
                *entry = table->value;
                return 0;
        }
        const uint32_t size = (table->type == 3) ? 2 : 4;
        if ((table->count == 2) && (size == 2)) { /* two SHORTs inline: the first in the field's first bytes */
                *entry = ((strip == 0) == t->little) ? (table->at & 0xffffu) : (table->at >> 16);
                return 0;
        }
        unsigned char b[4];
        if (fseek(t->fid, table->at + size * strip, SEEK_SET) != 0) return 1;
        if (fread(b, 1, size, t->fid) != size) return 1;
        *entry = (size == 2) ? rd16(b, t->swap) : rd32(b, t->swap);
        return 0;
}

/* ... and all of them (a table of thousands of entries: one read, not one per strip) */
static int strip_entries(struct tiff_file * t, const struct strip_table * table, uint32_t * entries)
{
        const uint32_t size = (table->type == 3) ? 2 : 4;
        uint32_t strip;
        if ((uint64_t)table->count * size <= 4) {
                for (strip = 0; strip < table->count; strip++)
                        if (strip_entry(t, table, strip, &entries[strip])) return 1;
                return 0;
        }
        /* (read in place, at the end of the array when they are SHORTs, and widened from the front) */
        unsigned char * raw = (unsigned char *)entries + (size_t)table->count * (4 - size);
        if (fseek(t->fid, table->at, SEEK_SET) != 0) return 1;
        if (fread(raw, size, table->count, t->fid) != table->count) return 1;
        for (strip = 0; strip < table->count; strip++)
                entries[strip] = (size == 2) ? rd16(raw + 2 * (size_t)strip, t->swap) :
                                               rd32(raw + 4 * (size_t)strip, t->swap);
        return 0;
}

static int strip_offset(struct tiff_file * t, uint32_t strip, uint32_t * offset)
{
        const struct strip_table table = { t->strip_offsets_at, t->strip_offsets_type, t->strip_offsets_count,
                t->strip_offsets_value };
        return strip_entry(t, &table, strip, offset);
}

static void tiff_close(struct tiff_file * t)
{
        if (t->fid != NULL) fclose(t->fid);
        free(t->offsets), free(t->counts);
        t->fid = NULL, t->offsets = t->counts = NULL;
}

/* The strips of a compressed file: every offset and byte count, each strip inside the file --
 * before anything is allocated for, or read from, a strip */
static int tiff_strips(struct tiff_file * t)
{
        if ((t->strip_counts_count != t->n_strips) || ((t->strip_counts_type != 3) && (t->strip_counts_type != 4)) ||
            ((t->strip_offsets_type != 3) && (t->strip_offsets_type != 4)))
                return 1;
        if (fseek(t->fid, 0, SEEK_END) != 0) return 1;
        const long end = ftell(t->fid);
        if (end < 0) return 1;
        const uint64_t file_size = (uint64_t)end;
        if ((uint64_t)t->n_strips * 4 > file_size) return 1; /* (the two tables are in the file too) */
        t->offsets = malloc((size_t)t->n_strips * sizeof(*t->offsets));
        t->counts = malloc((size_t)t->n_strips * sizeof(*t->counts));
        if ((t->offsets == NULL) || (t->counts == NULL)) return 1;
        const struct strip_table offsets = { t->strip_offsets_at, t->strip_offsets_type, t->strip_offsets_count,
                t->strip_offsets_value };
        const struct strip_table counts = { t->strip_counts_at, t->strip_counts_type, t->strip_counts_count,
                t->strip_counts_value };
        if (strip_entries(t, &offsets, t->offsets) || strip_entries(t, &counts, t->counts)) return 1;
        uint32_t strip;
        for (strip = 0; strip < t->n_strips; strip++)
                if ((uint64_t)t->offsets[strip] + t->counts[strip] > file_size) return 1;
        return 0;
}

/* Parse the header and the first image file directory */
static int tiff_open(const char * path, struct tiff_file * t)
{
        memset(t, 0, sizeof(*t));
        t->bits = 1, t->samples = 1, t->compression = COMPRESSION_NONE;
        t->predictor = 1, t->fill_order = 1;
        t->rows_per_strip = 0xffffffffu;
        t->fid = fopen(path, "rb");
        if (t->fid == NULL) return TURTLE_RETURN_PATH_ERROR;
        unsigned char h[8];
        if (fread(h, 1, 8, t->fid) != 8) goto bad;
        const uint16_t probe = 1;
        const int host_little = *(const unsigned char *)&probe;
        if ((h[0] == 'I') && (h[1] == 'I'))
                t->swap = !host_little, t->little = 1;
        else if ((h[0] == 'M') && (h[1] == 'M'))
                t->swap = host_little;
        else
                goto bad;
        if (rd16(h + 2, t->swap) != 42) goto bad; /* (43: BigTIFF) */
        const uint32_t ifd = rd32(h + 4, t->swap);
        if (fseek(t->fid, ifd, SEEK_SET) != 0) goto bad;
        unsigned char nb[2];
        if (fread(nb, 1, 2, t->fid) != 2) goto bad;
        const uint16_t n = rd16(nb, t->swap);
        uint16_t i;
        for (i = 0; i < n; i++) {
                unsigned char e[12];
                if (fseek(t->fid, ifd + 2 + 12u * i, SEEK_SET) != 0) goto bad;
                if (fread(e, 1, 12, t->fid) != 12) goto bad;
                const uint16_t tag = rd16(e, t->swap), type = rd16(e + 2, t->swap);
                const uint32_t count = rd32(e + 4, t->swap);
                /* SHORT values sit left-justified in the value field */
                const uint32_t value =
                    (type == 3) ? rd16(e + 8, t->swap) : rd32(e + 8, t->swap);
                switch (tag) {
                case 256: t->width = value; break;
                case 257: t->height = value; break;
                case 258: t->bits = value; break;
                case 259: t->compression = value; break;
                case 266: t->fill_order = value; break;
                case 277: t->samples = value; break;
                case 278: t->rows_per_strip = value; break;
                case 273:
                        t->strip_offsets_type = type;
                        t->strip_offsets_count = count;
                        t->strip_offsets_value = value;
                        t->strip_offsets_at = rd32(e + 8, t->swap);
                        break;
                case 279:
                        t->strip_counts_type = type;
                        t->strip_counts_count = count;
                        t->strip_counts_value = value;
                        t->strip_counts_at = rd32(e + 8, t->swap);
                        break;
                case 317: t->predictor = value; break;
                case 322: /* TileWidth: a tiled file */
                        goto bad;
                case 33550:
                        if ((type == 12) && (count >= 2)) {
                                if (read_doubles(t, rd32(e + 8, t->swap), count, t->scale, 3))
                                        goto bad;
                                t->have_scale = 1;
                        }
                        break;
                case 33922:
                        if ((type == 12) && (count >= 6)) {
                                if (read_doubles(t, rd32(e + 8, t->swap), count, t->tie, 6))
                                        goto bad;
                                t->have_tie = 1;
                        }
                        break;
                default: break;
                }
        }
        if ((t->width == 0) || (t->height == 0) || (t->bits != 16) || (t->samples != 1) ||
            (t->strip_offsets_count == 0) || (t->rows_per_strip == 0) || (t->fill_order == 2))
                goto bad;
        switch (t->compression) {
        case COMPRESSION_NONE:
        case COMPRESSION_PACKBITS:
                t->predictor = 1; /* (no predictor with these in libtiff: the tag is ignored) */
                break;
        case COMPRESSION_LZW:
        case COMPRESSION_DEFLATE:
        case COMPRESSION_DEFLATE_OLD:
                if ((t->predictor != 1) && (t->predictor != 2)) goto bad;
                break;
        default: goto bad;
        }
        if (t->rows_per_strip > t->height) t->rows_per_strip = t->height;
        t->n_strips = (t->height + t->rows_per_strip - 1) / t->rows_per_strip;
        if (t->n_strips != t->strip_offsets_count) goto bad;
        if ((t->compression != COMPRESSION_NONE) && tiff_strips(t)) goto bad;
        return TURTLE_RETURN_SUCCESS;
bad:
        tiff_close(t);
        return TURTLE_RETURN_BAD_FORMAT;
}

/* ---- strip decoders: (src, src_len) -> exactly dst_len bytes at dst, or 1.  None reads beyond
 * src_len or writes beyond dst_len; input left over once dst is full is ignored. ---- */

/* LZW as libtiff's decoder reads it (the TIFF 6.0 variant every writer of the last thirty years
 * emits): codes MSB first, 9 to 12 bits; 256 clears the table, 257 ends the data; the width grows
 * one code EARLY, when the next free entry is 511, 1023 or 2047.  The first code of a strip is a
 * Clear: the LSB-first streams of writers older than that, and raw samples under an LZW tag, end
 * there.  A code the table does not hold yet is an error but for the one the encoder may use
 * before the decoder has it (KwKwK: the previous string plus its own first byte). */
#define LZW_CLEAR 256
#define LZW_EOI 257
#define LZW_FIRST 258
#define LZW_SIZE 4096

struct lzw_entry {
        uint16_t prefix, length; /* the entry this one extends; bytes in its string */
        unsigned char first, last;
};

static int decode_lzw(const unsigned char * src, size_t src_len, unsigned char * dst, size_t dst_len)
{
        struct lzw_entry table[LZW_SIZE];
        uint32_t acc = 0;
        int avail = 0, nbits = 9, i;
        size_t at = 0, pos = 0;
        unsigned next = LZW_FIRST; /* the next free entry */
        int old = -1;              /* the previous code (-1: none since the Clear, or no Clear yet) */
        int cleared = 0;
        for (i = 0; i < 256; i++) {
                table[i].prefix = 0, table[i].length = 1;
                table[i].first = table[i].last = (unsigned char)i;
        }
        while (pos < dst_len) {
                while (avail < nbits) {
                        if (at >= src_len) return 1;
                        acc = (acc << 8) | src[at++];
                        avail += 8;
                }
                const unsigned code = (acc >> (avail - nbits)) & ((1u << nbits) - 1);
                avail -= nbits;
                if (code == LZW_EOI) return 1; /* (short: pos < dst_len) */
                if (code == LZW_CLEAR) {
                        next = LZW_FIRST, nbits = 9, old = -1, cleared = 1;
                        continue;
                }
                if (!cleared) return 1;
                if (old < 0) { /* the first code after a Clear is a byte */
                        if (code > 255) return 1;
                        dst[pos++] = (unsigned char)code;
                        old = (int)code;
                        continue;
                }
                if (code > next) return 1;
                if ((code == next) && (next >= LZW_SIZE)) return 1;
                if (next < LZW_SIZE) { /* (a full table stays as it is until the Clear) */
                        struct lzw_entry * e = &table[next];
                        e->prefix = (uint16_t)old;
                        e->length = (uint16_t)(table[old].length + 1);
                        e->first = table[old].first;
                        e->last = (code < next) ? table[code].first : table[old].first;
                        next++;
                        if ((next > (1u << nbits) - 2) && (nbits < 12)) nbits++;
                }
                const size_t length = table[code].length;
                if (length > dst_len - pos) return 1;
                unsigned char * tail = dst + pos + length;
                unsigned c = code;
                size_t k;
                for (k = 0; k < length; k++) {
                        *--tail = table[c].last;
                        c = table[c].prefix;
                }
                pos += length;
                old = (int)code;
        }
        return 0;
}

/* Deflate: one zlib stream per strip */
static int decode_deflate(const unsigned char * src, size_t src_len, unsigned char * dst, size_t dst_len)
{
        z_stream z;
        memset(&z, 0, sizeof(z));
        if ((src_len > 0xffffffffu) || (dst_len > 0xffffffffu) || (inflateInit(&z) != Z_OK)) return 1;
        z.next_in = (Bytef *)src, z.avail_in = (uInt)src_len;
        z.next_out = dst, z.avail_out = (uInt)dst_len;
        inflate(&z, Z_FINISH); /* (a stream that ends early, or is damaged, leaves room in dst) */
        const int full = (z.avail_out == 0);
        inflateEnd(&z);
        return !full;
}

/* PackBits: n in 0 .. 127 copies the n + 1 bytes that follow, n in -127 .. -1 repeats the next
 * byte 1 - n times, -128 does nothing */
static int decode_packbits(const unsigned char * src, size_t src_len, unsigned char * dst, size_t dst_len)
{
        size_t at = 0, pos = 0;
        while (pos < dst_len) {
                if (at >= src_len) return 1;
                const int n = (signed char)src[at++];
                if (n >= 0) {
                        const size_t length = (size_t)n + 1;
                        if ((length > src_len - at) || (length > dst_len - pos)) return 1;
                        memcpy(dst + pos, src + at, length);
                        at += length, pos += length;
                } else if (n != -128) {
                        const size_t length = (size_t)(1 - n);
                        if ((at >= src_len) || (length > dst_len - pos)) return 1;
                        memset(dst + pos, src[at++], length);
                        pos += length;
                }
        }
        return 0;
}

static int decode_strip(uint32_t compression, const unsigned char * src, size_t src_len, unsigned char * dst,
    size_t dst_len)
{
        switch (compression) {
        case COMPRESSION_LZW: return decode_lzw(src, src_len, dst, dst_len);
        case COMPRESSION_DEFLATE:
        case COMPRESSION_DEFLATE_OLD: return decode_deflate(src, src_len, dst, dst_len);
        case COMPRESSION_PACKBITS: return decode_packbits(src, src_len, dst, dst_len);
        default: return 1;
        }
}

int tamd_tiff_probe(const char * path, struct turtle_map * m)
{
        struct tiff_file t;
        const int rc = tiff_open(path, &t);
        if (rc != TURTLE_RETURN_SUCCESS) return rc;
        tiff_close(&t);
        m->nx = (int)t.width, m->ny = (int)t.height;
        m->x0 = m->y0 = 0., m->dx = m->dy = 0.;
        if (t.have_scale) m->dx = t.scale[0], m->dy = t.scale[1];
        if (t.have_tie) {
                m->x0 = t.tie[3];
                m->y0 = t.tie[4] + (1 - m->ny) * m->dy; /* [ref geotiff16.c:213] */
        }
        m->z0 = -32767., m->dz = 1.;
        m->is_signed = 1;
        m->projection.type = TAMD_PROJ_NONE;
        m->rows_together = (t.compression == COMPRESSION_NONE) ? 0 : (int)t.rows_per_strip;
        strcpy(m->encoding, "tif");
        return TURTLE_RETURN_SUCCESS;
}

/* A compressed file: every strip that holds image rows row0 .. row1 - 1 is read and decoded
 * whole, and the rows among these are copied out.  Byte order first, then the predictor's
 * running sum along the row, modulo 2^16 (libtiff's order: the differences were taken from
 * samples in the file's byte order read as numbers, not from bytes).  Rows stand alone for
 * both, so a row outside the range costs its share of the decoding and nothing more. */
static int read_rows_compressed(struct tiff_file * t, struct turtle_map * m, uint32_t row0, uint32_t row1)
{
        const size_t nx = t->width, row_bytes = nx * sizeof(uint16_t);
        const uint32_t first = row0 / t->rows_per_strip, last = (row1 - 1) / t->rows_per_strip;
        uint32_t strip, most = 0;
        for (strip = first; strip <= last; strip++)
                if (t->counts[strip] > most) most = t->counts[strip];
        unsigned char * src = malloc(most ? most : 1);
        /* (a strip of one row is decoded where it goes) */
        unsigned char * rows = (t->rows_per_strip > 1) ? malloc((size_t)t->rows_per_strip * row_bytes) : NULL;
        int rc = TURTLE_RETURN_SUCCESS;
        if ((src == NULL) || ((rows == NULL) && (t->rows_per_strip > 1))) rc = TURTLE_RETURN_MEMORY_ERROR;
        for (strip = first; (strip <= last) && (rc == TURTLE_RETURN_SUCCESS); strip++) {
                const uint32_t top = strip * t->rows_per_strip;
                const uint32_t n_rows = (t->height - top < t->rows_per_strip) ? t->height - top : t->rows_per_strip;
                unsigned char * to =
                    (rows != NULL) ? rows : (unsigned char *)(m->nodes + ((size_t)t->height - 1 - top) * nx);
                if ((fseek(t->fid, (long)t->offsets[strip], SEEK_SET) != 0) ||
                    (fread(src, 1, t->counts[strip], t->fid) != t->counts[strip]) ||
                    decode_strip(t->compression, src, t->counts[strip], to, n_rows * row_bytes)) {
                        rc = TURTLE_RETURN_BAD_FORMAT + 100;
                        break;
                }
                uint32_t row;
                for (row = (top > row0) ? top : row0; (row < top + n_rows) && (row < row1); row++) {
                        uint16_t * dst = m->nodes + ((size_t)t->height - 1 - row) * nx;
                        size_t i;
                        if (rows != NULL) memcpy(dst, rows + (size_t)(row - top) * row_bytes, row_bytes);
                        if (t->swap)
                                for (i = 0; i < nx; i++) dst[i] = (uint16_t)((dst[i] >> 8) | (dst[i] << 8));
                        if (t->predictor == 2)
                                for (i = 1; i < nx; i++) dst[i] = (uint16_t)(dst[i] + dst[i - 1]);
                }
        }
        free(src), free(rows);
        return rc;
}

/* grid rows iy0 .. iy1 - 1 (image row `row`, from the north, is grid row ny - 1 - row) */
int tamd_tiff_read_rows(const char * path, struct turtle_map * m, int iy0, int iy1)
{
        struct tiff_file t;
        int rc = tiff_open(path, &t);
        if (rc != TURTLE_RETURN_SUCCESS) return rc;
        if ((iy0 >= iy1) || (iy0 < 0) || (iy1 > (int)t.height) || ((int)t.width != m->nx) ||
            ((int)t.height != m->ny)) { /* no row, or a file that is no longer the one probed */
                tiff_close(&t);
                return (iy0 >= iy1) ? TURTLE_RETURN_SUCCESS : TURTLE_RETURN_BAD_FORMAT + 101;
        }
        if (t.compression != COMPRESSION_NONE) {
                rc = read_rows_compressed(&t, m, t.height - (uint32_t)iy1, t.height - (uint32_t)iy0);
                tiff_close(&t);
                return rc;
        }
        const size_t nx = t.width;
        uint32_t row, in_strip = 0xffffffffu;
        for (row = t.height - (uint32_t)iy1; (row < t.height - (uint32_t)iy0) && (rc == TURTLE_RETURN_SUCCESS);
             row++) {
                const uint32_t strip = row / t.rows_per_strip;
                if (strip != in_strip) {
                        uint32_t offset;
                        if (strip_offset(&t, strip, &offset) ||
                            (fseek(t.fid, (long)(offset + (size_t)(row % t.rows_per_strip) * nx * sizeof(uint16_t)),
                                 SEEK_SET) != 0)) {
                                rc = TURTLE_RETURN_BAD_FORMAT + 100;
                                break;
                        }
                        in_strip = strip;
                }
                uint16_t * dst = m->nodes + ((size_t)t.height - 1 - row) * nx;
                if (fread(dst, sizeof(*dst), nx, t.fid) != nx) {
                        rc = TURTLE_RETURN_BAD_FORMAT + 100;
                        break;
                }
                if (t.swap) {
                        size_t i;
                        for (i = 0; i < nx; i++)
                                dst[i] = (uint16_t)((dst[i] >> 8) | (dst[i] << 8));
                }
        }
        tiff_close(&t);
        return rc;
}

int tamd_tiff_read(const char * path, struct turtle_map * m)
{
        return tamd_tiff_read_rows(path, m, 0, m->ny);
}
