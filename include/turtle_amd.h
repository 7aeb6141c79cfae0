/*
 * turtle_amd.h -- C ABI of libturtle_amd.so, an MI355X-native implementation
 * of TURTLE's optimistic ray/terrain stepper path.
 *
 * Two groups of entry points:
 *
 *  (1) DROP-IN: the reference's own public functions for this path, with the
 *      same names, argument meaning, ownership and error convention, so that a
 *      caller written against the reference's `turtle.h` links unchanged
 *      (`#include "turtle.h"` from this directory forwards here).  Each
 *      declaration cites the reference declaration it replaces as
 *      [ref include/turtle.h:LINE] and the implementation it restates as
 *      [impl src/turtle/FILE.c:LINE] (paths under the reference tree).
 *      These are scalar calls: each one runs the same device kernels as the
 *      batch form with n = 1 and therefore costs one kernel launch -- unless
 *      the caller asks for them to be answered on the host
 *      (turtle_amd_scalar_set: a restatement of the reference's one-point
 *      functions for callers that keep its per-ray loop; off by default).
 *      Without a usable gfx950 device every computing entry point fails with
 *      TURTLE_RETURN_LIBRARY_ERROR through the error handler, whatever that
 *      option says: nothing in this library stands in for a missing GPU.
 *
 *  (2) BATCH EXTENSION (suffix _n, prefix turtle_amd_): the same operations on
 *      n independent rays/points per call, which is what a GPU is for.  The
 *      reference has no such entry points; INTEGRATION.md shows the few lines
 *      a maintainer adds to bind them.  Arrays are plain C arrays, one element
 *      (or one double[3] / double[2] / int[2] group) per ray, in HOST or DEVICE
 *      memory according to `space`.
 *
 * Units and conventions are the reference's: degrees, metres, WGS84 ECEF.
 */
#ifndef TURTLE_AMD_H
#define TURTLE_AMD_H

#ifdef __cplusplus
extern "C" {
#endif

#ifndef TURTLE_API
#define TURTLE_API
#endif

/* ---- return codes and handles [ref include/turtle.h:35-62, :64-106] ---- */
enum turtle_return {
        TURTLE_RETURN_SUCCESS = 0,
        TURTLE_RETURN_BAD_ADDRESS,
        TURTLE_RETURN_BAD_EXTENSION,
        TURTLE_RETURN_BAD_FORMAT,
        TURTLE_RETURN_BAD_PROJECTION,
        TURTLE_RETURN_BAD_JSON,
        TURTLE_RETURN_DOMAIN_ERROR,
        TURTLE_RETURN_LIBRARY_ERROR,
        TURTLE_RETURN_LOCK_ERROR,
        TURTLE_RETURN_MEMORY_ERROR,
        TURTLE_RETURN_PATH_ERROR,
        TURTLE_RETURN_UNLOCK_ERROR,
        N_TURTLE_RETURNS
};

struct turtle_projection;
struct turtle_map;
struct turtle_stack;
struct turtle_client;
struct turtle_stepper;

/* [ref include/turtle.h:93-106] */
struct turtle_map_info {
        int nx, ny;           /* nodes along x and y */
        double x[2];          /* x range (longitude for geodetic maps) */
        double y[2];          /* y range (latitude) */
        double z[2];          /* elevation range spanned by the 16-bit code */
        const char * encoding;
};

/* ---- error handling [ref include/turtle.h:114-194; impl error.c:28-198] ----
 * Every enum-returning function returns TURTLE_RETURN_SUCCESS or a code and,
 * unless the handler is NULL, calls the handler once with a message shaped
 * "{ <function> [#<code>], <file>:<line> } <text>".  The default handler prints
 * the message to stderr and exit(EXIT_FAILURE)s, as the reference's does. */
typedef void turtle_function_t(void);
typedef void turtle_error_handler_t(enum turtle_return code,
    turtle_function_t * function, const char * message);
typedef int turtle_stack_locker_t(void); /* [ref include/turtle.h:149] */

TURTLE_API const char * turtle_error_function(turtle_function_t * function);
TURTLE_API turtle_error_handler_t * turtle_error_handler_get(void);
TURTLE_API void turtle_error_handler_set(turtle_error_handler_t * handler);

/* ---- ECEF transforms [ref include/turtle.h:556-602; impl ecef.c:41-207] ---- */
TURTLE_API void turtle_ecef_from_geodetic(
    double latitude, double longitude, double elevation, double ecef[3]);
TURTLE_API void turtle_ecef_to_geodetic(const double ecef[3], double * latitude,
    double * longitude, double * altitude);
TURTLE_API void turtle_ecef_from_horizontal(double latitude, double longitude,
    double azimuth, double elevation, double direction[3]);
TURTLE_API void turtle_ecef_to_horizontal(double latitude, double longitude,
    const double direction[3], double * azimuth, double * elevation);

/* ---- projections [ref include/turtle.h:235-333; impl projection.c:53-468] ----
 * Names as in the reference: "Lambert I|II|IIe|III|IV|93", "UTM <zone>N|S",
 * "UTM <central meridian>.<fraction>N|S". */
TURTLE_API enum turtle_return turtle_projection_create(
    struct turtle_projection ** projection, const char * name);
TURTLE_API void turtle_projection_destroy(
    struct turtle_projection ** projection);
TURTLE_API enum turtle_return turtle_projection_configure(
    struct turtle_projection * projection, const char * name);
TURTLE_API const char * turtle_projection_name(
    const struct turtle_projection * projection);
TURTLE_API enum turtle_return turtle_projection_project(
    const struct turtle_projection * projection, double latitude,
    double longitude, double * x, double * y);
TURTLE_API enum turtle_return turtle_projection_unproject(
    const struct turtle_projection * projection, double x, double y,
    double * latitude, double * longitude);

/* ---- maps [ref include/turtle.h:362-543; impl map.c:54-421] ----
 * `projection` is NULL for a geodetic grid (x = longitude, y = latitude) or a
 * projection name; under a stepper a projected map is looked up at the
 * projected coordinates [impl stepper.c:65-83, :243-248].
 * turtle_map_load reads .hgt tiles [impl io/hgt.c:45-151] and GeoTIFF-16
 * .tif files [impl io/geotiff16.c:165-258] with a native reader (no libtiff):
 * classic TIFF in strips, either byte order, one 16-bit sample a pixel,
 * Compression 1 (none), 5 (LZW), 8 or 32946 (Deflate) or 32773 (PackBits),
 * with LZW and Deflate also Predictor 2 (horizontal differencing) -- which is
 * how ASTER GDEM, SRTM and GDAL exports ship; and the reference's own .png map format (16-bit
 * greyscale + JSON "topography" header, incl. its projection) [impl
 * io/png16.c:183-448] with a native reader (zlib's inflate only), and the
 * text formats .grd / .asc [impl io/grd.c, io/asc.c]; other
 * extensions return TURTLE_RETURN_BAD_EXTENSION.  TURTLE_RETURN_BAD_FORMAT:
 * tiled TIFFs, BigTIFF, any other compression (JPEG, CCITT, LZMA, ZSTD ...)
 * or predictor, FillOrder 2, a compressed file without StripByteCounts or with
 * a strip beyond the end of the file, a strip that does not decode to exactly
 * its rows ("missing data"); non-16-bit or interlaced PNGs. */
TURTLE_API enum turtle_return turtle_map_create(struct turtle_map ** map,
    const struct turtle_map_info * info, const char * projection);
TURTLE_API void turtle_map_destroy(struct turtle_map ** map);
TURTLE_API enum turtle_return turtle_map_load(
    struct turtle_map ** map, const char * path);
/* [ref include/turtle.h:401-424; impl map.c:165-180] Writes the map as .png
 * (the reference's map format, projection included) or as .tif (GeoTIFF-16:
 * maps with z scale [-32767, 32768] and no projection), without libpng /
 * libtiff; .hgt / .grd / .asc return TURTLE_RETURN_BAD_FORMAT, anything else
 * TURTLE_RETURN_BAD_EXTENSION, as in the reference. */
TURTLE_API enum turtle_return turtle_map_dump(
    const struct turtle_map * map, const char * path);
TURTLE_API enum turtle_return turtle_map_fill(
    struct turtle_map * map, int ix, int iy, double elevation);
TURTLE_API enum turtle_return turtle_map_node(const struct turtle_map * map,
    int ix, int iy, double * x, double * y, double * elevation);
TURTLE_API enum turtle_return turtle_map_elevation(
    const struct turtle_map * map, double x, double y, double * elevation,
    int * inside);
/* [ref include/turtle.h:515-517; impl map.c:280-392].  gx, gy are in-out: the
 * reference leaves them untouched outside the map and, by a slip at
 * map.c:352-353 that is reproduced, stores the y-gradient in gx and leaves gy
 * untouched for a point in the grid's first half-row. */
TURTLE_API enum turtle_return turtle_map_gradient(
    const struct turtle_map * map, double x, double y, double * gx, double * gy,
    int * inside);
TURTLE_API const struct turtle_projection * turtle_map_projection(
    const struct turtle_map * map);
TURTLE_API void turtle_map_meta(const struct turtle_map * map,
    struct turtle_map_info * info, const char ** projection);

/* ---- tile stacks [ref include/turtle.h:637-719; impl stack.c:46-450] ----
 * As in the reference a stack keeps at most `stack_size` tiles in memory (no
 * limit if <= 0), loads a tile when a query first needs it and drops the least
 * recently used one to make room [ref stack.c:150, :399-450].  Here "memory" is
 * HBM and a query is a batch: the kernels list the rays / points that met a
 * tile that is not resident, the host pages those tiles in and the list runs
 * again, until it is empty -- results are those of a stack with every tile
 * loaded.  The effective limit is never below 16: a lookup decides a seam
 * against the boxes of the neighbouring tiles, and the bisection of a ray's
 * crossing can need two 3 x 3 neighbourhoods, side by side, at once.
 * turtle_stack_load brings tiles in up to the limit (all of them without
 * one): after it a batch over the loaded area runs in a single round.  Lookup
 * semantics: half-open tile boxes, exclusive outer upper edge, missing tile =>
 * inside = 0. */
TURTLE_API enum turtle_return turtle_stack_create(struct turtle_stack ** stack,
    const char * path, int stack_size, turtle_stack_locker_t * lock,
    turtle_stack_locker_t * unlock);
TURTLE_API void turtle_stack_destroy(struct turtle_stack ** stack);
TURTLE_API enum turtle_return turtle_stack_clear(struct turtle_stack * stack);
TURTLE_API enum turtle_return turtle_stack_load(struct turtle_stack * stack);
/* extension: the number of tiles in memory right now [ref stack.h: tiles.size] */
TURTLE_API int turtle_amd_stack_resident(const struct turtle_stack * stack);
TURTLE_API enum turtle_return turtle_stack_elevation(
    struct turtle_stack * stack, double latitude, double longitude,
    double * elevation, int * inside);

/* [ref include/turtle.h:748-750; impl stack.c:364-388] */
TURTLE_API enum turtle_return turtle_stack_gradient(
    struct turtle_stack * stack, double latitude, double longitude,
    double * glat, double * glon, int * inside);

/* ---- clients [ref include/turtle.h:773-842; impl client.c:41-188] ----
 * Same answers as the stack; the reference's per-thread tile pinning has no
 * device analogue and is not reproduced. */
TURTLE_API enum turtle_return turtle_client_create(
    struct turtle_client ** client, struct turtle_stack * stack);
TURTLE_API enum turtle_return turtle_client_destroy(
    struct turtle_client ** client);
TURTLE_API enum turtle_return turtle_client_clear(
    struct turtle_client * client);
TURTLE_API enum turtle_return turtle_client_elevation(
    struct turtle_client * client, double latitude, double longitude,
    double * elevation, int * inside);

/* ---- stepper [ref include/turtle.h:859-1155; impl stepper.c:379-931] ---- */
TURTLE_API enum turtle_return turtle_stepper_create(
    struct turtle_stepper ** stepper);
TURTLE_API enum turtle_return turtle_stepper_destroy(
    struct turtle_stepper ** stepper);
TURTLE_API void turtle_stepper_geoid_set(
    struct turtle_stepper * stepper, struct turtle_map * geoid);
TURTLE_API struct turtle_map * turtle_stepper_geoid_get(
    const struct turtle_stepper * stepper);
TURTLE_API void turtle_stepper_reset(struct turtle_stepper * stepper);
/* The local-linear-approximation range [impl stepper.c:85-171] is stored and
 * returned for compatibility; the device always uses the exact transform,
 * i.e. behaves as the reference does at range 0 (difference at the default
 * range 1: 1.5e-9 relative on path length). */
TURTLE_API void turtle_stepper_range_set(
    struct turtle_stepper * stepper, double range);
TURTLE_API double turtle_stepper_range_get(
    const struct turtle_stepper * stepper);
TURTLE_API double turtle_stepper_slope_get(
    const struct turtle_stepper * stepper);
TURTLE_API void turtle_stepper_slope_set(
    struct turtle_stepper * stepper, double slope);
TURTLE_API double turtle_stepper_resolution_get(
    const struct turtle_stepper * stepper);
TURTLE_API void turtle_stepper_resolution_set(
    struct turtle_stepper * stepper, double resolution);
TURTLE_API enum turtle_return turtle_stepper_add_layer(
    struct turtle_stepper * stepper);
TURTLE_API enum turtle_return turtle_stepper_add_stack(
    struct turtle_stepper * stepper, struct turtle_stack * stack,
    double offset);
TURTLE_API enum turtle_return turtle_stepper_add_map(
    struct turtle_stepper * stepper, struct turtle_map * map, double offset);
TURTLE_API enum turtle_return turtle_stepper_add_flat(
    struct turtle_stepper * stepper, double ground_level);
/* [ref include/turtle.h:1126-1129; impl stepper.c:780-875] */
TURTLE_API enum turtle_return turtle_stepper_step(
    struct turtle_stepper * stepper, double * position,
    const double * direction, double * latitude, double * longitude,
    double * altitude, double * elevation, double * step, int * index);
/* [ref include/turtle.h:1153-1155; impl stepper.c:877-931] */
TURTLE_API enum turtle_return turtle_stepper_position(
    struct turtle_stepper * stepper, double latitude, double longitude,
    double height, int layer_index, double * position, int * data_index);

/* ======================================================================== */
/*                    BATCH EXTENSION (not in the reference)                */
/* ======================================================================== */

/* Where the arrays of a batch call live. */
enum turtle_amd_space {
        TURTLE_AMD_HOST = 0,  /* host pointers: copied in/out, call is synchronous */
        TURTLE_AMD_DEVICE = 1 /* device pointers on the selected GPU: the call
                                 only enqueues work on the library stream */
};

/* Device / stream management, per calling THREAD: the device a thread's calls
 * run on ($LOCAL_RANK if set, else 0, until it calls turtle_amd_device_set), its
 * stream, its arithmetic mode and the scratch memory its calls use are its own.
 * The reference's threading rule carries over [ref include/turtle.h:129-132,
 * :620-626, examples/example-pthread.c]: a stepper (and its client) belongs to
 * one thread at a time; maps and stacks may be shared -- a stack whose tiles can
 * change (stack_size below its number of files) with lock / unlock callbacks, as
 * in the reference.  One process may drive one GPU (one process per GPU: what
 * bench.py does) or several, a thread each: maps and tiles get a copy on every
 * device that uses them.  A worker thread calls turtle_amd_thread_release before
 * it ends (its stream and scratch memory are freed then, never behind its back). */
TURTLE_API int turtle_amd_device_count(void);
TURTLE_API enum turtle_return turtle_amd_device_set(int device);
TURTLE_API int turtle_amd_device_get(void);
TURTLE_API void turtle_amd_thread_release(void);
/* Use a caller-owned hipStream_t (e.g. torch's current stream) for every
 * subsequent launch of the calling thread; NULL restores the library's own stream.
 * A batch call on device arrays returns when its kernels are queued.  One thread may
 * keep several batches IN FLIGHT: a stepper and a stream per batch (turtle_amd_stream_set
 * before each call; the steppers may share their maps and stacks).  A trace ends with
 * a few rays of thousands of steps in an all but empty GPU, which another stream's
 * batch fills: C2 batches take 2.6 ms each with two in flight, 2.2-2.3 with three, 3.6 ms
 * one at a time, the same bits (bench.py `in_flight`; tests/test_gpu_properties.py). */
TURTLE_API enum turtle_return turtle_amd_stream_set(void * hip_stream);
/* A second stepper over the same geometry -- the layers and their data in the order
 * they were added, the geoid, range, slope and resolution -- for a batch more in flight.
 * It borrows the same maps and stacks; destroy it with turtle_stepper_destroy. */
TURTLE_API enum turtle_return turtle_amd_stepper_clone(
    const struct turtle_stepper * stepper, struct turtle_stepper ** clone);
/* A hint, per thread: how many batches the caller keeps in flight (default 1).  With two or
 * more a trace kernel takes a smaller share of every compute unit, which leaves room for a
 * wave of another batch's kernel beside its own: better for the batches together, worse for
 * one alone.  Results do not depend on it. */
TURTLE_API void turtle_amd_in_flight_set(int batches);
TURTLE_API int turtle_amd_in_flight_get(void);
TURTLE_API enum turtle_return turtle_amd_synchronize(void);
/* Number of compute units of the selected device (0 if none). */
TURTLE_API int turtle_amd_compute_units(void);

/* Arithmetic of the trace kernel (turtle_stepper_trace_n) and of
 * turtle_ecef_to_geodetic(_n), which exposes the same transform for checking.
 *   STRICT  the reference's expressions in the reference's operand order, no
 *           FMA contraction, OCML asin/acos/atan2: differs from the x86
 *           reference only by the last ulp of those three functions.
 *   FAST    (default) the same algorithm with shared reciprocals, rsqrt-based
 *           roots, one polynomial arctangent and FMAs: ~3x fewer instructions
 *           per sample; coordinates differ from STRICT by a few ulp (<= 3e-9 m
 *           in altitude).  In turtle_stepper_trace_n a long ray samples a cubic
 *           Taylor line of the transform along its path (truncation <= 1e-9 m
 *           near a boundary), advances its position with one fused operation a
 *           step, and every crossing of the batch is located afterwards, in a
 *           kernel of its own, inside the reference's bracket by false position
 *           rather than by halving (the end point agrees to 1e-8 m).
 *           WHAT IS GUARANTEED (and tested, with no allowance, against the
 *           reference's golden vectors and the CPU restatement at full size):
 *           the same medium index; the path length within 1e-6 relative
 *           (measured: <= 5e-8 on every test, 1.6e-8 on C2's million rays); the
 *           step count equal, or off by one on a ray that grazes a surface
 *           within 1e-9 m (measured: 4 rays of C2's million).  The one ray kind
 *           outside the length bar is a ray that reaches no boundary before
 *           max_steps: its "length" is a sum of clearance-sized steps, not a
 *           distance (tests/test_gpu_parity.py names the one the suite has).
 * Both are checked against the reference's golden vectors at the 1e-6 bar.
 * Every other kernel (elevation, position, step, the other ecef transforms)
 * is always STRICT. */
/* WHERE the scalar (one point a call) drop-in functions compute.  DEVICE (default):
 * in the kernels, with n = 1 -- every call a launch and two copies, 20-35 us.  HOST:
 * turtle_ecef_*, turtle_map_elevation, turtle_stack_elevation, turtle_client_elevation,
 * turtle_stepper_step and turtle_stepper_position are answered by a host restatement of
 * the same reference functions (turtle_amd/csrc/scalar.c; the reference's arithmetic
 * with the exact transform, its `last`-sample cache, its tile list) on the host copies
 * of the maps and tiles -- ~0.1 us a call, for callers that keep the reference's per-ray
 * loop.  The batch calls (`_n`) run on the GPU whatever this says; a geometry with a
 * projected map stays with the kernels; and a usable device is required either way:
 * this is an option of a GPU library, not a fallback for machines without one.
 * Process-wide; set it before the stepping starts.  Without a call, the environment decides
 * at the first scalar call: TURTLE_AMD_SCALAR=host (a caller relinked against this library,
 * its source unchanged: examples/reference_loop.c); a call wins over the variable.  A stack
 * that threads share has lock / unlock callbacks, as in the reference; a host lookup in it
 * holds its tile against the other threads' loads while it reads it. */
enum turtle_amd_scalar { TURTLE_AMD_SCALAR_DEVICE = 0, TURTLE_AMD_SCALAR_HOST = 1 };
TURTLE_API void turtle_amd_scalar_set(int mode);
TURTLE_API int turtle_amd_scalar_get(void);

enum turtle_amd_math { TURTLE_AMD_MATH_FAST = 0, TURTLE_AMD_MATH_STRICT = 1 };
TURTLE_API void turtle_amd_math_set(int mode);
TURTLE_API int turtle_amd_math_get(void);

/* n independent ECEF transforms; same arithmetic as the scalar forms. */
TURTLE_API enum turtle_return turtle_ecef_from_geodetic_n(long n,
    const double * latitude, const double * longitude,
    const double * elevation, double * ecef /* [n][3] */, int space);
TURTLE_API enum turtle_return turtle_ecef_to_geodetic_n(long n,
    const double * ecef /* [n][3] */, double * latitude, double * longitude,
    double * altitude, int space);
TURTLE_API enum turtle_return turtle_ecef_from_horizontal_n(long n,
    const double * latitude, const double * longitude, const double * azimuth,
    const double * elevation, double * direction /* [n][3] */, int space);
TURTLE_API enum turtle_return turtle_ecef_to_horizontal_n(long n,
    const double * latitude, const double * longitude,
    const double * direction /* [n][3] */, double * azimuth,
    double * elevation, int space);

/* n projections / inverse projections */
TURTLE_API enum turtle_return turtle_projection_project_n(
    const struct turtle_projection * projection, long n,
    const double * latitude, const double * longitude, double * x, double * y,
    int space);
TURTLE_API enum turtle_return turtle_projection_unproject_n(
    const struct turtle_projection * projection, long n, const double * x,
    const double * y, double * latitude, double * longitude, int space);

/* n bilinear lookups.  `inside` is mandatory (a point outside the data is
 * reported there, never raised). */
TURTLE_API enum turtle_return turtle_map_elevation_n(
    const struct turtle_map * map, long n, const double * x, const double * y,
    double * elevation, int * inside, int space);
TURTLE_API enum turtle_return turtle_stack_elevation_n(
    struct turtle_stack * stack, long n, const double * latitude,
    const double * longitude, double * elevation, int * inside, int space);

/* Flags of turtle_map_resample. */
enum turtle_amd_resample_flags {
        /* an elevation outside the map's span is stored as the nearest end of the span
         * instead of failing the call */
        TURTLE_AMD_RESAMPLE_CLAMP = 1
};

/* Fills every node of `map` from `stack` or from another map `source` (exactly one of them):
 * the loop of the reference's examples/example-projection.c as one call.  For every node
 * (ix, iy) of the map it does exactly this:
 *
 *     x = x0 + ix*dx;  y = y0 + iy*dy;                       (turtle_map_node)
 *     if map is projected: turtle_projection_unproject(proj(map), x, y, &lat, &lon);
 *     else                 lat = y, lon = x;
 *     if stack:  turtle_stack_elevation(stack, lat, lon, &z, &inside);
 *     else: (u, v) = source has the SAME projection as map (same type and parameters,
 *                    or both geographic) ? (x, y)
 *                  : source projected ? turtle_projection_project(proj(source), lat, lon)
 *                  : (lon, lat);
 *           turtle_map_elevation(source, u, v, &z, &inside);
 *     if (inside) turtle_map_fill(map, ix, iy, z);           (else the node keeps its value)
 *
 * One departure from the example: it fills the nodes that fall outside the data too (with
 * the 0 its turtle_stack_elevation returns there); this call leaves them as they are and
 * counts them in *outside.  Each node gets the 16-bit code turtle_map_fill stores for z.
 * A z outside [z0, z0 + 65535 dz] (or z != z0 when dz <= 0; HGT voids among them) fails
 * the call with DOMAIN_ERROR and turtle_map_fill's message, and then NO node changes, on
 * the host or in any HBM copy; with TURTLE_AMD_RESAMPLE_CLAMP it is stored as the nearest
 * end of the span and counted in *clamped.  Lookups are always the strict bilinear ones:
 * the result does not depend on turtle_amd_math_set.  BAD_ADDRESS: map == NULL, or neither
 * source; DOMAIN_ERROR: both sources, source == map, a map that is a tile of a stack, or
 * unknown flags -- all of them change nothing.  Afterwards every reader sees the new
 * nodes: turtle_map_node / _dump and the host path, the kernels, and steppers that hold
 * the map already.  A paged stack is read in rounds, as the other batch calls do.
 * outside, clamped: may be NULL.  A map in use by another thread is the caller's race, as
 * with turtle_map_fill. */
TURTLE_API enum turtle_return turtle_map_resample(struct turtle_map * map,
    struct turtle_stack * stack /* or NULL */, const struct turtle_map * source /* or NULL */,
    int flags, long * outside /* or NULL */, long * clamped /* or NULL */);

/* Flags of turtle_map_fill_n. */
enum turtle_amd_fill_flags {
        /* an elevation outside the map's span is stored as the nearest end of the span
         * instead of failing the call (TURTLE_AMD_RESAMPLE_CLAMP's rule) */
        TURTLE_AMD_FILL_CLAMP = 1
};

/* Writes the window of nx x ny nodes whose south-west corner is node (ix0, iy0) from rows of
 * doubles: a numpy array, or a tensor already on the GPU, becomes a map without a file or a
 * call per node.  It is exactly this loop, done all or nothing:
 *
 *     for (j = 0; j < ny; j++) for (i = 0; i < nx; i++)
 *             turtle_map_fill(map, ix0 + i, iy0 + j, elevation[j * ld + i]);
 *
 * Row j of the array is map row iy0 + j, SOUTH TO NORTH, as turtle_map_node counts iy (an
 * image that has north first is flipped by its owner); ld >= nx is the distance between two
 * rows, in doubles, so a window of a wider array is passed as it lies.  Every stored code is
 * the one turtle_map_fill stores, signed (hgt) maps included.  The departures from the loop:
 * 1. if any element fails turtle_map_fill's checks the call fails with DOMAIN_ERROR and that
 * function's message ("inconsistent elevation value", "elevation is outside of map span"),
 * NO node changes, on the host or in any HBM copy, and *clamped is left alone; 2. a NaN,
 * which the scalar call lets through to an undefined cast, always fails, with "elevation is
 * outside of map span"; 3. with TURTLE_AMD_FILL_CLAMP an off-span value is stored as the
 * nearest end of the span (z0 when dz <= 0) and counted in *clamped; a NaN still fails.
 * BAD_ADDRESS: map or elevation is NULL; DOMAIN_ERROR: unknown flags, an unknown space, a map
 * that is a tile of a stack, a window that is not inside the map ("point is outside of map"),
 * ld < nx -- all raised before the device is touched, and changing nothing.  nx <= 0 or
 * ny <= 0 does nothing and succeeds.  Afterwards every reader sees the new nodes:
 * turtle_map_node / _dump and the host path, the kernels, and steppers that hold the map
 * already; copies on other devices go stale.  Both spaces run the same kernels (HOST rows go
 * through HBM: the (ny - 1) * ld + nx doubles they span), and the call has completed when it
 * returns, in either space.  The work follows the window, not the map: a patch of a large
 * map that is on the device moves the patch.  A map in use by another thread is the caller's
 * race, as with turtle_map_fill.  clamped: may be NULL. */
TURTLE_API enum turtle_return turtle_map_fill_n(struct turtle_map * map, int ix0, int iy0,
    int nx, int ny, const double * elevation /* [ny][ld] */, long ld, int flags,
    long * clamped /* or NULL */, int space);

/* Reads the same window: elevation[j * ld + i] is the value that
 *
 *     turtle_map_node(map, ix0 + i, iy0 + j, NULL, NULL, &z)
 *
 * returns, bit for bit, signed maps included; row j of the array is map row iy0 + j, south
 * to north.  The departures: the elements between the rows (ld > nx) are not touched; the
 * node coordinates are not returned (they are x0 + ix * dx, y0 + iy * dy of turtle_map_meta);
 * the values come from the map's HBM copy, through a kernel, in either space, and in DEVICE
 * space the call is asynchronous as the other batch calls are.  Errors as for
 * turtle_map_fill_n, without the flags; a tile of a stack can be read. */
TURTLE_API enum turtle_return turtle_map_node_n(const struct turtle_map * map, int ix0, int iy0,
    int nx, int ny, double * elevation /* [ny][ld] */, long ld, int space);

/* n gradients (the surface normal a Monte-Carlo needs at a hit point).  The
 * output arrays are in-out, as in the scalar calls. */
TURTLE_API enum turtle_return turtle_map_gradient_n(
    const struct turtle_map * map, long n, const double * x, const double * y,
    double * gx, double * gy, int * inside, int space);
TURTLE_API enum turtle_return turtle_stack_gradient_n(
    struct turtle_stack * stack, long n, const double * latitude,
    const double * longitude, double * glat, double * glon, int * inside,
    int space);

/* n calls of turtle_stepper_position; `position` rows of rays with no data
 * are left untouched and their data_index is -1 (data_index is mandatory). */
TURTLE_API enum turtle_return turtle_stepper_position_n(
    struct turtle_stepper * stepper, long n, const double * latitude,
    const double * longitude, const double * height, int layer_index,
    double * position /* [n][3] */, int * data_index, int space);

/* n unit normals of layer surfaces: what a Monte-Carlo needs where a ray crosses the topography
 * (flux through it, exit angle, reflection, refraction).  The normal is that of the TOP surface of
 * layer[r] above or below position[r], whatever the point's own altitude.  For each point r,
 * exactly this, with the reference's functions:
 *
 *     turtle_ecef_to_geodetic(position[r], &lat, &lon, &alt);         (alt is not used)
 *     if (layer[r] < 0 || layer[r] >= layers) { data_index[r] = -1; continue; }
 *     for (the layer's data, LAST ADDED FIRST, k = 0, 1, ...) {       [as turtle_stepper_position]
 *             glat = glon = gx = gy = 0;
 *             flat:           z = 0; inside = 1;
 *             stack:          turtle_stack_elevation(stack, lat, lon, &z, &inside);
 *                             turtle_stack_gradient(stack, lat, lon, &glat, &glon, &inside);
 *             geodetic map:   turtle_map_elevation(map, lon, lat, &z, &inside);
 *                             turtle_map_gradient(map, lon, lat, &glon, &glat, &inside);
 *             projected map:  P(la, lo) = turtle_projection_project(proj(map), la, lo) -> (x, y);
 *                             (x, y) = P(lat, lon);
 *                             turtle_map_elevation(map, x, y, &z, &inside);
 *                             turtle_map_gradient(map, x, y, &gx, &gy, &inside);
 *                             d = 1e-3;  (xp, yp) = P(lat + d, lon);  (xm, ym) = P(lat - d, lon);
 *                             glat = gx * (xp - xm) / (2. * d) + gy * (yp - ym) / (2. * d);
 *                             (xp, yp) = P(lat, lon + d);  (xm, ym) = P(lat, lon - d);
 *                             glon = gx * (xp - xm) / (2. * d) + gy * (yp - ym) / (2. * d);
 *             if (inside) { data_index[r] = k; hs = z + offset; break; }
 *     }
 *     if (none was inside) { data_index[r] = -1; continue; }           (reported, never raised)
 *     if (geoid) {                                                    [as turtle_stepper_position]
 *             lo = (lon >= 0) ? lon : lon + 360.;
 *             turtle_map_elevation(geoid, lo, lat, &u, &in);  if (in) hs += u;
 *             ugx = ugy = 0;  turtle_map_gradient(geoid, lo, lat, &ugx, &ugy, &in);
 *             if (in) { glon += ugx; glat += ugy; }
 *     }
 *     (E, N, U) = east, north, up at (lat, lon)     [the frame of turtle_ecef_from_horizontal]
 *     s = sin(lat);  c = cos(lat);  g = 1. - e * e * s * s;            [a, e: the WGS84 constants]
 *     Rn = a / sqrt(g);  Rm = Rn * (1. - e * e) / g;
 *     A = (Rn + hs) * c * M_PI / 180.;  B = (Rm + hs) * M_PI / 180.;  (metres per degree)
 *     w = U - (glon / A) * E - (glat / B) * N;   normal[r] = w / sqrt(w0*w0 + w1*w1 + w2*w2);
 *
 * The surface (lat, lon) -> from_geodetic(lat, lon, hs(lat, lon)) has the tangents A E + glon U
 * and B N + glat U: w is their cross product over A B.  The normal has unit length and points to
 * the side of increasing altitude.  At a pole (position x == 0 && y == 0, the special case of
 * turtle_ecef_to_geodetic) the east term is dropped.  Rows of `normal` whose data_index is -1
 * are left untouched.  The gradients are the reference's as it returns them, its slip in a
 * grid's first half-row included (see turtle_map_gradient_n).
 *
 * With turtle_stepper_crossings_n: the surface a crossing media[c][r] = {a, b} lies on is the top
 * of layer min(a, b) -- the ray was on one side of that layer's top and is now on the other
 * [ref stepper.c:690-700], whichever way it went and however many media it jumped.  For a ray
 * that left the data, {m, -1}, min is -1: no layer, data_index -1.  An empty slot {0, 0} reads
 * as layer 0: mask the slots by n_crossings.
 *
 * The arithmetic is always the strict one: the result does not depend on turtle_amd_math_set.
 * Over stacks with tiles to page in the call runs in rounds, as turtle_stepper_position_n does
 * (turtle_amd_stepper_rounds), with the results of a fully resident stack.  BAD_ADDRESS: any
 * pointer NULL; n <= 0 does nothing. */
TURTLE_API enum turtle_return turtle_stepper_normal_n(
    struct turtle_stepper * stepper, long n, const double * position /* [n][3] */,
    const int * layer /* [n] */, double * normal /* [n][3], in / out */,
    int * data_index /* [n], mandatory */, int space);

/* The skyline around n observers: for each of n_azimuths directions, how high the top of a layer
 * stands against the sky, the maximum over n_distances samples of the line -- what decides the
 * open-sky acceptance of a muography telescope, or whether an antenna on the ground sees a shower.
 * Item i = r * n_azimuths + a is line a of observer r; the outputs are observer-major, an
 * observer's profile contiguous.  `azimuth` (degrees) and `distance` (metres along the observer's
 * horizontal) are shared by all observers and live in the same memory space as the other arrays.
 * For every item, exactly this, with the reference's functions:
 *
 *     turtle_ecef_to_geodetic(p = position[r], &lat0, &lon0, &alt0);           (alt0 is not used)
 *     (E, N, U) = east, north, up at (lat0, lon0)     [the frame of turtle_ecef_from_horizontal]
 *     turtle_ecef_from_horizontal(lat0, lon0, azimuth[a], 0., h);  (the horizontal unit vector)
 *     best = -HUGE_VAL;  best_k = 0;
 *     for (k = 0; k < n_distances; k++) {
 *             s = distance[k];  q[j] = p[j] + s * h[j];              (a product, then a sum)
 *             turtle_ecef_to_geodetic(q, &la, &lo, &al);                      (al is not used)
 *             turtle_stepper_position(stepper, la, lo, 0., layer_index, g, &di);
 *             if (di < 0) continue;                (no data there: reported by omission, never raised)
 *             d = g - p;  rr = d0*d0 + d1*d1 + d2*d2;
 *             if (rr <= FLT_EPSILON) continue;               [turtle_ecef_to_horizontal's own test]
 *             arg = (U0*d0 + U1*d1 + U2*d2) / sqrt(rr);        (the sine of the elevation angle)
 *             if (arg > best) { best = arg; best_k = k + 1; best_range = sqrt(rr); }
 *     }
 *     sample[i] = best_k;                             (0: no sample of the line had data)
 *     if (best_k) { elevation[i] = best > 1. ? 90. : best < -1. ? -90. : asin(best) * 180. / M_PI;
 *                   if (range) range[i] = best_range; }       (else both keep their values)
 *
 * The choice is made on the sine, and asin is taken once, of the winner: the angle's maximum,
 * without near-vertical values collapsing into ties.  Ties go to the smallest k.  A NaN never wins
 * (a NaN distance gives one).  A sample at the observer's own foot (distance 0 from an observer
 * that turtle_stepper_position_n placed at height 0) is skipped by the rr test.  The arithmetic of
 * the selection is the strict one, as in turtle_stepper_position_n; only the two
 * turtle_ecef_to_geodetic transforms honour turtle_amd_math_set, as turtle_ecef_to_geodetic_n does.
 *
 * BAD_ADDRESS: stepper, position, azimuth, distance, elevation or sample NULL (range may be).
 * DOMAIN_ERROR: layer_index outside the stepper's layers ("no valid data"), an unknown space,
 * n * n_azimuths beyond an int.  n, n_azimuths or n_distances <= 0 does nothing and succeeds.
 * A wave cannot wait for a tile in the middle of its reduction, so every tile of every stack has
 * to be in memory, as for turtle_amd_stepper_view_acquire: the call loads what is missing
 * (turtle_stack_load) and fails with DOMAIN_ERROR where a stack's stack_size is below its number
 * of tiles.  turtle_amd_stepper_rounds reports 1 afterwards.  In DEVICE space the call only queues
 * work. */
TURTLE_API enum turtle_return turtle_stepper_horizon_n(
    struct turtle_stepper * stepper, long n, const double * position /* [n][3] */,
    int n_azimuths, const double * azimuth /* [n_azimuths], degrees */,
    int n_distances, const double * distance /* [n_distances], metres */,
    int layer_index, double * elevation /* [n][n_azimuths], in / out */,
    int * sample /* [n][n_azimuths], mandatory */,
    double * range /* [n][n_azimuths] or NULL */, int space);

/* The polar viewshed around n observers: which of the samples along the lines of
 * turtle_stepper_horizon_n the observer SEES -- which slopes the lines of sight of a muography
 * telescope enter first, which ground an antenna is in view of, and from which range on a target
 * `target_height` metres above the ground comes into view.  Items, observers, azimuths, distances,
 * the observer's frame (E, N, U) and the horizontal unit vector h are exactly those of
 * turtle_stepper_horizon_n; the distances are swept in the order they are given (increasing, for
 * a viewshed).  The outputs are [n][n_azimuths][n_distances], a line's samples contiguous:
 * element e = (long)i * n_distances + k.  For every item i, after horizon_n's preamble:
 *
 *     best = -HUGE_VAL;  count = 0;
 *     for (k = 0; k < n_distances; k++) {
 *             s = distance[k];  q[j] = p[j] + s * h[j];  turtle_ecef_to_geodetic(q, &la, &lo, &al);
 *             turtle_stepper_position(stepper, la, lo, 0., layer_index, g, &di);
 *             skip = (di < 0);                                              (no data there)
 *             if (!skip) { d = g - p;  rr = d0*d0 + d1*d1 + d2*d2;  skip = (rr <= FLT_EPSILON);
 *                          ground = (U0*d0 + U1*d1 + U2*d2) / sqrt(rr); }
 *             if (!skip) {
 *                     if (target_height == 0.) target = ground;
 *                     else { turtle_stepper_position(stepper, la, lo, target_height, layer_index, t, &di);
 *                            d = t - p;  rr = d0*d0 + d1*d1 + d2*d2;  skip = (rr <= FLT_EPSILON);
 *                            target = (U0*d0 + U1*d1 + U2*d2) / sqrt(rr); }
 *             }
 *             if (horizon) horizon[e] = best;    (the maximum of the GROUND sines of the samples before k)
 *             if (skip) { visible[e] = -1;  if (sine) sine[e] = NAN;  continue; }
 *             if (sine) sine[e] = target;
 *             v = (target >= best);              (a NaN is never visible; grazing counts as seen)
 *             visible[e] = v;  count += v;
 *             if (ground > best) best = ground;  (a NaN never raises the horizon)
 *     }
 *     if (n_visible) n_visible[i] = count;
 *
 * Every element of every output that is given is written: they are OUT only, nothing is read from
 * them.  The first sample with data is visible, behind a horizon of -HUGE_VAL.  A skipped sample
 * (-1) neither is seen nor hides anything.  The arithmetic is the strict one; only the
 * turtle_ecef_to_geodetic transforms honour turtle_amd_math_set, as in turtle_stepper_horizon_n --
 * and of a sample's transform only latitude and altitude: its longitude is the closed form's
 * atan2 in either arithmetic.  A line due north or south of an observer on a whole degree runs
 * along a seam of the tiles, where the last ulp of the longitude says which tile answers and,
 * beside a missing tile, whether a sample has data at all; those flags are the reference's too.
 * A maximum rounds nothing: whatever the order the samples of a line are combined in on the
 * device, horizon[] is the running maximum of the ground's sines to the bit.
 *
 * BAD_ADDRESS: stepper, position, azimuth, distance or visible NULL (sine, horizon and n_visible
 * may be).  DOMAIN_ERROR: layer_index outside the stepper's layers ("no valid data"), an unknown
 * space, n * n_azimuths beyond an int.  n, n_azimuths or n_distances <= 0 does nothing and
 * succeeds.  Every tile of every stack has to be in memory, as for turtle_stepper_horizon_n: the
 * call loads what is missing and fails with DOMAIN_ERROR where a stack's stack_size is below its
 * number of tiles; turtle_amd_stepper_rounds reports 1 afterwards.  In DEVICE space the call only
 * queues work. */
TURTLE_API enum turtle_return turtle_stepper_viewshed_n(
    struct turtle_stepper * stepper, long n, const double * position /* [n][3] */,
    int n_azimuths, const double * azimuth /* [n_azimuths], degrees */,
    int n_distances, const double * distance /* [n_distances], metres, in the order they are swept */,
    int layer_index, double target_height /* metres above the layer's top */,
    signed char * visible /* [n][n_azimuths][n_distances], mandatory */,
    double * sine /* same shape, or NULL */, double * horizon /* same shape, or NULL */,
    int * n_visible /* [n][n_azimuths], or NULL */, int space);

/* Flags of turtle_stepper_clearance_n. */
enum turtle_amd_clearance_flags {
        /* line r joins observer[r] to target[r] (m must equal n); outputs are [n] */
        TURTLE_AMD_CLEARANCE_PAIRED = 1
};

/* The clearance of point-to-point lines: which of n observers and m targets (antennas, shower
 * maxima in the air, telescope sites, the nodes of a map lifted by turtle_stepper_position_n) see
 * each other over the top of a layer, and by what margin.  Where the two calls above follow an
 * observer's horizontal tangent and judge by angles, this one samples the true straight chord
 * between the two points, at the fractions `fraction` of it (shared by all lines, in the same
 * memory space as the other arrays), and reduces it to its minimum height above the layer's top.
 * Item i = r * m + t is the line from observer r to target t, the outputs observer-major [n][m];
 * with TURTLE_AMD_CLEARANCE_PAIRED item i = r is the line from observer r to target r and the
 * outputs are [n].  For every item, exactly this, with the reference's functions:
 *
 *     p = observer[r];  t = target[..];  d[j] = t[j] - p[j];
 *     best = HUGE_VAL;  best_k = 0;  count = 0;
 *     for (k = 0; k < n_fractions; k++) {
 *             f = fraction[k];  q[j] = p[j] + f * d[j];                     (a product, then a sum)
 *             turtle_ecef_to_geodetic(q, &la, &lo, &al);                    (al is not used)
 *             turtle_stepper_position(stepper, la, lo, 0., layer_index, g, &di);
 *             if (di < 0) continue;                                         (no data under the sample)
 *             count++;
 *             U = (cos(lo) cos(la), sin(lo) cos(la), sin(la));    [ref ecef.c:151-153, the sample's vertical;
 *                                                                  of la, lo * M_PI / 180.]
 *             c = U0*(q0 - g0) + U1*(q1 - g1) + U2*(q2 - g2);     (metres above the layer's top; < 0: below it)
 *             if (c < best) { best = c; best_k = k + 1; }         (ties to the smallest k; a NaN never wins)
 *     }
 *     sample[i] = best_k;  if (n_data) n_data[i] = count;
 *     if (best_k) clearance[i] = best;                            (else it keeps its value)
 *
 * The pair sees each other over that layer iff clearance[i] >= 0 -- or above a margin of the
 * caller's own (a Fresnel zone, the mast that would make a blocked pair visible); sample[i] says
 * where along the chord it comes closest, n_data[i] how many samples had data under them.  The
 * fractions are not checked: values outside [0, 1] extrapolate the chord, repeated values are
 * legal; at 0 and 1 the clearance is the end point's own height.  p == t is not special.  The
 * arithmetic is the strict one; only the sample's turtle_ecef_to_geodetic honours
 * turtle_amd_math_set, exactly as a sample of turtle_stepper_viewshed_n does: FAST takes latitude
 * and altitude from the fast transform and the longitude from the closed form's atan2, which keeps
 * n_data the reference's beside seams and missing tiles.
 *
 * BAD_ADDRESS: stepper, observer, target, fraction, clearance or sample NULL (n_data may be).
 * DOMAIN_ERROR: layer_index outside the stepper's layers ("no valid data"), an unknown space,
 * unknown flag bits, PAIRED with m != n, a number of lines beyond an int; all of them before a
 * device is touched, changing nothing.  n, m or n_fractions <= 0 does nothing and succeeds.  Every
 * tile of every stack has to be in memory, as for turtle_stepper_horizon_n: the call loads what is
 * missing and fails with DOMAIN_ERROR where a stack's stack_size is below its number of tiles;
 * turtle_amd_stepper_rounds reports 1 afterwards.  In DEVICE space the call only queues work. */
TURTLE_API enum turtle_return turtle_stepper_clearance_n(
    struct turtle_stepper * stepper, long n, const double * observer /* [n][3] */,
    long m, const double * target /* [m][3] */,
    int n_fractions, const double * fraction /* [n_fractions], shared by all lines */,
    int layer_index, int flags,
    double * clearance /* [n][m] (or [n]), in / out */,
    int * sample /* same shape, mandatory */,
    int * n_data /* same shape, or NULL */, int space);

/* Flags of turtle_stepper_step_n. */
enum turtle_amd_step_flags {
        /* On entry altitude[], elevation[][2] and index[][2] hold the values a
         * previous call returned for the SAME positions: skip the sample at
         * the start point, exactly as the reference's `last` cache does when
         * the position is unchanged [impl stepper.c:708-710, :745-748].  A ray
         * handed back with index[r][0] = -1 has left the data and takes no step
         * (step[r] = 0), whatever a fresh sample of the point where its exit
         * was located, within 1e-8 m of the rim, would say. */
        TURTLE_AMD_STEP_RESUME = 1
};

/* n independent turtle_stepper_step calls.  `direction` may be NULL (sample
 * only; step[] is the tentative length).  Every output array may be NULL
 * except index, which is mandatory: leaving the data is reported as
 * index[r][0] = -1, never raised.  position is updated in place. */
TURTLE_API enum turtle_return turtle_stepper_step_n(
    struct turtle_stepper * stepper, long n, double * position /* [n][3] */,
    const double * direction /* [n][3] or NULL */, double * latitude,
    double * longitude, double * altitude, double * elevation /* [n][2] */,
    double * step, int * index /* [n][2] */, int flags, int space);

/* The same steps for a walk that keeps the LEAST state between its calls.  What a step resumes
 * from is the medium the ray is in and the tentative length its last sample gave it [impl
 * stepper.c:799-813: all the reference reads its cached sample for]: `next` holds that length --
 * one double in, one out, where turtle_stepper_step_n with TURTLE_AMD_STEP_RESUME moves altitude and
 * two elevations each way (a third of what a step streams; a batch of single steps is bound by its
 * memory traffic) -- and `index` the medium.  direction == NULL begins a walk: the positions are
 * sampled, `next` and `index` filled (step[], if given, is that tentative length too); with a
 * direction every ray with index[r][0] >= 0 takes the step turtle_stepper_step would: position
 * advanced in place, step[r] its length, index[r] and next[r] for the one after.  A ray that has
 * left the data (index[r][0] = -1) takes no step.  The same arithmetic on the same values as the
 * RESUME form: the same bits. */
TURTLE_API enum turtle_return turtle_stepper_walk_n(
    struct turtle_stepper * stepper, long n, double * position /* [n][3] */,
    const double * direction /* [n][3], or NULL to begin */, double * next /* [n], in / out */,
    double * step /* [n] or NULL */, int * index /* [n][2], in / out */, int space);

/* Flags of turtle_stepper_scatter_n. */
enum turtle_amd_scatter_flags {
        /* Begin a walk: sample the positions first (as turtle_stepper_step_n with
         * a NULL direction does) and zero length[] and steps[].  Without it the
         * call continues the walk whose state the arrays hold. */
        TURTLE_AMD_SCATTER_START = 1
};

/* A scattering walk: generations first_step .. first_step + n_steps - 1 of
 *     for every ray still inside the data (index[r][0] >= 0):
 *         turtle_stepper_step(position[r], direction = isotropic unit vector of
 *                             Philox(first_ray + r, generation; seed))
 *         length[r] += the step's length;  steps[r] += 1
 * i.e. the loop of examples/example-pthread.c:66-99 with a new direction at
 * every step (turtle_amd_isotropic_n gives the same vectors), each step resumed
 * from the sample the last one returned (TURTLE_AMD_STEP_RESUME: one sample per
 * step, as the reference's `last` cache has it [impl stepper.c:708-710]).  The
 * directions are drawn inside the step kernels and the sums kept there, so a
 * generation moves 80 bytes of ray state in and 64 out and nothing else.
 * altitude, elevation and index are the sample state between generations (in /
 * out; filled by the call itself with TURTLE_AMD_SCATTER_START); a ray that
 * leaves the data keeps index[r][0] = -1 and takes no further step.
 * turtle_stepper_trace_stats reports the totals of the call. */
TURTLE_API enum turtle_return turtle_stepper_scatter_n(
    struct turtle_stepper * stepper, long n, double * position /* [n][3] */,
    unsigned long long seed, long first_ray, int first_step, int n_steps,
    double * altitude, double * elevation /* [n][2] */, int * index /* [n][2] */,
    double * length, int * steps, int flags, int space);

/* Flags of turtle_stepper_trace_n. */
enum turtle_amd_trace_flags {
        /* On entry index[r][0] holds the medium the ray is in, as returned by
         * the previous trace/step that left it at this position.  A ray that
         * has just been put ON a boundary by the bisection sits within 1e-8 m
         * of it, where re-deriving the medium from a fresh sample is
         * ill-conditioned; the reference never re-derives it either (its next
         * step starts from the cached `last` sample [impl stepper.c:708-710,
         * :826]).  Use this flag to continue rays through successive media. */
        TURTLE_AMD_TRACE_RESUME = 1
};

/* The per-ray loop of a Monte-Carlo harness, moved into one kernel: for each
 * ray sample its start point, then step until index[0] differs from its
 * initial value (a boundary was located) or max_steps steps were taken
 * [shape of examples/example-stepper.c:128-140].  Outputs per ray: final
 * index pair, path length = sum of the step lengths, number of steps; the
 * position is advanced in place.  Rays that start outside the data take 0
 * steps and report index[0] = -1.  length/n_steps may be NULL: which outputs a
 * caller asks for changes neither the kernels that run nor a bit of the others. */
TURTLE_API enum turtle_return turtle_stepper_trace_n(
    struct turtle_stepper * stepper, long n, double * position /* [n][3] */,
    const double * direction /* [n][3] */, int max_steps,
    int * index /* [n][2] */, double * length, int * n_steps, int flags,
    int space);

/* ---- the stepper inside the caller's own kernel (turtle_amd_device.h) ----------------
 *
 * turtle_amd_stepper_view_acquire lends a kernel the stepper's geometry: it flattens the
 * stepper for the calling thread's device, brings every tile of every stack into memory (as
 * turtle_stack_load does), copies a `struct turtle_amd_view` (turtle_amd_device.h) to `view`
 * and keeps everything the view points at where it is until
 * turtle_amd_stepper_view_release(stepper), called by the same thread.  `size` is the caller's
 * sizeof(struct turtle_amd_view): the library refuses a view that is not laid out as its own
 * (turtle_amd_view_layout gives the library's version and size).
 *   BAD_ADDRESS    stepper or view is NULL
 *   DOMAIN_ERROR   `size` is not the library's; the view is out already; a stack's stack_size
 *                  is below the number of its tiles (the device side does not page)
 *   LIBRARY_ERROR  no usable device ("no HIP device is visible ...")
 * Ordering is the caller's: the library's own work is ordered on the thread's stream
 * (turtle_amd_stream_set, turtle_amd_synchronize); the acquire returns with the tables in
 * place, the caller's kernels may be launched on any stream after it returns, and must have
 * FINISHED before the release.
 * While a thread holds a view, batch calls over resident geometry work as ever (on that
 * stepper too).  What would change the geometry fails in the holding thread with DOMAIN_ERROR
 * instead of waiting for its own view: turtle_map_fill, turtle_map_fill_n, turtle_map_resample,
 * turtle_stack_clear / _load, turtle_map_destroy / turtle_stack_destroy (through the handler;
 * the object stays), a batch call that has to page tiles in, and, on the stepper itself,
 * turtle_stepper_add_* and turtle_stepper_destroy.  Other threads that would change it wait
 * for the release, as they wait for a batch call.  Releasing what is not held: DOMAIN_ERROR. */
TURTLE_API enum turtle_return turtle_amd_stepper_view_acquire(
    struct turtle_stepper * stepper, void * view, size_t size);
TURTLE_API enum turtle_return turtle_amd_stepper_view_release(struct turtle_stepper * stepper);
TURTLE_API void turtle_amd_view_layout(int * version, size_t * size);

/* Number of media of the stepper's geometry: its layers + 1 (index[0] ranges
 * over [0, media)). */
TURTLE_API int turtle_amd_stepper_media(const struct turtle_stepper * stepper);

/* Lines of sight: the rock length along each ray, every medium it meets, in one
 * call.  For each ray r, exactly what this loop does with a fresh stepper history
 * per ray [the loop of the reference's examples/example-stepper.c:128-140]:
 *
 *     turtle_stepper_step(s, pos, NULL, NULL, NULL, &alt, NULL, NULL, idx);
 *     while (idx[0] >= 0 && alt < altitude_max && steps < max_steps) {
 *             const int m = idx[0];
 *             turtle_stepper_step(s, pos, dir, NULL, NULL, &alt, NULL, &ds, idx);
 *             length[m * n + r] += ds;  steps++;  if (idx[0] != m) crossings++;
 *     }
 *
 * The one departure from the reference's loop is the test idx[0] >= 0: its loop
 * never ends on a ray that leaves the data (a step from outside returns ds = 0
 * with the altitude unchanged).  altitude_max = HUGE_VAL: until the data ends or
 * max_steps.  A ray that starts outside the data, or at or above the ceiling,
 * takes 0 steps and reports the sample at its origin.  Outputs: position advanced
 * in place; index[r] the final sample's pair; length medium-major, [media][n]
 * (turtle_amd_stepper_media), each medium's column contiguous (it can go to
 * turtle_amd_tally_n as it is), each sum accumulated step by step in the loop's
 * order; n_steps and n_crossings per ray.  length, n_steps and n_crossings may be
 * NULL: which outputs a caller asks for changes no bit of the others.
 * turtle_stepper_trace_stats reports the call.  n <= 0 does nothing.
 * Each crossing is located by HALVING the step's bracket, as the reference does,
 * in either arithmetic (turtle_amd_math_set).  STRICT: the reference's arithmetic,
 * up to the last ulp of asin/acos/atan2.  WHAT IS GUARANTEED in both (and tested
 * against the reference's golden vectors and the CPU restatement at full size):
 * the same final medium; the same step and crossing counts and every per-medium
 * length within 1e-6 of the ray's total path, except on a ray that grazes a
 * surface or cuts a sliver of it thinner than its step, where an ulp decides a
 * sample (measured: 2 of 2e5 C2 rays on the sin.cos tile, ~40 of 2e5 on a rough
 * tile with 200 m of node-to-node noise; DESIGN.md 3.7 and the test name them).
 * Over stacks with tiles to page in, the rays go generation by generation over
 * the step kernels (same bits in STRICT). */
TURTLE_API enum turtle_return turtle_stepper_traverse_n(
    struct turtle_stepper * stepper, long n, double * position /* [n][3], in / out */,
    const double * direction /* [n][3] */, double altitude_max, int max_steps,
    int * index /* [n][2], out: final */, double * length /* [media][n] or NULL */,
    int * n_steps /* [n] or NULL */, int * n_crossings /* [n] or NULL */, int space);

/* Lines of sight with every crossing point: turtle_stepper_traverse_n's loop and outputs, and
 * where each ray changed medium.  For each ray r, exactly (a fresh stepper history per ray):
 *
 *     turtle_stepper_step(s, pos, NULL, NULL, NULL, &alt, NULL, NULL, idx);  d = 0;
 *     while (idx[0] >= 0 && alt < altitude_max && steps < max_steps) {
 *             m = idx[0];  turtle_stepper_step(s, pos, dir, NULL, NULL, &alt, NULL, &ds, idx);
 *             length[m*n + r] += ds;  d += ds;  steps++;
 *             if (idx[0] != m) {
 *                     c = crossings++;
 *                     if (c < capacity) { point[c][r] = pos; distance[c][r] = d; media[c][r] = {m, idx[0]}; }
 *             }
 *     }
 *
 * n_crossings[r] is the true count: it may exceed capacity, and then only the first `capacity`
 * crossings are recorded.  The slots from min(n_crossings[r], capacity) on are zero: point and
 * distance 0, media {0, 0} (no crossing has that pair).  Leaving the data is a crossing, media
 * {m, -1}, at the ray's final position; stopping at the ceiling or at max_steps is not.  The
 * slot arrays are crossing-major, as length is medium-major: slot c of ray r is element
 * (long)c * n + r, each slot's column contiguous.  point, distance, media, length and n_steps may
 * be NULL; capacity = 0 records nothing (traverse_n with the counts).  position, index, length,
 * n_steps and n_crossings are bit for bit those of turtle_stepper_traverse_n on the same inputs,
 * in either arithmetic, resident or paged: recording a crossing changes no decision and no
 * addition.  turtle_stepper_trace_stats reports the call as it does traverse_n.  BAD_ADDRESS:
 * position, direction, index or n_crossings NULL; DOMAIN_ERROR: max_steps < 0 or capacity < 0;
 * n <= 0 does nothing. */
TURTLE_API enum turtle_return turtle_stepper_crossings_n(
    struct turtle_stepper * stepper, long n, double * position /* [n][3], in / out */,
    const double * direction /* [n][3] */, double altitude_max, int max_steps,
    int * index /* [n][2], out: final */, double * length /* [media][n] or NULL */,
    int * n_steps /* [n] or NULL */, int * n_crossings /* [n], mandatory */,
    int capacity, double * point /* [capacity][n][3] or NULL */,
    double * distance /* [capacity][n] or NULL */, int * media /* [capacity][n][2] or NULL */,
    int space);

/* Why turtle_stepper_advance_n stopped a ray. */
enum turtle_amd_advance_status {
        TURTLE_AMD_ADVANCE_SPENT = 0,     /* the depth budget ran out (or was <= 0, or NaN, at the origin) */
        TURTLE_AMD_ADVANCE_DISTANCE = 1,  /* distance_max was reached */
        TURTLE_AMD_ADVANCE_LEFT = 2,      /* the ray left the data (or started outside it) */
        TURTLE_AMD_ADVANCE_CEILING = 3,   /* altitude >= altitude_max */
        TURTLE_AMD_ADVANCE_MAX_STEPS = 4
};

/* Rays advanced by a column-depth budget: turtle_stepper_traverse_n's loop, which the physics may
 * stop before the geometry does -- after the column depth budget[r] (the sum of density[medium] x
 * path: a muon's range, the grammage to an interaction) or at the distance distance_max[r] (the
 * other end of a chord).  density has turtle_amd_stepper_media(stepper) elements and lies, like
 * every array of the call, in `space`.  For each ray r, exactly (a fresh stepper history per ray;
 * B = budget[r], M = distance_max ? distance_max[r] : HUGE_VAL):
 *
 *     turtle_stepper_step(s, pos, NULL, NULL, NULL, &alt, NULL, NULL, idx);  X = 0; d = 0; steps = 0;
 *     for (;;) {
 *             if (idx[0] < 0)            { status = LEFT; break; }
 *             if (!(X < B))              { status = SPENT; break; }
 *             if (!(d < M))              { status = DISTANCE; break; }
 *             if (!(alt < altitude_max)) { status = CEILING; break; }
 *             if (steps >= max_steps)    { status = MAX_STEPS; break; }
 *             m = idx[0]; k = idx[1]; p0 = pos;                      (the step starts in medium m)
 *             turtle_stepper_step(s, pos, dir, NULL, NULL, &alt, NULL, &ds, idx);
 *             x = density[m] * ds;
 *             spent = (X + x >= B);  far = (d + ds >= M);
 *             if (spent || far) {                 (the step is cut short: by the model it lies in medium m)
 *                     f = ds;  status = SPENT;
 *                     if (far)   { f = M - d; status = DISTANCE; }
 *                     if (spent) { fs = (B - X) / density[m]; if (fs <= f) { f = fs; status = SPENT; } }
 *                     if (f > ds) f = ds;                            (a rounding guard)
 *                     pos[j] = p0[j] + dir[j] * f;                   (a product, then a sum)
 *                     if (status == SPENT) { X = B; d += f; } else { X += density[m] * f; d = M; }
 *                     steps++; idx[0] = m; idx[1] = k; break;
 *             }
 *             X += x; d += ds; steps++;
 *     }
 *     index[r] = idx; depth[r] = X; distance[r] = d; n_steps[r] = steps; status[r] = status;
 *
 * (`status = SPENT` before the two ifs decides the one case they leave open: spent alone, with fs
 * rounded above ds.)  What follows from it, and is tested:
 *  - with budget = HUGE_VAL, distance_max = NULL and finite densities, position, index and n_steps
 *    are bit for bit those of turtle_stepper_traverse_n on the same inputs: the tests on a ray are
 *    traverse's, in traverse's order, and the budget tests never fire; distance is then the bits of
 *    the last recorded distance of turtle_stepper_crossings_n for a ray that left the data;
 *  - with every density equal to 1, depth == distance to the bit on every ray that no cut stopped;
 *  - a density of 0 (vacuum) never spends anything, and a division by it cannot happen: spent needs
 *    x > 0;
 *  - densities and budgets are not checked (as turtle_stepper_clearance_n does not check its
 *    fractions); a NaN budget stops the ray at its origin as SPENT;
 *  - point to point: direction the unit vector from p to t and distance_max = |t - p|; status
 *    DISTANCE then means that the chord lies inside the data and under the ceiling, depth is the
 *    column depth between the two points, and with density = {1, 0, ...} the rock between them;
 *  - after a cut the ray stands INSIDE medium index[r][0], not on a boundary: a later call from that
 *    position starts from a fresh sample.
 * Arithmetic follows turtle_amd_math_set as turtle_stepper_traverse_n does; crossings are located
 * by halving in either mode, and the cut itself (fs, f, the position, X, d) is plain IEEE arithmetic
 * in the order stated.  depth, distance, n_steps and distance_max may be NULL: which outputs a
 * caller asks for changes no bit of the others.  BAD_ADDRESS: stepper, position, direction, density,
 * budget, index or status NULL; DOMAIN_ERROR: max_steps < 0 or an unknown space (both before a
 * device is touched: nothing changes); n <= 0 does nothing.  Every tile of every stack has to be
 * in memory, as for turtle_stepper_horizon_n: the call loads what is missing and fails with
 * DOMAIN_ERROR where a stack's stack_size is below its number of tiles (a cut needs the position
 * a step began at, which the paged, generation-by-generation form does not keep).
 * turtle_amd_stepper_rounds reports 1, turtle_stepper_trace_stats reports the call as it does
 * traverse_n.  In DEVICE space the call only queues work. */
TURTLE_API enum turtle_return turtle_stepper_advance_n(
    struct turtle_stepper * stepper, long n, double * position /* [n][3], in / out */,
    const double * direction /* [n][3] */, const double * density /* [media] */,
    const double * budget /* [n] */, const double * distance_max /* [n] or NULL */,
    double altitude_max, int max_steps, int * index /* [n][2], out */,
    double * depth /* [n] or NULL */, double * distance /* [n] or NULL */,
    int * n_steps /* [n] or NULL */, int * status /* [n], mandatory */, int space);

/* turtle_stepper_advance_n through media whose density falls off with altitude: the density of
 * medium m at altitude h is density[m] * exp(-h / scale_height[m]), h the altitude that
 * turtle_stepper_step returns and density[m] the density at h = 0 (air: 1.205 kg/m^3 and 8400 m).
 * scale_height has turtle_amd_stepper_media(stepper) elements, in `space`; scale_height[m] =
 * HUGE_VAL makes medium m uniform, scale_height = NULL every medium.  The model: WITHIN A STEP THE
 * ALTITUDE IS TAKEN AS LINEAR IN THE PATH, from the altitude a0 the step began at to the altitude
 * a1 it ended at, so that the density f metres into the step is c * exp(w * f).  For each ray r,
 * exactly, turtle_stepper_advance_n's loop with the same tests in the same order, the step's law in
 * the place of density[m] * ds, and the law's inverse in the cut:
 *
 *     turtle_stepper_step(s, pos, NULL, NULL, NULL, &alt, NULL, NULL, idx);  X = 0; d = 0; steps = 0;
 *     for (;;) {
 *             if (idx[0] < 0)            { status = LEFT; break; }
 *             if (!(X < B))              { status = SPENT; break; }
 *             if (!(d < M))              { status = DISTANCE; break; }
 *             if (!(alt < altitude_max)) { status = CEILING; break; }
 *             if (steps >= max_steps)    { status = MAX_STEPS; break; }
 *             m = idx[0]; k = idx[1]; p0 = pos; a0 = alt;           (the step starts in medium m, at a0)
 *             turtle_stepper_step(s, pos, dir, NULL, NULL, &alt, NULL, &ds, idx);  a1 = alt;
 *             if (scale_height == NULL || scale_height[m] == HUGE_VAL) { c = density[m]; w = 0; }
 *             else { H = scale_height[m];  c = density[m] * exp(-a0 / H);  w = -((a1 - a0) / H) / ds; }
 *             S(f) := (w * f == 0) ? c * f : c * expm1(w * f) / w   (the depth of the step's first f metres)
 *             x = S(ds);
 *             spent = (X + x >= B);  far = (d + ds >= M);
 *             if (spent || far) {
 *                     f = ds;  status = SPENT;
 *                     if (far)   { f = M - d; status = DISTANCE; }
 *                     if (spent) { fs = (w == 0) ? (B - X) / c : log1p((B - X) * w / c) / w;
 *                                  if (fs <= f) { f = fs; status = SPENT; } }    (a NaN fs leaves f as it was)
 *                     if (f > ds) f = ds;
 *                     pos[j] = p0[j] + dir[j] * f;
 *                     if (status == SPENT) { X = B; d += f; } else { X += S(f); d = M; }
 *                     steps++; idx[0] = m; idx[1] = k; break;
 *             }
 *             X += x; d += ds; steps++;
 *     }
 *     index[r] = idx; depth[r] = X; distance[r] = d; n_steps[r] = steps; status[r] = status;
 *
 * What follows from it, and is tested:
 *  - with scale_height = NULL, or every element HUGE_VAL, every output is bit for bit
 *    turtle_stepper_advance_n's: c = density[m], w = 0, and both branches are its expressions;
 *  - a SPENT ray has depth == budget and a DISTANCE ray distance == distance_max, to the bit;
 *  - status, position and n_steps are turtle_stepper_traverse_n's whenever no cut fires;
 *  - one call answers "where along this line has the particle crossed 800 g/cm^2?" (budget) and
 *    "what is the slant depth between these two points?" (distance_max = |t - p|, budget = HUGE_VAL).
 * Neither density nor scale_height is checked: a zero, negative or NaN scale height gives what the
 * arithmetic above gives.  exp, expm1 and log1p are the plain double-precision functions in either
 * arithmetic (turtle_amd_math_set); the device keeps 1 / scale_height[m] and multiplies by it, so a
 * result agrees with the statement above to rounding, not to the bit, where a medium is not
 * uniform.  The same arithmetic is column_depth and column_reach of turtle_amd_device.h.
 *
 * The model's error.  Along a straight line the altitude departs from linear by the Earth's
 * curvature, at most ds^2 / (8 R) over a step of length ds (R the Earth's radius), so the depth of
 * a step is off by at most ds^2 / (8 R H) of itself.  Steps in air far from any surface are the
 * long ones; flat layers at band boundaries (turtle_stepper_add_flat) shorten steps only near those
 * boundaries.  Measured on the 961 climbing rays of the tests' 1201^2 tile that stay in the air
 * (scripts/exp_advance_exp_model.py: to the edge of the tile, up to 54 km of altitude, longest step
 * 16.5 km), against a quadrature of the density along the true line every 5 m: the depth of a ray
 * is off by at most 2.3e-5 of itself, where the bound for that ray's longest step is 5.7e-4.
 *
 * Everything else -- optional outputs, errors and their order, resident tiles only,
 * turtle_amd_stepper_rounds, turtle_stepper_trace_stats, spaces -- is turtle_stepper_advance_n's;
 * scale_height = NULL is no error. */
TURTLE_API enum turtle_return turtle_stepper_advance_exp_n(
    struct turtle_stepper * stepper, long n, double * position /* [n][3], in / out */,
    const double * direction /* [n][3] */, const double * density /* [media] */,
    const double * scale_height /* [media] or NULL */,
    const double * budget /* [n] */, const double * distance_max /* [n] or NULL */,
    double altitude_max, int max_steps, int * index /* [n][2], out */,
    double * depth /* [n] or NULL */, double * distance /* [n] or NULL */,
    int * n_steps /* [n] or NULL */, int * status /* [n], mandatory */, int space);

/* A box of voxels with straight edges in ECEF, each voxel one density: the rock of a volcano, an
 * ore body, an aquifer under a hill.  A voxel (i0, i1, i2) spans origin + sum over a of
 * axis[a] * [i_a, i_a + 1] * size[a].  The axes are taken as given and are expected to be
 * orthonormal (turtle_amd_grid_enu makes them so); they are not checked. */
struct turtle_amd_grid {
        double origin[3];       /* ECEF of the corner of voxel (0, 0, 0) that every axis leaves from */
        double axis[3][3];      /* unit vectors of the grid's three directions, in ECEF */
        double size[3];         /* a voxel's edge along each axis, metres */
        int n[3];               /* voxels along each axis */
        int medium;             /* the medium the grid describes (0: under the first layer's top) */
        const double * density; /* [n[2]][n[1]][n[0]], axis 0 fastest; lies in the call's `space` */
};

/* origin and axis of a box whose axes are east, north, up at (latitude, longitude) [the frame of
 * turtle_ecef_from_horizontal], its origin `east0`, `north0`, `up0` metres from the point
 * (latitude, longitude, height) along them.  Host arithmetic; fills grid->origin and grid->axis only. */
TURTLE_API void turtle_amd_grid_enu(struct turtle_amd_grid * grid, double latitude, double longitude,
    double height, double east0, double north0, double up0);

/* turtle_stepper_advance_n through rock whose density varies in three dimensions: inside the box
 * `grid` the density of medium grid->medium is the voxel's; outside the box that medium has
 * density[grid->medium], and every other medium is turtle_stepper_advance_n's.  A ray is a straight
 * line in ECEF and so are the box's edges: the depth of a step is an exact sum over the voxels it
 * meets, not a quadrature.  The struct itself is read on the host in both spaces; only
 * grid->density follows `space` (HOST: staged to the device for the call; DEVICE: read where it
 * lies).  For each ray r, exactly, turtle_stepper_advance_n's loop with its tests in its order; one
 * walk a step takes the place of density[m] * ds and of the cut:
 *
 *     turtle_stepper_step(s, pos, NULL, NULL, NULL, &alt, NULL, NULL, idx);  X = 0; d = 0; steps = 0;
 *     for (;;) {
 *             if (idx[0] < 0)            { status = LEFT; break; }
 *             if (!(X < B))              { status = SPENT; break; }
 *             if (!(d < M))              { status = DISTANCE; break; }
 *             if (!(alt < altitude_max)) { status = CEILING; break; }
 *             if (steps >= max_steps)    { status = MAX_STEPS; break; }
 *             m = idx[0]; k = idx[1]; p0 = pos;
 *             turtle_stepper_step(s, pos, dir, NULL, NULL, &alt, NULL, &ds, idx);
 *             far = (d + ds >= M);  L = far ? M - d : ds;  if (L > ds) L = ds;
 *             (x, f, stopped) = grid_depth(grid, density[m], m, p0, dir, L, B - X);
 *             if (stopped) { pos = p0 + dir * f; X = B;  d += f; steps++; idx = {m, k}; status = SPENT;    break; }
 *             if (far)     { pos = p0 + dir * L; X += x; d = M;  steps++; idx = {m, k}; status = DISTANCE; break; }
 *             X += x; d += ds; steps++;
 *     }
 *     index[r] = idx; depth[r] = X; distance[r] = d; n_steps[r] = steps; status[r] = status;
 *
 * grid_depth(G, rho_out, m, p0, dir, L, R) goes through the pieces of [0, L] in order and adds
 * rho * (b - a) for each piece (a, b, rho) to a running sum acc, starting from 0.  A piece with
 * x = rho * (b - a) > 0 and acc + x >= R stops the walk at f = a + (R - acc) / rho (stopped): a
 * piece of density 0 never stops a ray and never divides.  Otherwise the walk returns x = acc,
 * f = L, not stopped.  The pieces:
 *
 *     if (G == NULL || m != G->medium): one piece (0, L, rho_out).
 *     s[a] = axis[a][0]*(p0[0]-origin[0]) + axis[a][1]*(p0[1]-origin[1]) + axis[a][2]*(p0[2]-origin[2]);
 *     t[a] = axis[a][0]*dir[0] + axis[a][1]*dir[1] + axis[a][2]*dir[2];                  (a = 0, 1, 2)
 *     f0 = 0; f1 = L; hit = 1;                                                           (the slab test)
 *     for a: E = n[a] * size[a];
 *            if (t[a] == 0) { if (!(s[a] >= 0 && s[a] < E)) hit = 0; }
 *            else { u = (0 - s[a]) / t[a]; v = (E - s[a]) / t[a]; if (u > v) swap(u, v);
 *                   if (u > f0) f0 = u;  if (v < f1) f1 = v; }
 *     f = 0;
 *     if (hit && f0 < f1) {
 *             piece (0, f0, rho_out);
 *             for a: i[a] = clamp((int)floor((s[a] + f0 * t[a]) / size[a]), 0, n[a] - 1);
 *                    next[a] = (t[a] == 0) ? HUGE_VAL : ((i[a] + (t[a] > 0)) * size[a] - s[a]) / t[a];
 *             f = f0;
 *             for (;;) {
 *                     a = the axis of the least next[] (ties: the lowest a);
 *                     g = min(next[a], f1);  if (g < f) g = f;                           (no piece is negative)
 *                     piece (f, g, G->density[((long)i[2] * n[1] + i[1]) * n[0] + i[0]]);
 *                     f = g;
 *                     if (!(next[a] < f1)) break;
 *                     i[a] += (t[a] > 0) ? 1 : -1;  if (i[a] < 0 || i[a] >= n[a]) break;
 *                     next[a] = ((i[a] + (t[a] > 0)) * size[a] - s[a]) / t[a];           (from the index: nothing accumulates)
 *             }
 *     }
 *     piece (f, L, rho_out);                                  (what lies past the box, or all of it)
 *
 * What follows from it, and is tested:
 *  - grid = NULL is turtle_stepper_advance_n, bit for bit (the same kernel instance runs); error
 *    messages carry this call's name;
 *  - a SPENT ray has depth == budget and a DISTANCE ray distance == distance_max, to the bit;
 *  - status, position and n_steps of a ray that no cut stopped are turtle_stepper_traverse_n's bits;
 *  - a grid whose voxels all hold density[medium] agrees with turtle_stepper_advance_n to rounding
 *    (one rounding a piece met), not to the bit: the sum is taken piece by piece;
 *  - a voxel of density 0 (a void) spends nothing; where rock is void the place a budget ends is
 *    discontinuous in the budget;
 *  - densities are not checked.
 * The walk is turtle_amd_device.h's grid_depth, for callers that step rays in their own kernel.
 * BAD_ADDRESS as turtle_stepper_advance_n, and grid != NULL with grid->density == NULL.
 * DOMAIN_ERROR as turtle_stepper_advance_n, and: an n[a] < 1, a size[a] that is not finite and
 * > 0, n[0] * n[1] * n[2] beyond an int, medium outside [0, media).  All of them before a device is
 * touched: nothing changes.  Everything else -- statuses, optional outputs, resident tiles only
 * (paged stacks are refused), turtle_amd_stepper_rounds (1), turtle_stepper_trace_stats, spaces --
 * is turtle_stepper_advance_n's.  Not offered: a grid together with scale heights, more than one
 * grid, densities interpolated between voxel centres. */
TURTLE_API enum turtle_return turtle_stepper_advance_grid_n(
    struct turtle_stepper * stepper, long n, double * position /* [n][3], in / out */,
    const double * direction /* [n][3] */, const double * density /* [media] */,
    const struct turtle_amd_grid * grid /* host memory, or NULL */,
    const double * budget /* [n] */, const double * distance_max /* [n] or NULL */,
    double altitude_max, int max_steps, int * index /* [n][2], out */,
    double * depth /* [n] or NULL */, double * distance /* [n] or NULL */,
    int * n_steps /* [n] or NULL */, int * status /* [n], mandatory */, int space);

/* Totals of the LAST trace_n, scatter_n, traverse_n, crossings_n, advance_n, advance_exp_n or advance_grid_n call on this stepper,
 * accumulated on the device: stats[0] rays, [1] steps, [2] samples (transform +
 * layer lookup; the same from run to run), [3] rays that stopped at max_steps.
 * Synchronises the stream. */
TURTLE_API enum turtle_return turtle_stepper_trace_stats(
    struct turtle_stepper * stepper, unsigned long long stats[4]);

/* Rounds the last batch call on this stepper took: 1 when every tile it needed was
 * in memory, one more each time tiles had to come in for rays that waited (paged
 * stacks: stack_size below the tiles a batch touches). */
TURTLE_API int turtle_amd_stepper_rounds(const struct turtle_stepper * stepper);

/* Reduce trace results for a multi-GPU tally: hits[m + 1] counts
 * rays whose final index[0] == m, for m in [-1, n_media); histogram[b] counts
 * path lengths in bin b of n_bins linear bins over [0, length_max), the last
 * extra bin (histogram[n_bins]) collecting overflows.  Both are uint64 and are
 * ADDED to, so ranks can accumulate and then all-reduce them. */
TURTLE_API enum turtle_return turtle_amd_tally_n(long n,
    const int * index /* [n][2] */, const double * length, int n_media,
    unsigned long long * hits /* [n_media + 1] */, int n_bins,
    double length_max, unsigned long long * histogram /* [n_bins + 1] */,
    int space);

/* Counter-based random directions for scattering harnesses (BASELINE config
 * C5: a new isotropic direction after every step).  Philox-4x32-10 with counter
 * = (first_ray + r, stream) and key = seed; `stream` is typically the step
 * number, first_ray the global index of this shard's first ray.  The same
 * (ray, stream, seed) gives the same words on any rank.  turtle_amd_philox_n
 * exposes the raw 4 x 32-bit blocks (for known-answer tests). */
TURTLE_API enum turtle_return turtle_amd_isotropic_n(long n,
    unsigned long long seed, unsigned long long stream, long first_ray,
    double * direction /* [n][3] */, int space);
TURTLE_API enum turtle_return turtle_amd_philox_n(long n,
    unsigned long long seed, unsigned long long stream, long first_ray,
    unsigned int * words /* [n][4] */, int space);

#ifdef __cplusplus
}
#endif
#endif
