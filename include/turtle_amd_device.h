/*
 * turtle_amd_device.h -- the stepper of libturtle_amd as DEVICE functions: step rays inside
 * your own kernel.  HIP C++ for gfx950 (CDNA4, wave64); include it from a .hip file compiled
 * with hipcc --offload-arch=gfx950 -ffp-contract=off (the STRICT arithmetic reproduces the
 * reference's roundings: a fused multiply-add across them changes bits).  It needs nothing but
 * this directory on the include path.  The library's own kernels (the .hip files of turtle_amd/csrc)
 * include this same file: there is one source of the arithmetic.
 *
 * The shape of a caller (examples/own_kernel.hip is a complete one):
 *
 *     host:   turtle_amd_view view;
 *             turtle_amd_stepper_view_acquire(stepper, &view, sizeof(view));   // turtle_amd.h
 *             turtle_amd_device::dispatch(view, [&](auto mode) {
 *                     my_kernel<decltype(mode)::value><<<grid, 256, 0, stream>>>(view, ...); });
 *             hipStreamSynchronize(stream);
 *             turtle_amd_stepper_view_release(stepper);
 *
 *     device: template <int MODE> __global__ void my_kernel(turtle_amd_view view, ...)
 *             {
 *                     using namespace turtle_amd_device;
 *                     const Geometry<MODE, FAST> geo(view);   // once, at the top
 *                     Stepping<MODE, FAST> ray;
 *                     ray.start(position, direction);
 *                     for (int trips = 0; __ballot(ray.live) && (trips < limit); trips++) {
 *                             const int event = ray.trip(geo);   // ONE sample, full exec mask
 *                             if (event != NONE) my_physics(ray, event);   // may redirect() or stop()
 *                     }
 *             }
 *
 * Three levels, all templated on the kernel mode of the view (view.geometry.mode: what
 * dispatch() turns into a constant, as the library's launchers do) and on the arithmetic
 * (FAST / STRICT, the two values of turtle_amd_math_set):
 *   sample()   turtle_stepper_step(..., direction = NULL, ...): the layers at a position;
 *   step()     one whole turtle_stepper_step with a direction, the crossing halved in place:
 *              simple and divergent, for a loop ported first and tuned later;
 *   Stepping   the library's own idiom: trip() evaluates exactly one sample per live lane,
 *              whatever the ray is doing, and reports events.  k_walk's and k_traverse's
 *              inner block, lifted out.
 * and isotropic(), the Philox direction of turtle_amd_isotropic_n / turtle_stepper_scatter_n,
 * and normal(), one point of turtle_stepper_normal_n: the normal of the surface a ray crossed.
 *
 * What the functions assume: wave64, and trip() called from converged code (it predicates on
 * `live` itself).  They use no LDS, no global state and no atomics.  Paging is not offered on
 * the device side: turtle_amd_stepper_view_acquire makes every tile resident, or fails.  The
 * samples are the closed form of the transform (as k_walk's and k_traverse's); the lined samples
 * of a whole trace stay the library's own.  Names that begin with d_, f_, k or tamd_ are the
 * library's internals: they are here because its kernels are built from them, and may change
 * with TURTLE_AMD_VIEW_VERSION.  Citations [ref FILE:LINE] are paths under the reference tree.
 */
#ifndef TURTLE_AMD_DEVICE_H
#define TURTLE_AMD_DEVICE_H

#include <stddef.h>
#include <stdint.h>

/* ------------------------------------------------------------------------ */
/* POD tables read by the kernels (layout shared by host and device code)   */
/* ------------------------------------------------------------------------ */

/* One DEM grid resident in HBM: 16-bit nodes, native little-endian, in BLOCKS
 * of 8 x 8 nodes (128 bytes, one cache line; rows south->north inside a block
 * and from block to block, nbx blocks per block row, the grid padded to whole
 * blocks): node (ix, iy) is at ((iy / 8) * nbx + ix / 8) * 64 + (iy % 8) * 8 +
 * ix % 8.  A sample reads the 2 x 2 nodes of a cell; in rows of nx nodes those
 * are two lines 2 nx bytes apart, in blocks one line three times out of four,
 * and the next cells of the ray -- whichever way it heads -- are in it too.
 * Decoding the file format (byte order, row flip, sign) happens ONCE at upload
 * instead of per node access as the reference's get_z callbacks do [ref
 * src/turtle/map.h:47-49, io/hgt.c:127-131, map.c:41-44]; integers are exact,
 * so parity is unaffected.  z = z0 + v * dz with v read as int16 if is_signed
 * else uint16 (signed codecs use z0 = 0, dz = 1, which reproduces "(int16)v"
 * exactly). */
#define TAMD_BLOCK 8
/* A map projection [ref src/turtle/projection.h:29-46]; type < 0: geodetic */
enum tamd_proj_type { TAMD_PROJ_NONE = -1, TAMD_PROJ_LAMBERT = 0, TAMD_PROJ_UTM = 1 };

struct tamd_proj {
        int type;           /* enum tamd_proj_type */
        int lambert_tag;    /* 0..5: I, II, IIe, III, IV, 93 */
        double longitude_0; /* UTM central meridian, degrees */
        int hemisphere;     /* UTM: +1 north, -1 south */
        int pad_;
};

struct tamd_grid {
        const uint16_t * nodes;
        int nx, ny;
        double x0, y0, dx, dy;
        double z0, dz;
        double inv_dx, inv_dy; /* 1/dx, 1/dy: the fast-math kernels multiply */
        int is_signed;
        int nbx; /* blocks of TAMD_BLOCK x TAMD_BLOCK nodes per block row */
        struct tamd_proj proj; /* x, y of a projected map; the stepper projects
                                * (latitude, longitude) first [ref stepper.c:243-248] */
};

/* Tile directory of a stack [ref src/turtle/stack.h:32-49]: O(1) lookup
 * replaces the reference's MRU list scan [ref stack.c:300-335]. */
struct tamd_stack {
        double lat0, lon0, dlat, dlon;
        double inv_dlat, inv_dlon; /* the fast-math lookup multiplies (seams: exact) */
        int nlat, nlon;
        int tile_first; /* offset into the tiles[] table: grid index or -1 */
        /* `regular`: every tile present has the same shape and encoding (nx,
         * ny, dx, dy, z0, dz, sign) and sits exactly on the lattice (x0 ==
         * lon0 + ix*dlon, y0 == lat0 + iy*dlat) whose cell it spans ((nx-1) dx
         * == dlon up to rounding), as SRTM/ASTER tiles do.  The
         * fast-math kernels then need one pointer per tile (slot_nodes[
         * nodes_first + slot], NULL for a missing tile) instead of a whole
         * per-lane grid descriptor; `proto` holds the shared shape. */
        int regular;
        int nodes_first, pad_;
        struct tamd_grid proto;
};

enum tamd_kind { TAMD_FLAT = 0, TAMD_MAP = 1, TAMD_STACK = 2 };

/* values of the tile table (tamd_view.tiles) besides a grid index */
#define TAMD_TILE_NONE (-1)  /* no file for this slot */
#define TAMD_TILE_PAGED (-2) /* a file, not resident: see "Paging" in csrc/device_common.h */

/* One (data, offset) entry of a layer [ref src/turtle/stepper.h:80-85], stored
 * in the reference's iteration order: last added first [ref stepper.c:722-724] */
struct tamd_meta {
        int kind; /* enum tamd_kind */
        int src;  /* grid index (MAP) or stack index (STACK) */
        double offset;
};

enum tamd_mode {
        TAMD_MODE_GENERIC = 0,   /* any layers / data / geoid */
        TAMD_MODE_ONE_MAP = 1,   /* one layer, one geodetic map, no geoid */
        TAMD_MODE_ONE_STACK = 2  /* one layer, one stack, no geoid */
};

/* Everything a kernel needs about a stepper, passed BY VALUE as a kernel
 * argument so that it sits in scalar registers. */
struct tamd_view {
        const struct tamd_grid * grids;
        const struct tamd_stack * stacks;
        const int * tiles;
        const uint16_t * const * slot_nodes; /* see tamd_stack.regular */
        const struct tamd_meta * metas;
        const int * layer_first; /* n_layers + 1 offsets into metas */
        int n_layers;
        int geoid; /* grid index or -1 */
        double slope, resolution;
        int mode; /* enum tamd_mode */
        int fast_ok; /* every grid has nx, ny >= 2: the clamped fast lookup applies */
};

/* The stepper's geometry as turtle_amd_stepper_view_acquire lends it: a POD, passed to a kernel
 * BY VALUE (it then sits in scalar registers).  `version` and `size` are filled by the library
 * and checked by turtle_amd_view_ok() against this header's: that is the whole compatibility
 * promise.  It names resident tiles only, and stays good until the release. */
#define TURTLE_AMD_VIEW_VERSION 1
struct turtle_amd_view {
        struct tamd_view geometry;
        int version; /* TURTLE_AMD_VIEW_VERSION of the library that filled it */
        int size;    /* its sizeof(struct turtle_amd_view) */
};
#ifdef __cplusplus
typedef struct turtle_amd_view turtle_amd_view;
#endif

__attribute__((unused)) static inline int turtle_amd_view_ok(const struct turtle_amd_view * view)
{
        return (view->version == TURTLE_AMD_VIEW_VERSION) && (view->size == (int)sizeof(struct turtle_amd_view));
}

/* struct turtle_amd_grid (turtle_amd.h) as a kernel reads it: a POD, passed BY VALUE like the view
 * (the scalars then sit in scalar registers); `density` is a DEVICE pointer to n[2] x n[1] x n[0]
 * voxels, axis 0 fastest.  The argument of turtle_amd_device::grid_depth below. */
struct turtle_amd_grid_view {
        double origin[3];
        double axis[3][3];
        double size[3];
        int n[3];
        int medium;
        const double * density;
};
#ifdef __cplusplus
typedef struct turtle_amd_grid_view turtle_amd_grid_view;
#endif

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include <cfloat>
#include <type_traits>
#include <utility>

namespace turtle_amd_device {

/* (the bookkeeping of a sample is written with & and | on booleans on purpose: selects, not branches) */
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wbitwise-instead-of-logical"

typedef unsigned long long ull;

/* Node arrays live in HBM.  Pointers that reach a kernel inside a descriptor
 * table are generic as far as the compiler can tell, and a generic load is a
 * flat_load (slower, and it ties up both memory counters): say "global". */
typedef const __attribute__((address_space(1))) uint16_t * global_nodes_t;
#define GLOBAL_NODES(p) ((global_nodes_t)(p))

/* ======================================================================== */
/*                               device math                                */
/* ======================================================================== */


constexpr double kPi = 3.14159265358979323846; /* [ref ecef.c:30-33] */
constexpr double kA = 6378137;                 /* [ref ecef.c:36-38] */
constexpr double kB = 6356752.3142;
constexpr double kE = 0.081819190842622;

/* [ref ecef.c:41-55] */
__device__ __forceinline__ void d_from_geodetic(
    double latitude, double longitude, double elevation, double & x, double & y, double & z)
{
        const double a = kA, e = kE;
        const double s = sin(latitude * kPi / 180.);
        const double c = cos(latitude * kPi / 180.);
        const double R = a / sqrt(1. - e * e * s * s);
        x = (R + elevation) * c * cos(longitude * kPi / 180.);
        y = (R + elevation) * c * sin(longitude * kPi / 180.);
        z = (R * (1. - e * e) + elevation) * s;
}

/* [ref ecef.c:63-130] Olson (1996) closed form.  All three outputs are always
 * produced (the pointer-null shortcuts of the scalar API live on the host). */
__device__ __forceinline__ void d_to_geodetic(
    double x, double y, double z, double & latitude, double & longitude, double & altitude)
{
        const double a = kA;
        const double e2 = kE * kE;
        const double a1 = a * e2;
        const double a2 = a1 * a1;
        const double a3 = 0.5 * a1 * e2;
        const double a4 = 2.5 * a2;
        const double a5 = a1 + a3;
        const double a6 = 1. - e2;

        if ((x == 0.) && (y == 0.)) { /* [ref ecef.c:77-84] */
                latitude = (z >= 0.) ? 90. : -90.;
                longitude = 0.;
                altitude = fabs(z) - kB;
                return;
        }

        longitude = atan2(y, x) * 180. / kPi;

        const double zp = fabs(z);
        const double w2 = x * x + y * y;
        const double w = sqrt(w2);
        const double z2 = z * z;
        const double r2 = w2 + z2;
        const double r = sqrt(r2);
        const double s2 = z2 / r2;
        const double c2 = w2 / r2;

        double c, s, ss, la;
        const double u0 = a2 / r;
        const double v0 = a3 - a4 / r;
        if (c2 > 0.3) { /* [ref ecef.c:101-107] */
                s = (zp / r) * (1. + c2 * (a1 + u0 + s2 * v0) / r);
                la = asin(s);
                ss = s * s;
                c = sqrt(1. - ss);
        } else { /* [ref ecef.c:108-115] */
                c = (w / r) * (1. - s2 * (a5 - u0 - c2 * v0) / r);
                la = acos(c);
                ss = 1. - c * c;
                s = sqrt(ss);
        }

        const double g = 1. - e2 * ss; /* [ref ecef.c:117-129] */
        const double rg = a / sqrt(g);
        const double rf = a6 * rg;
        const double u = w - rg * c;
        const double v = zp - rf * s;
        const double f = c * u + s * v;
        const double m = c * v - s * u;
        const double p = m / (rf / g + f);

        la += p;
        if (z < 0.) la = -la;
        latitude = la * 180. / kPi;
        altitude = f + 0.5 * m * p;
}

/* [ref ecef.c:136-154] */
__device__ __forceinline__ void d_enu(
    double latitude, double longitude, double e[3], double n[3], double u[3])
{
        const double lambda = longitude * kPi / 180.;
        const double phi = latitude * kPi / 180.;
        const double sl = sin(lambda), cl = cos(lambda);
        const double sp = sin(phi), cp = cos(phi);
        e[0] = -sl, e[1] = cl, e[2] = 0.;
        n[0] = -cl * sp, n[1] = -sl * sp, n[2] = cp;
        u[0] = cl * cp, u[1] = sl * cp, u[2] = sp;
}

/* ---- fast-math variant of the transform ----------------------------------
 *
 * Same algorithm (Olson 1996, [ref ecef.c:63-130]), leaner arithmetic: the ten
 * divisions become reciprocals shared between terms, sqrt/rsqrt pairs come
 * from one v_rsq_f64 seed with two Goldschmidt steps, asin/acos/atan2 become
 * one first-octant arctangent (3 sectors of half-width pi/16, one division,
 * degree-8 minimax polynomial in t^2, error < 1e-19), and FMAs are used freely.
 * Each primitive is good to ~1 ulp, so latitude/longitude/altitude differ from
 * the strict evaluation by a few ulp (<= 3e-9 m in altitude, <= 1e-13 deg):
 * the same order as the OCML-vs-glibc differences of the strict path and four
 * orders of magnitude inside the 1e-6 parity bar.  tests/test_gpu_parity.py
 * checks both variants against the reference's golden vectors.
 *
 * Why it exists: the trace kernel's run time on the 1 M-ray workload is the
 * latency of its longest ray (11 327 sequential samples), i.e. proportional to
 * the instruction count of ONE sample, and its throughput on larger batches is
 * fp64-VALU bound.  This variant needs ~3x fewer instructions per sample. */

__device__ __forceinline__ double f_rcp(double a)
{
        double y = __builtin_amdgcn_rcp(a);
        double e = __builtin_fma(-a, y, 1.);
        y = __builtin_fma(y, e, y);
        e = __builtin_fma(-a, y, 1.);
        return __builtin_fma(y, e, y);
}

/* sqrt(a) and 1/sqrt(a) for a normal, positive a (no denormal scaling) */
__device__ __forceinline__ void f_sqrt_rsqrt(double a, double & root, double & inverse)
{
        const double y = __builtin_amdgcn_rsq(a);
        double g = a * y, h = 0.5 * y;
        double r = __builtin_fma(-h, g, 0.5);
        g = __builtin_fma(g, r, g);
        h = __builtin_fma(h, r, h);
        r = __builtin_fma(-h, g, 0.5);
        g = __builtin_fma(g, r, g);
        h = __builtin_fma(h, r, h);
        /* one correction of the root: g += (a - g*g) * h */
        const double d = __builtin_fma(-g, g, a);
        root = __builtin_fma(d, h, g);
        inverse = h + h;
}

/* atan(y / x) for 0 <= y <= x, x > 0: result in [0, pi/4] */
__device__ __forceinline__ double f_atan_octant(double y, double x)
{
        const bool s1 = y > x * 0.198912367379658;  /* tan(pi/16) */
        const bool s2 = y > x * 0.6681786379192989; /* tan(3pi/16) */
        const double tk = s2 ? 1. : (s1 ? 0.41421356237309503 : 0.);
        const double th = s2 ? 0.7853981633974483 : (s1 ? 0.39269908169872414 : 0.);
        const double num = __builtin_fma(-x, tk, y);
        const double den = __builtin_fma(y, tk, x);
        const double rd = f_rcp(den);
        double t = num * rd;
        t = __builtin_fma(__builtin_fma(-den, t, num), rd, t);
        const double u = t * t;
        double q = 0.050273062752334695;
        q = __builtin_fma(q, u, -0.0660516727229625);
        q = __builtin_fma(q, u, 0.0768988435768423);
        q = __builtin_fma(q, u, -0.0909085307967067);
        q = __builtin_fma(q, u, 0.11111110348139375);
        q = __builtin_fma(q, u, -0.14285714279864764);
        q = __builtin_fma(q, u, 0.19999999999977505);
        q = __builtin_fma(q, u, -0.333333333333333);
        return th + __builtin_fma(t * u, q, t);
}

/* atan2 for s >= 0, c >= 0 (not both 0): result in [0, pi/2] */
__device__ __forceinline__ double f_atan2_q1(double s, double c)
{
        const bool swap = s > c;
        const double a = f_atan_octant(swap ? c : s, swap ? s : c);
        return swap ? 1.5707963267948966 - a : a;
}

__device__ __forceinline__ double f_atan2(double y, double x)
{
        const double ax = fabs(x), ay = fabs(y);
        double a = f_atan2_q1(ay, ax);
        if (x < 0.) a = 3.141592653589793 - a;
        return copysign(a, y);
}

/* ---- a ray's geodetic coordinates as cubics in its path length -----------
 *
 * Along a straight ray q(s) = O + d s the latitude, longitude and altitude are
 * smooth functions of the scalar s, and their Taylor series at O follow from
 * the transform itself.  With (E, N, U) the components of the (constant)
 * direction in the East-North-Up frame of the moving point, M and N' the
 * meridional and prime-vertical radii,
 *     lat' = N / (M + h)      lon' = E / ((N' + h) cos lat)      h' = U
 *     E' = lon' (N sin lat - U cos lat)
 *     N' = -lat' U - lon' E sin lat        U' = lat' N + lon' E cos lat
 * and differentiating twice more gives the second and third derivatives in
 * closed form (~130 flops, no transcendental: the sines and cosines are at
 * hand in the closed-form transform of O).  The neglected term is c4 s^4 with
 * c4 <= 1e-21 (1 + tan^3 lat) m^-3 -- measured against a 40-digit evaluation
 * of the transform, latitudes to 89.5 degrees, any direction, h <= 9 km; at
 * latitude 45: 2.5e-13 m at 100 m, 1.6e-10 m at 500 m, 2.5e-9 m at 1 km.  For
 * comparison the reference's own local approximation (first order,
 * finite-difference Jacobian, 1 m range, [ref stepper.c:85-171]) is off by
 * 8e-8 m.
 *
 * A sample on the line costs 9 FMAs instead of the ~230 instructions of the
 * closed form; in phase B (rays skimming the ground with ~0.5 m steps) a line
 * serves ~1000 samples.  Whether a sample comes from the line depends on the
 * ray alone (its own line and path parameter), never on its wave. */
constexpr double kLineRange = 4000.; /* m, either side of the origin: hard limit */
/* The truncation a line is allowed near a boundary: a third of the closed form's own
 * rounding noise there (3e-9 m).  Rounds 1 and 2 allowed 2e-10 m; at 1e-9 m a line
 * reaches 1.5 x as far (5^(1/4): 760 m at latitude 45) and a ray takes a third fewer
 * closed forms (round 3, measured: C2 4.17 -> 4.05 ms, C4 30.2 -> 28.8; 3e-9 and 1e-8
 * bring no more, the million rays of C2 against the CPU restatement the same 0 / 0,
 * worst path length 2.1e-8 against 1.6e-8). */
#ifndef LINE_TOLERANCE
#define LINE_TOLERANCE 1e-9
#endif
#ifndef LINE_TAU0
#define LINE_TAU0 2e-9
#endif
constexpr double kLineTolerance = LINE_TOLERANCE; /* see f_line_serves */
/* what a lean step counts a clearance as, at most: with k4 <= kLineTolerance / 1.8e-21 (the
 * equator) a sample that passes its reach test is then inside kLineRange as well */
constexpr double kLeanClearance = 400.;
static_assert(kLineTolerance / 1.8e-21 * kLeanClearance < kLineRange * kLineRange * kLineRange * kLineRange,
    "a lean step's reach test must imply the line's hard limit");
/* A ray's position is ACCUMULATED step by step, B += d * ds with the reference's
 * roundings [ref stepper.c:824, :862-863], in every phase: each step leaves B
 * up to half an ulp of 6.4e6 m per coordinate (8e-10 m) off the straight line,
 * mostly the same way from step to step (a skimming ray adds the same increment
 * thousands of times: 2.7e-6 m measured over the 11 326 steps of C2's longest
 * ray) -- and the reference decides on ITS positions.  The line is a function of
 * the path length alone, so a sample taken from it answers for the ideal point
 * O + d * s, which is off the reference's by that drift.  That is harmless where
 * it only sizes the next step, and decisive where the medium is decided within
 * the drift of the boundary (a ray tangent to the ground: one step more or
 * less is 1e-2 m of path; with positions kept ON the line, as round 1 had them,
 * 1 ray of C2's million ended a step early, 1.6e-6 of its path, and the others
 * were within 2e-7 instead of 5e-9).  So the line keeps count of what its
 * truncation and the drift since it was laid can amount to (tau: kLineTau0 at
 * the origin + kLineDrift per accepted step), and a sample whose clearance is
 * not above it is taken again by the closed form AT THE ACCUMULATED POSITION, as
 * phase A would -- which lays a new line there, whose drift starts from nothing
 * (the samples of a bisection all leave from one accumulated position: the line
 * laid at the first of them that is too close to call serves the others -- ALL
 * the others (`bracketed`): it has no drift, and the last halvings of every ray
 * are within 1e-9 m of the ground, where its truncation (kLineTolerance) is below
 * the closed form's own noise.) */
constexpr double kLineTau0 = LINE_TAU0;  /* m: the truncation allowed near a boundary (1e-9 m) and
                                     * the rounding of latitude and longitude (8e-10 m on the
                                     * ground, a third of that in elevation) */
[[maybe_unused]] constexpr double kLineDrift = 1e-9; /* m per step: (3 x (2^-31)^2)^0.5 = 8.1e-10 rounded up */

struct RayLine {
        double s;                /* path parameter of the ray's position B */
        double lat[4], lon[4], alt[4]; /* degrees, degrees, metres; [k]: s^k */
        double k4;               /* kLineTolerance / c4, c4 s^4 metres bounding the neglected term */
        double tau;
        bool valid;
};

/* Is the line good enough for a sample at parameter s that came out at
 * `clearance` metres from the nearest boundary?  The truncation error must be
 * below kLineTolerance = 1e-9 m (a third of the closed form's own rounding noise)
 * -- or, far from any boundary, below 1e-9 OF the clearance: all such a sample
 * decides is the length of the next step, to the same relative accuracy.  At
 * latitude 45 this lets a line serve 760 m near the ground and ~3 km in free flight. */
__device__ __forceinline__ bool f_line_serves(const RayLine & L, double s, double clearance,
    bool bracketed = false)
{
        const double s2 = s * s;
        return (s2 * s2 <= L.k4 * fmax(clearance, 1.)) &
            ((bracketed & (L.tau <= kLineTau0)) | (clearance > L.tau));
}

__device__ __forceinline__ void f_line_eval(const RayLine & L, double s, double & latitude,
    double & longitude, double & altitude)
{
        latitude = __builtin_fma(
            s, __builtin_fma(s, __builtin_fma(s, L.lat[3], L.lat[2]), L.lat[1]), L.lat[0]);
        longitude = __builtin_fma(
            s, __builtin_fma(s, __builtin_fma(s, L.lon[3], L.lon[2]), L.lon[1]), L.lon[0]);
        altitude = __builtin_fma(
            s, __builtin_fma(s, __builtin_fma(s, L.alt[3], L.alt[2]), L.alt[1]), L.alt[0]);
}

/* The series at a point whose transform is known: S, C = sin, cos of its
 * latitude; sl, cl of its longitude; rn = N', rm = M; iw2 = 1 / (1 - e2 S^2). */
__device__ __forceinline__ void f_line_build(RayLine & L, double latitude, double longitude,
    double h, double S, double C, double sl, double cl, double rn, double rm, double iw2,
    double dx, double dy, double dz)
{
        constexpr double kRad2Deg = 57.29577951308232;
        const double e2 = kE * kE;
        /* the direction in the local frame */
        const double a = __builtin_fma(cl, dx, sl * dy);
        const double E = __builtin_fma(cl, dy, -(sl * dx));
        const double N = __builtin_fma(C, dz, -(S * a));
        const double U = __builtin_fma(C, a, S * dz);
        /* the radii and their first two derivatives in latitude */
        const double SC = S * C;
        const double k = e2 * SC * iw2;
        const double k1 = e2 * iw2 * ((C * C - S * S) + 2. * e2 * SC * SC * iw2);
        const double rn1 = rn * k, rm1 = 3. * rm * k;
        const double rn2 = __builtin_fma(rn1, k, rn * k1);
        const double rm2 = 3. * __builtin_fma(rm1, k, rm * k1);
        const double re = rn + h;
        const double rho = f_rcp(rm + h), nu = f_rcp(re * C);
        /* first derivatives */
        const double p1 = N * rho, l1 = E * nu, h1 = U;
        const double SNCU = __builtin_fma(S, N, -(C * U));
        const double E1 = l1 * SNCU;
        const double N1 = -(p1 * U) - l1 * S * E;
        const double U1 = __builtin_fma(p1, N, l1 * C * E);
        /* second */
        const double f = __builtin_fma(rm1, p1, h1);       /* (M + h)' */
        const double rho1 = -(rho * rho) * f;
        const double gq = __builtin_fma(rn1, p1, h1);
        const double g = gq * C - re * S * p1;             /* ((N' + h) cos lat)' */
        const double nu1 = -(nu * nu) * g;
        const double p2 = __builtin_fma(N1, rho, N * rho1);
        const double l2 = __builtin_fma(E1, nu, E * nu1);
        const double h2 = U1;
        const double E2 = l2 * SNCU + l1 * (C * p1 * N + S * N1 + S * p1 * U - C * U1);
        const double N2 = -(p2 * U) - p1 * U1 - l2 * S * E - l1 * C * p1 * E - l1 * S * E1;
        const double U2 = p2 * N + p1 * N1 + l2 * C * E - l1 * S * p1 * E + l1 * C * E1;
        /* third */
        const double f1 = rm2 * p1 * p1 + rm1 * p2 + h2;
        const double rho2 = 2. * rho * rho * rho * f * f - rho * rho * f1;
        const double g1 = (rn2 * p1 * p1 + rn1 * p2 + h2) * C - 2. * gq * S * p1 -
            re * C * p1 * p1 - re * S * p2;
        const double nu2 = 2. * nu * nu * nu * g * g - nu * nu * g1;
        const double p3 = N2 * rho + 2. * N1 * rho1 + N * rho2;
        const double l3 = E2 * nu + 2. * E1 * nu1 + E * nu2;
        const double h3 = U2;

        L.lat[0] = latitude, L.lat[1] = kRad2Deg * p1;
        L.lat[2] = (0.5 * kRad2Deg) * p2, L.lat[3] = (kRad2Deg / 6.) * p3;
        L.lon[0] = longitude, L.lon[1] = kRad2Deg * l1;
        L.lon[2] = (0.5 * kRad2Deg) * l2, L.lon[3] = (kRad2Deg / 6.) * l3;
        L.alt[0] = h, L.alt[1] = h1, L.alt[2] = 0.5 * h2, L.alt[3] = h3 * (1. / 6.);
        L.s = 0.;
        L.tau = kLineTau0;
        /* measured (40-digit reference, any direction, h <= 9 km): the
         * fourth-order term is within 1e-21 (1 + tan^3 lat) s^4 metres */
        const double tl = fabs(S) * nu * re;
        L.k4 = kLineTolerance / (1.2e-21 * __builtin_fma(tl * tl, tl, 1.5));
        /* not near a pole (1 / cos lat), nor where the longitude wraps; and only
         * where the bound above was measured: s is a LENGTH (a unit direction;
         * the reference steps along any vector, and so does the closed form that
         * a ray without a valid line keeps using), not deep inside the Earth
         * (1 / (M + h)).  NaNs fail every test. */
        const double dd = __builtin_fma(dx, dx, __builtin_fma(dy, dy, dz * dz));
        L.valid = (C > 1e-3) & (fabs(longitude) < 179.9) & (fabs(dd - 1.) < 1e-6) & (h > -1e5);
}

__device__ __forceinline__ void f_to_geodetic(double x, double y, double z,
    double & latitude, double & longitude, double & altitude, RayLine * build = nullptr,
    double dx = 0., double dy = 0., double dz = 0.)
{
        constexpr double kRad2Deg = 57.29577951308232;
        const double a = kA;
        const double e2 = kE * kE;
        const double a1 = a * e2;
        const double a2 = a1 * a1;
        const double a3 = 0.5 * a1 * e2;
        const double a4 = 2.5 * a2;
        const double a5 = a1 + a3;
        const double a6 = 1. - e2;

        if ((x == 0.) && (y == 0.)) { /* [ref ecef.c:77-84] */
                latitude = (z >= 0.) ? 90. : -90.;
                longitude = 0.;
                altitude = fabs(z) - kB;
                if (build != nullptr) build->valid = false;
                return;
        }

        longitude = f_atan2(y, x) * kRad2Deg;

        const double zp = fabs(z);
        const double w2 = __builtin_fma(x, x, y * y);
        const double z2 = z * z;
        const double r2 = w2 + z2;
        double r, ir, w, iw;
        f_sqrt_rsqrt(r2, r, ir);
        f_sqrt_rsqrt(w2, w, iw);
        if (w2 == 0.) w = 0.; /* x*x + y*y underflowed: on the axis to within 1e-162 m */
        const double ir2 = ir * ir;
        const double s2 = z2 * ir2;
        const double c2 = w2 * ir2;
        const double u0 = a2 * ir;
        const double v0 = __builtin_fma(-a4, ir, a3);

        /* [ref ecef.c:101-115] both seeds are cheap; selecting instead of
         * branching keeps the wave converged whatever the latitudes */
        const double s_seed = (zp * ir) * __builtin_fma(c2 * (a1 + u0 + s2 * v0), ir, 1.);
        const double c_seed = (w * ir) * __builtin_fma(-s2 * (a5 - u0 - c2 * v0), ir, 1.);
        const bool low = c2 > 0.3; /* |latitude| below ~56.8 deg: seed the sine */
        const double seed = low ? s_seed : c_seed;
        const double ss = low ? seed * seed : __builtin_fma(-seed, seed, 1.);
        double other, unused;
        f_sqrt_rsqrt(low ? 1. - ss : ss, other, unused);
        const double s = low ? seed : other;
        const double c = low ? other : seed;
        double la = f_atan2_q1(s, c);

        const double g = __builtin_fma(-e2, ss, 1.); /* [ref ecef.c:117-129] */
        double sg, isg;
        f_sqrt_rsqrt(g, sg, isg);
        const double rg = a * isg;
        const double rf = a6 * rg;
        const double u = __builtin_fma(-rg, c, w);
        const double v = __builtin_fma(-rf, s, zp);
        const double f = __builtin_fma(c, u, s * v);
        const double m = __builtin_fma(c, v, -(s * u));
        const double p = m * f_rcp(__builtin_fma(rf * isg, isg, f));
        (void)sg;

        la += p;
        if (z < 0.) la = -la;
        latitude = la * kRad2Deg;
        altitude = __builtin_fma(0.5 * m, p, f);

        if (build != nullptr) { /* everything it needs is at hand */
                /* sine and cosine of the corrected latitude, and the radii there:
                 * p is ~4e-8 rad, which the radii of the seed would turn into
                 * 4e-10 of the distance along the line (2e-7 m at 500 m) */
                const double sf = __builtin_fma(c, p, s), cf = __builtin_fma(-s, p, c);
                double sw, isw;
                f_sqrt_rsqrt(__builtin_fma(-e2 * sf, sf, 1.), sw, isw);
                (void)sw;
                const double isw2 = isw * isw, rn = a * isw;
                f_line_build(*build, latitude, longitude, altitude, (z < 0.) ? -sf : sf, cf,
                    y * iw, x * iw, rn, a6 * rn * isw2, isw2, dx, dy, dz);
                build->valid = build->valid & (w2 != 0.);
        }
}

/* ---- map projections ------------------------------------------------------ */

/* [ref projection.c:329-349]: e, n, c, lambda_c, xs, ys of Lambert I, II, IIe,
 * III, IV (NTG_71) and Lambert 93 (RGF93) */
static __constant__ double kLambert[6][6] = {
        { 0.08248325676, 0.7604059656, 11603796.98, 0.04079234433, 600000.0, 5657616.674 },
        { 0.08248325676, 0.7289686274, 11745793.39, 0.04079234433, 600000.0, 6199695.768 },
        { 0.08248325676, 0.7289686274, 11745793.39, 0.04079234433, 600000.0, 8199695.768 },
        { 0.08248325676, 0.6959127966, 11947992.52, 0.04079234433, 600000.0, 6791905.085 },
        { 0.08248325676, 0.6712679322, 12136281.99, 0.04079234433, 234.358, 7239161.542 },
        { 0.08181919112, 0.7253743710, 11755528.70, 0.05235987756, 700000.0, 12657560.145 }
};

/* [ref projection.c:192-210, :238-244, :286-295 (Lambert), :377-408 (UTM)].  The kernels
 * call d_project / d_unproject, out of line; k_resample, whose whole work they are, has the
 * bodies inlined (a call takes its outputs through scratch memory). */
/* TYPE: TAMD_PROJ_LAMBERT or _UTM when the caller knows it, else -2: decided by pr.type */
template <int TYPE = -2>
__device__ __forceinline__ void d_project_body(
    const tamd_proj & pr, double latitude, double longitude, double & x, double & y)
{
        if ((TYPE == TAMD_PROJ_LAMBERT) || ((TYPE != TAMD_PROJ_UTM) && (pr.type == TAMD_PROJ_LAMBERT))) {
                const double * P = kLambert[pr.lambert_tag];
                const double e = P[0];
                const double phi = latitude * kPi / 180.;
                const double s = sin(phi);
                const double L = log(tan(0.25 * kPi + 0.5 * phi) *
                    pow((1. - e * s) / (1. + e * s), 0.5 * e));
                const double cenL = P[2] * exp(-P[1] * L);
                const double lambda = longitude / 180. * kPi;
                const double theta = P[1] * (lambda - P[3]);
                x = P[4] + cenL * sin(theta);
                y = P[5] - cenL * cos(theta);
                return;
        }
        const double a = 6378.137E+03;
        const double f = 1. / 298.257223563;
        const double E0 = 5E+05;
        const double N0 = (pr.hemisphere > 0) ? 0. : 1E+07;
        const double k0 = 0.9996;
        const double n = f / (2. - f);
        const double A = a / (1. + n) * (1. + n * n * (0.25 + 0.0625 * n * n));
        const double alpha[3] = { n * (0.5 + n * (-2. / 3. + 5. / 16. * n)),
                n * n * (13. / 48. - 3. / 5. * n), 61. / 240. * n * n * n };
        const double c = 2. * sqrt(n) / (1. + n);
        const double s = sin(latitude * kPi / 180.);
        const double t = sinh(atanh(s) - c * atanh(c * s));
        const double dl = (longitude - pr.longitude_0) * kPi / 180.;
        const double zeta = atan2(t, cos(dl));
        const double eta = atanh(sin(dl) / sqrt(1. + t * t));
        double xs = 0., ys = 0.;
        for (int i = 0; i < 3; i++) {
                xs += alpha[i] * cos(2. * (i + 1) * zeta) * sinh(2. * (i + 1) * eta);
                ys += alpha[i] * sin(2. * (i + 1) * zeta) * cosh(2. * (i + 1) * eta);
        }
        x = E0 + k0 * A * (eta + xs);
        y = N0 + k0 * A * (zeta + ys);
}

__attribute__((unused)) static __device__ __noinline__ void d_project(
    const tamd_proj & pr, double latitude, double longitude, double & x, double & y)
{
        d_project_body(pr, latitude, longitude, x, y);
}

/* [ref projection.c:213-230, :253-268, :304-318 (Lambert), :417-448 (UTM)] */
template <int TYPE = -2>
__device__ __forceinline__ void d_unproject_body(
    const tamd_proj & pr, double x, double y, double & latitude, double & longitude)
{
        if ((TYPE == TAMD_PROJ_LAMBERT) || ((TYPE != TAMD_PROJ_UTM) && (pr.type == TAMD_PROJ_LAMBERT))) {
                const double * P = kLambert[pr.lambert_tag];
                const double e = P[0];
                const double dx = x - P[4];
                const double dy = y - P[5];
                const double R = sqrt(dx * dx + dy * dy);
                const double gamma = atan2(dx, -dy);
                longitude = (P[3] + gamma / P[1]) * 180. / kPi;
                const double L = -log(R / P[2]) / P[1];
                const double eL = exp(L);
                double phi0 = 2. * atan(eL) - 0.5 * kPi;
                for (int it = 0; it < 64; it++) { /* converges in 3-4 rounds */
                        const double s = sin(phi0);
                        const double phi1 =
                            2. * atan(pow((1. + e * s) / (1. - e * s), 0.5 * e) * eL) - 0.5 * kPi;
                        const bool stop = fabs(phi1 - phi0) <= (double)FLT_EPSILON;
                        phi0 = phi1;
                        if (stop) break;
                }
                latitude = phi0 / kPi * 180.;
                return;
        }
        const double a = 6378.137E+03;
        const double f = 1. / 298.257223563;
        const double E0 = 5E+05;
        const double N0 = (pr.hemisphere > 0) ? 0. : 1E+07;
        const double k0 = 0.9996;
        const double n = f / (2. - f);
        const double A = a / (1. + n) * (1. + n * n * (0.25 + 0.0625 * n * n));
        const double beta[3] = { n * (0.5 + n * (-2. / 3. + 37. / 96. * n)),
                n * n * (1. / 48. + 1. / 15. * n), 17. / 480. * n * n * n };
        const double delta[3] = { n * (2. + n * (-2. / 3. - 2. * n)),
                n * n * (7. / 3. - 8. / 5. * n), 56. / 15. * n * n * n };
        const double zeta0 = (y - N0) / (k0 * A);
        const double eta0 = (x - E0) / (k0 * A);
        double zeta = zeta0, eta = eta0;
        for (int i = 0; i < 3; i++) {
                zeta -= beta[i] * sin(2. * (i + 1) * zeta0) * cosh(2. * (i + 1) * eta0);
                eta -= beta[i] * cos(2. * (i + 1) * zeta0) * sinh(2. * (i + 1) * eta0);
        }
        const double chi = asin(sin(zeta) / cosh(eta));
        double s = 0.;
        for (int i = 0; i < 3; i++) s += delta[i] * sin(2. * (i + 1) * chi);
        latitude = (chi + s) * 180. / kPi;
        longitude = pr.longitude_0 + atan2(sinh(eta), cos(zeta)) * 180. / kPi;
}

__attribute__((unused)) static __device__ __noinline__ void d_unproject(
    const tamd_proj & pr, double x, double y, double & latitude, double & longitude)
{
        d_unproject_body(pr, x, y, latitude, longitude);
}

/* ---- one grid --------------------------------------------------------- */

/* Where node (ix, iy) sits in HBM: the grid is stored in blocks of 8 x 8 nodes
 * (128 bytes = one cache line: struct tamd_grid), so that the four nodes of a cell --
 * and the cells a ray visits next, whichever way it heads -- share a line far
 * more often than in rows of 7 KB. */
__device__ __forceinline__ unsigned d_node_index(int nbx, int ix, int iy)
{
        return (((unsigned)iy >> 3) * (unsigned)nbx + ((unsigned)ix >> 3)) * 64u +
            (((unsigned)iy & 7u) << 3) + ((unsigned)ix & 7u);
}

/* the four raw nodes of cell (ix, iy): lo = z00 | z10 << 16, hi = z01 | z11 << 16.
 * One index computation; the upper row is +8 inside a block, or a jump to the
 * next block row.  The two nodes of a row are neighbours in memory except in a
 * block's last column: one 32-bit load (2-byte aligned) fetches both, and only
 * the lanes in a last column (1 in 8) go back for the node of the next block.
 * Per wave that is ~144 line look-ups in the vector L1 instead of 256 -- the
 * gathers are most of what a batch of single steps asks of it.  (The pair load
 * never overruns the array: a cell's left-hand nodes have ix <= nx - 2, which
 * is never the last node of the last block.) */
typedef unsigned __attribute__((aligned(2))) u32_a2;
typedef const __attribute__((address_space(1))) u32_a2 * global_pair_t;

__device__ __forceinline__ void d_cell_fetch(
    const uint16_t * nodes, int nbx, int ix, int iy, unsigned & lo, unsigned & hi)
{
        global_nodes_t p = GLOBAL_NODES(nodes) + d_node_index(nbx, ix, iy);
        const unsigned up = (((unsigned)iy & 7u) == 7u) ? (unsigned)nbx * 64u - 56u : 8u;
        lo = *(global_pair_t)p, hi = *(global_pair_t)(p + up);
        if (((unsigned)ix & 7u) == 7u) { /* 64 - 7: the next block's first column */
                const unsigned z10 = p[57], z11 = p[up + 57];
                lo = (lo & 0xffffu) | (z10 << 16), hi = (hi & 0xffffu) | (z11 << 16);
        }
}

__device__ __forceinline__ double d_node(const tamd_grid & g, int ix, int iy)
{
        const uint16_t raw = GLOBAL_NODES(g.nodes)[d_node_index(g.nbx, ix, iy)];
        const double v = g.is_signed ? (double)(int16_t)raw : (double)raw;
        return g.z0 + v * g.dz; /* [ref map.c:41-44]; exact for z0=0, dz=1 */
}

/* [ref map.c:229-277]: inclusive upper edge, truncation toward zero, the
 * four-term sum in the reference's operand order. */
/* Last cell a lane looked up: its id and its four raw nodes.  A ray that
 * creeps along the surface (the long rays that set the run time of a launch)
 * stays in one 20-30 m cell for tens of steps; re-using the nodes takes the
 * gather out of its critical path. */
struct CellCache {
        unsigned id;     /* iy * nx + ix, or ~0u when empty */
        unsigned lo, hi; /* (z00 | z10 << 16), (z01 | z11 << 16), raw codes */
        /* regular stacks: the tile the last lookup fell in, and its nodes (saves the
         * dependent pointer load of every sample that stays in the tile) */
        int slot;
        const uint16_t * tile;
};

/* [ref map.c:229-277], fast-math form.  Differences from the strict form, none
 * of which changes an elevation by more than ~1e-12 m: (x - x0) is multiplied
 * by 1/dx instead of divided (except within 1e-6 cell of the rim, where the
 * exact quotient decides inside/outside as in the reference); the cell index is
 * clamped instead of special-cased (hx == nx-1 gives ix = nx-2, fx = 1 either
 * way); the two nodes of a row come from one unaligned 32-bit load. */
struct CellAt {
        double hx, hy; /* node coordinates of the point */
        int ix, iy;    /* its cell, clamped into the grid */
        unsigned id;   /* iy * nx + ix */
        bool inside;   /* [ref map.c:247-255], NaN => false */
        bool rim;      /* within 1e-6 cell of the rim: exact quotients were used */
};

__device__ __forceinline__ CellAt f_grid_locate(const tamd_grid & g, double x, double y)
{
        CellAt c;
        c.hx = (x - g.x0) * g.inv_dx;
        c.hy = (y - g.y0) * g.inv_dy;
        const double mx = (double)(g.nx - 1), my = (double)(g.ny - 1);
        c.rim = !((c.hx > 1e-6) && (c.hx < mx - 1e-6) && (c.hy > 1e-6) && (c.hy < my - 1e-6));
        if (__builtin_expect(c.rim, 0)) {
                c.hx = (x - g.x0) / g.dx;
                c.hy = (y - g.y0) / g.dy;
        }
        c.inside = (c.hx >= 0.) && (c.hx <= mx) && (c.hy >= 0.) && (c.hy <= my);
        c.ix = min(max((int)c.hx, 0), g.nx - 2);
        c.iy = min(max((int)c.hy, 0), g.ny - 2);
        c.id = (unsigned)c.iy * (unsigned)g.nx + (unsigned)c.ix;
        return c;
}

__device__ __forceinline__ unsigned d_upper_word(double x)
{
        return (unsigned)((unsigned long long)__double_as_longlong(x) >> 32);
}

/* The bilinear patch over a cell, fast-math form: z00 + fx b + fy (c + fx d) with
 * b = z10 - z00, c = z01 - z00, d = (z11 - z10) - c -- three fused operations
 * where the reference's four-term sum [ref map.c:270-276] takes thirteen, within
 * an ulp or two of it (1e-13 m).  The lean steps of the lined pass keep b, c, d
 * per cell. */
__device__ __forceinline__ double f_patch(double z00, double b, double c, double d, double fx, double fy)
{
        return __builtin_fma(fy, __builtin_fma(fx, d, c), __builtin_fma(fx, b, z00));
}

/* the bilinear blend of a cell's four raw nodes (lo = z00 | z10 << 16, hi =
 * z01 | z11 << 16); one function so that every caller rounds identically */
__device__ __forceinline__ double f_grid_blend(
    const tamd_grid & g, const CellAt & c, unsigned lo, unsigned hi)
{
        const double fx = c.hx - (double)c.ix, fy = c.hy - (double)c.iy;
        double z00, z10, z01, z11;
        if (g.is_signed) {
                z00 = (double)(int16_t)(lo & 0xffffu), z10 = (double)((int)lo >> 16);
                z01 = (double)(int16_t)(hi & 0xffffu), z11 = (double)((int)hi >> 16);
        } else {
                z00 = (double)(lo & 0xffffu), z10 = (double)(lo >> 16);
                z01 = (double)(hi & 0xffffu), z11 = (double)(hi >> 16);
        }
        z00 = __builtin_fma(z00, g.dz, g.z0), z10 = __builtin_fma(z10, g.dz, g.z0);
        z01 = __builtin_fma(z01, g.dz, g.z0), z11 = __builtin_fma(z11, g.dz, g.z0);
        return f_patch(z00, z10 - z00, z01 - z00, (z11 - z10) - (z01 - z00), fx, fy);
}

__device__ __forceinline__ bool f_grid_elevation(
    const tamd_grid & g, double x, double y, double & z, CellCache * cache = nullptr)
{
        const CellAt c = f_grid_locate(g, x, y);
        unsigned lo, hi;
        if ((cache != nullptr) && (cache->id == c.id)) {
                lo = cache->lo, hi = cache->hi;
        } else {
                d_cell_fetch(g.nodes, g.nbx, c.ix, c.iy, lo, hi);
                if (cache != nullptr) cache->id = c.id, cache->lo = lo, cache->hi = hi;
        }
        z = f_grid_blend(g, c, lo, hi);
        return c.inside;
}

/* [ref map.c:229-277]: inclusive upper edge, truncation toward zero, the
 * four-term sum in the reference's operand order. */
template <bool FAST = false>
__device__ __forceinline__ bool d_grid_elevation(
    const tamd_grid & g, double x, double y, double & z)
{
        if (FAST) return f_grid_elevation(g, x, y, z);
        if (isnan(x) || isnan(y)) return false; /* [ref map.c:233-240] */
        double hx = (x - g.x0) / g.dx;
        double hy = (y - g.y0) / g.dy;
        if ((hx > g.nx - 1) || (hx < 0) || (hy > g.ny - 1) || (hy < 0))
                return false; /* [ref map.c:247-255] */
        int ix = (int)hx;
        int iy = (int)hy;
        if (ix == g.nx - 1) { /* [ref map.c:256-265] */
                ix--;
                hx = 1.;
        } else
                hx -= ix;
        if (iy == g.ny - 1) {
                iy--;
                hy = 1.;
        } else
                hy -= iy;
        const double z00 = d_node(g, ix, iy);
        const double z10 = d_node(g, ix + 1, iy);
        const double z01 = d_node(g, ix, iy + 1);
        const double z11 = d_node(g, ix + 1, iy + 1);
        z = z00 * (1. - hx) * (1. - hy) + z01 * (1. - hx) * hy +
            z10 * hx * (1. - hy) + z11 * hx * hy; /* [ref map.c:272-273] */
        return true;
}

/* [ref map.c:280-378], as it is -- including the slip at map.c:352-353: for a
 * point in the grid's first half-row (iy == 0, hy <= 0.5) the y-gradient lands
 * in gx and gy is left untouched.  gx, gy are therefore in-out. */
/* SELECTS: which of gx, gy the first half-row writes is said with selects on the two values.
 * (Written as the reference's branches, the compiler merges the two stores into one store
 * through a selected ADDRESS, and gx, gy then live in scratch memory: 24 bytes a lane in
 * k_gradient, whose instruction stream is kept as it is.)  Same values either way. */
template <bool SELECTS = false>
__device__ __forceinline__ bool d_grid_gradient(
    const tamd_grid & g, double x, double y, double & gx, double & gy)
{
        if (isnan(x) || isnan(y)) return false;
        double hx = (x - g.x0) / g.dx;
        double hy = (y - g.y0) / g.dy;
        if ((hx > g.nx - 1) || (hx < 0) || (hy > g.ny - 1) || (hy < 0)) return false;
        int ix = (int)hx;
        int iy = (int)hy;
        if (ix == g.nx - 1) {
                ix--;
                hx = 1.;
        } else
                hx -= ix;
        if (iy == g.ny - 1) {
                iy--;
                hy = 1.;
        } else
                hy -= iy;
        const double z00 = d_node(g, ix, iy), z10 = d_node(g, ix + 1, iy);
        const double z01 = d_node(g, ix, iy + 1), z11 = d_node(g, ix + 1, iy + 1);

        if (hx <= 0.5) { /* [ref map.c:324-335] */
                const double gx1 = (z10 - z00) * (1. - hy) + (z11 - z01) * hy;
                if (ix == 0) {
                        gx = gx1 / g.dx;
                } else {
                        const double z_10 = d_node(g, ix - 1, iy), z_11 = d_node(g, ix - 1, iy + 1);
                        const double gx0 = (z00 - z_10) * (1. - hy) + (z01 - z_11) * hy;
                        const double ax = hx + 0.5;
                        gx = (gx0 * (1. - ax) + gx1 * ax) / g.dx;
                }
        } else { /* [ref map.c:336-348] */
                const double gx0 = (z10 - z00) * (1. - hy) + (z11 - z01) * hy;
                if (ix == g.nx - 2) {
                        gx = gx0 / g.dx;
                } else {
                        const double z20 = d_node(g, ix + 2, iy), z21 = d_node(g, ix + 2, iy + 1);
                        const double gx1 = (z20 - z10) * (1. - hy) + (z21 - z11) * hy;
                        const double ax = hx - 0.5;
                        gx = (gx0 * (1. - ax) + gx1 * ax) / g.dx;
                }
        }
        if (hy <= 0.5) { /* [ref map.c:350-361] */
                const double gy1 = (z01 - z00) * (1. - hx) + (z11 - z10) * hx;
                if (SELECTS) {
                        double q = gy1;
                        if (iy != 0) {
                                const double z0_1 = d_node(g, ix, iy - 1), z1_1 = d_node(g, ix + 1, iy - 1);
                                const double gy0 = (z00 - z0_1) * (1. - hx) + (z10 - z1_1) * hx;
                                const double ay = hy + 0.5;
                                q = gy0 * (1. - ay) + gy1 * ay;
                        }
                        q = q / g.dy;
                        gx = (iy == 0) ? q : gx, gy = (iy == 0) ? gy : q;
                } else if (iy == 0) {
                        gx = gy1 / g.dy; /* sic [ref map.c:353] */
                } else {
                        const double z0_1 = d_node(g, ix, iy - 1), z1_1 = d_node(g, ix + 1, iy - 1);
                        const double gy0 = (z00 - z0_1) * (1. - hx) + (z10 - z1_1) * hx;
                        const double ay = hy + 0.5;
                        gy = (gy0 * (1. - ay) + gy1 * ay) / g.dy;
                }
        } else { /* [ref map.c:362-374] */
                const double gy0 = (z01 - z00) * (1. - hx) + (z11 - z10) * hx;
                if (iy == g.ny - 2) {
                        gy = gy0 / g.dy;
                } else {
                        const double z02 = d_node(g, ix, iy + 2), z12 = d_node(g, ix + 1, iy + 2);
                        const double gy1 = (z02 - z01) * (1. - hx) + (z12 - z11) * hx;
                        const double ay = hy - 0.5;
                        gy = (gy0 * (1. - ay) + gy1 * ay) / g.dy;
                }
        }
        return true;
}

/* ---- tile directory --------------------------------------------------- */

/* half-open box of a resident tile [ref stack.c:307-311, :320-321] */
__device__ __forceinline__ bool d_tile_holds(
    const tamd_grid & g, double latitude, double longitude)
{
        const double hx = (longitude - g.x0) / g.dx;
        const double hy = (latitude - g.y0) / g.dy;
        return (hx >= 0.) && (hx < g.nx - 1) && (hy >= 0.) && (hy < g.ny - 1);
}

/* [ref stack.c:338-361] with every tile resident.  The reference scans its
 * tile list for the one whose half-open box holds the point and only then
 * falls back on the directory formula of turtle_stack_load_ [ref
 * stack.c:413-424], applying the inclusive bilinear test to that tile.  Here
 * the directory formula proposes the tile first (O(1)); its neighbours are
 * consulted only when rounding at a seam makes the box test disagree, which
 * reproduces the list scan's answer without the list. */
/* Paging.  A stack may hold more tiles than it keeps in HBM (its stack_size,
 * [ref stack.c:150, :434-443]).  In the tile table a tile that has a file but is
 * not resident reads TAMD_TILE_PAGED; a lookup that needs such a tile -- to
 * answer, or to decide a seam -- returns a FAULT code instead of a tile:
 * tile_fault(table index), any value below -1.  The kernels list the rays /
 * points that met one (page_fault), with the tiles they want; the host brings
 * those in (evicting the least recently wanted) and runs the list again. */
/* What a faulting lookup wants: tiles of the 3 x 3 neighbourhood of the
 * directory slot `centre` (an index into the tile table; -1: no fault); bit
 * 3 (j + 1) + (i + 1) of `mask` stands for the tile at centre + j * stride + i.
 * A point inside a tile wants that tile only; a point on a seam, where the
 * boxes of the neighbours decide, wants every neighbour that has a file: they
 * all come in together, and none is dropped to make room for another. */
struct TileFault {
        int centre, mask, stride;
};
constexpr double kRimGuard = 1e-9; /* of a directory cell: ~1e4 x the rounding of fx, fy */
/* Of a tile cell: how close to a seam the fast lookup trusts hx = (x - x0) * (1/dx)
 * to land on the same side as the reference's quotient.  The two differ by
 * < 4 ulp of hx (2e-11 cell for the largest grid, 65 535 nodes a side); 1e-9
 * leaves a factor 50, and is narrow enough (3e-8 m of a 30 m cell) that the
 * bisection of an exit through the mosaic's rim -- which converges ON the seam,
 * to 1e-8 m -- takes the exact way, with its dependent loads, for its last
 * couple of samples only and not for a dozen. */
constexpr double kSeamGuard = 1e-9;
constexpr int kTileFault = TAMD_TILE_PAGED; /* d_stack_tile's return value then */

/* The tile of a stack that answers for a point, -1 for none, or kTileFault
 * with `f` filled in [ref stack.c:300-335, :413-424]: see d_stack_elevation. */
__device__ __forceinline__ int d_stack_tile(const tamd_view & v, const tamd_stack & st,
    double latitude, double longitude, TileFault & f)
{
        const double fx = (longitude - st.lon0) / st.dlon;
        const double fy = (latitude - st.lat0) / st.dlat;
        /* No tile box reaches further than one cell from the directory -- and in
         * a regular stack (tiles exactly on the lattice, each spanning its cell up
         * to rounding) none reaches beyond its rim: out there the directory
         * formula [ref stack.c:413-424] finds no tile either.  This early answer
         * is what a ray that has left the mosaic gets at every later step of a
         * batch, and half the samples of the bisection of its exit: without it
         * each of them costs its whole wave the neighbourhood scan below (four
         * dependent loads, a dozen divisions). */
        const double reach = st.regular ? kRimGuard : 1.5;
        if (!((fx > -reach) && (fx < st.nlon + reach) && (fy > -reach) &&
                (fy < st.nlat + reach)))
                return -1;
        const int cx = min(max((int)fx, 0), st.nlon - 1);
        const int cy = min(max((int)fy, 0), st.nlat - 1);
        const int * tiles = v.tiles + st.tile_first;
        int tile = tiles[cy * st.nlon + cx];
        f.centre = st.tile_first + cy * st.nlon + cx, f.stride = st.nlon, f.mask = 1 << 4;
        /* Outside the directory's range the formula [ref stack.c:413-424] names no
         * tile, and the reference loads none: only tiles that ARE in memory can
         * answer (its list scan); a tile that is not is wanted only for a point in
         * the range, or within rounding of its rim. */
        const bool in_range = (fx > -kRimGuard) && (fx < st.nlon + kRimGuard) && (fy > -kRimGuard) &&
            (fy < st.nlat + kRimGuard);
        if (tile == TAMD_TILE_PAGED) {
                if (in_range) return kTileFault;
                tile = TAMD_TILE_NONE;
        }
        if ((tile < 0) || !d_tile_holds(v.grids[tile], latitude, longitude)) {
                /* rare: a seam, the rim, or a hole in the mosaic.  A neighbour
                 * that is not resident may be the one whose box holds the point:
                 * the whole neighbourhood has to be in memory to tell */
                int mask = 0, paged = 0;
                for (int j = -1; j <= 1; j++) {
                        for (int i = -1; i <= 1; i++) {
                                const int ix = cx + i, iy = cy + j;
                                if ((ix < 0) || (ix >= st.nlon) || (iy < 0) || (iy >= st.nlat)) continue;
                                const int t = tiles[iy * st.nlon + ix];
                                if (t == TAMD_TILE_NONE) continue;
                                mask |= 1 << (3 * (j + 1) + (i + 1));
                                if ((t == TAMD_TILE_PAGED) && in_range) paged = 1;
                        }
                }
                if (paged) {
                        f.mask = mask;
                        return kTileFault;
                }
                tile = -1;
                for (int j = -1; (j <= 1) && (tile < 0); j++) {
                        for (int i = -1; (i <= 1) && (tile < 0); i++) {
                                const int ix = cx + i, iy = cy + j;
                                if (((i == 0) && (j == 0)) || (ix < 0) || (ix >= st.nlon) ||
                                    (iy < 0) || (iy >= st.nlat))
                                        continue;
                                const int t = tiles[iy * st.nlon + ix];
                                if ((t >= 0) && d_tile_holds(v.grids[t], latitude, longitude))
                                        tile = t;
                        }
                }
                if (tile < 0) { /* [ref stack.c:413-424] */
                        if ((longitude < st.lon0) || (latitude < st.lat0)) return -1;
                        if (!(fx < st.nlon) || !(fy < st.nlat)) return -1;
                        tile = tiles[(int)fy * st.nlon + (int)fx]; /* == the centre: resident or none */
                }
        }
        return tile;
}

/* 1: inside (z set), 0: outside (z = 0), -1: a fault (f filled in) */
template <bool FAST = false>
__device__ __forceinline__ int d_stack_elevation(const tamd_view & v,
    const tamd_stack & st, double latitude, double longitude, double & z, TileFault & f)
{
        z = 0.;
        const int tile = d_stack_tile(v, st, latitude, longitude, f);
        if (tile < 0) return (tile == kTileFault) ? -1 : 0;
        const bool inside = d_grid_elevation<FAST>(v.grids[tile], longitude, latitude, z);
        if (!inside) z = 0.;
        return inside ? 1 : 0;
}

/* Fast-math lookup in a `regular` stack (see struct tamd_stack): interior
 * points take the tile by the directory formula and read its nodes through one
 * pointer; anything within kSeamGuard of a cell of a tile seam or of the directory's rim,
 * and any irregular stack, goes through the general routine above, which
 * decides seams and edges exactly as the reference does. */
/* `slots`: the stack's node pointers, one per directory slot, copied to LDS by
 * the kernel (see d_load_ctx) when TABLE.  The per-lane copy of the last tile's
 * pointer is then not needed (8 registers fewer in the trace kernel), and a
 * sample in a new tile waits for HBM once (the nodes), not twice in a row. */
typedef const uint16_t * node_ptr_t;
typedef const __attribute__((address_space(3))) node_ptr_t * lds_slots_t;

template <bool TABLE = false> /* TABLE: `slots` is there whenever the stack is regular */
__device__ __forceinline__ int f_stack_elevation(const tamd_view & v,
    const tamd_stack & st, double latitude, double longitude, double & z,
    CellCache * cache, TileFault & f, lds_slots_t slots = nullptr)
{
        if (st.regular) {
                const tamd_grid & p = st.proto;
                /* 1/dlon, 1/dlat: a last-ulp difference from the quotient can only
                 * pick the neighbouring tile for a point ON a seam, which is then
                 * not `interior` below and goes the exact way */
                const double fx = (longitude - st.lon0) * st.inv_dlon;
                const double fy = (latitude - st.lat0) * st.inv_dlat;
                const bool in_dir =
                    (fx > 0.) && (fx < (double)st.nlon) && (fy > 0.) && (fy < (double)st.nlat);
                const int tx = in_dir ? (int)fx : 0, ty = in_dir ? (int)fy : 0;
                const double x0 = st.lon0 + tx * st.dlon, y0 = st.lat0 + ty * st.dlat;
                const double hx = (longitude - x0) * p.inv_dx;
                const double hy = (latitude - y0) * p.inv_dy;
                const double mx = (double)(p.nx - 1) - kSeamGuard, my = (double)(p.ny - 1) - kSeamGuard;
                const bool interior =
                    in_dir && (hx > kSeamGuard) && (hx < mx) && (hy > kSeamGuard) && (hy < my);
                const int slot = ty * st.nlon + tx;
                const uint16_t * nodes = nullptr;
                if (TABLE) {
                        if (interior) nodes = slots[slot];
                } else if (interior) {
                        if ((cache != nullptr) && (cache->slot == slot))
                                nodes = cache->tile;
                        else {
                                nodes = v.slot_nodes[st.nodes_first + slot];
                                if (cache != nullptr) cache->slot = slot, cache->tile = nodes;
                        }
                }
                if (nodes != nullptr) {
                        const int ix = (int)hx, iy = (int)hy;
                        const double fxc = hx - (double)ix, fyc = hy - (double)iy;
                        const unsigned cell = (unsigned)iy * (unsigned)p.nx + (unsigned)ix;
                        const unsigned id = ((unsigned)slot << 24) | cell;
                        unsigned lo, hi;
                        if ((cache != nullptr) && (cache->id == id)) {
                                lo = cache->lo, hi = cache->hi;
                        } else {
                                d_cell_fetch(nodes, p.nbx, ix, iy, lo, hi);
                                if (cache != nullptr)
                                        cache->id = id, cache->lo = lo, cache->hi = hi;
                        }
                        double z00, z10, z01, z11;
                        if (p.is_signed) {
                                z00 = (double)(int16_t)(lo & 0xffffu), z10 = (double)((int)lo >> 16);
                                z01 = (double)(int16_t)(hi & 0xffffu), z11 = (double)((int)hi >> 16);
                        } else {
                                z00 = (double)(lo & 0xffffu), z10 = (double)(lo >> 16);
                                z01 = (double)(hi & 0xffffu), z11 = (double)(hi >> 16);
                        }
                        z00 = __builtin_fma(z00, p.dz, p.z0), z10 = __builtin_fma(z10, p.dz, p.z0);
                        z01 = __builtin_fma(z01, p.dz, p.z0), z11 = __builtin_fma(z11, p.dz, p.z0);
                        z = f_patch(z00, z10 - z00, z01 - z00, (z11 - z10) - (z01 - z00), fxc, fyc);
                        return 1;
                }
        }
        return d_stack_elevation<true>(v, st, latitude, longitude, z, f);
}

/* ---- layered sample ---------------------------------------------------- */

struct Sample {
        double lat, lon, alt;
        double e0, e1; /* bounding elevations [ref stepper.h:93-98] */
        int m, k;      /* index[0] = medium/layer, index[1] = data */
        TileFault fault; /* .centre >= 0: tiles have to be paged in (nothing else of
                          * the sample is then meaningful) */
        int slot;        /* tile-table index of the stack tile that answered (the first
                          * stack consulted), or -1: a ray that later waits for another
                          * tile wants this one kept too -- it is where it resumes */
};

/* 1: inside, 0: outside, -1: a fault, f filled in (stacks only) */
template <bool FAST = false>
__device__ __forceinline__ int d_source_elevation(const tamd_view & v,
    const tamd_meta & mt, double latitude, double longitude, double & z, TileFault & f)
{
        if (mt.kind == TAMD_FLAT) { /* [ref stepper.c:252-264] */
                z = 0.;
                return 1;
        } else if (mt.kind == TAMD_MAP) {
                const tamd_grid & g = v.grids[mt.src];
                if (g.proj.type >= 0) { /* [ref stepper.c:243-248, :304-311] */
                        double x, y;
                        d_project(g.proj, latitude, longitude, x, y);
                        return d_grid_elevation<FAST>(g, x, y, z);
                }
                /* [ref stepper.c:240-241] geodetic grid: x = lon, y = lat */
                return d_grid_elevation<FAST>(g, longitude, latitude, z);
        }
        return d_stack_elevation<FAST>(v, v.stacks[mt.src], latitude, longitude, z, f);
}

/* [ref stepper.c:703-756] + check_layer [ref stepper.c:687-701], always with
 * the exact transform (the reference at local_range = 0) and, when a geoid is
 * set, its undulation removed from the altitude [ref stepper.c:37-51]. */
/* Descriptors of the single data source of the one-map / one-stack modes,
 * read ONCE per kernel (they are wave-uniform: SGPRs) instead of per sample. */
struct OneCtx {
        tamd_grid grid;
        tamd_stack stack;
        double offset;
        lds_slots_t slots; /* one-stack mode, fast math, regular stack: see f_stack_elevation */
};

/* Called by every thread of the block, at the top of the kernel (it holds a
 * barrier when it fills the LDS table: blocks are 256 threads, and a regular
 * stack has at most 255 slots). */
template <int MODE, bool FAST = false>
__device__ __forceinline__ void d_load_ctx(const tamd_view & v, OneCtx & c)
{
        c.slots = nullptr;
        if (MODE == TAMD_MODE_GENERIC) return;
        const tamd_meta mt = v.metas[0];
        c.offset = mt.offset;
        if (MODE == TAMD_MODE_ONE_MAP) c.grid = v.grids[mt.src];
        if (MODE == TAMD_MODE_ONE_STACK) c.stack = v.stacks[mt.src];
        if ((MODE == TAMD_MODE_ONE_STACK) && FAST) {
                __shared__ node_ptr_t table[256];
                if (c.stack.regular) {
                        if ((int)threadIdx.x < c.stack.nlat * c.stack.nlon)
                                table[threadIdx.x] = v.slot_nodes[c.stack.nodes_first + threadIdx.x];
                        __syncthreads();
                        c.slots = (lds_slots_t)table;
                }
        }
}

/* The layers at geodetic coordinates already in s.lat, s.lon, s.alt */
/* TABLE: the one-stack fast lookup reads the tile pointers from ctx.slots (d_load_ctx); without,
 * from the lane's own copy of its last tile's pointer (cache->slot, cache->tile) */
template <int MODE, bool FAST = false, bool TABLE = true>
__device__ __forceinline__ void d_classify(
    const tamd_view & v, const OneCtx & ctx, Sample & s, CellCache * cache = nullptr)
{
        s.m = -1, s.k = -1, s.fault.centre = -1, s.slot = -1;
        s.e0 = -DBL_MAX, s.e1 = DBL_MAX; /* [ref stepper.c:713-716] */

        if (MODE != TAMD_MODE_GENERIC) {
                /* one layer holding one data: no loops, no geoid */
                double elevation;
                int inside;
                if (MODE == TAMD_MODE_ONE_MAP)
                        inside = FAST ?
                            f_grid_elevation(ctx.grid, s.lon, s.lat, elevation, cache) :
                            d_grid_elevation<false>(ctx.grid, s.lon, s.lat, elevation);
                else
                        inside = FAST ?
                            f_stack_elevation<TABLE>(v, ctx.stack, s.lat, s.lon, elevation, cache, s.fault, ctx.slots) :
                            d_stack_elevation<false>(v, ctx.stack, s.lat, s.lon, elevation, s.fault);
                if ((MODE == TAMD_MODE_ONE_STACK) && (inside >= 0)) s.slot = s.fault.centre;
                if ((MODE != TAMD_MODE_ONE_STACK) || (inside >= 0)) s.fault.centre = -1;
                if (inside > 0) {
                        elevation += ctx.offset;
                        s.k = 0;
                        if (elevation >= s.alt) {
                                s.m = 0;
                                s.e1 = elevation;
                        } else {
                                s.m = 1;
                                s.e0 = elevation;
                        }
                }
                return;
        }

        if (v.geoid >= 0) {
                double undulation;
                const double lo = (s.lon >= 0) ? s.lon : s.lon + 360.;
                if (d_grid_elevation<FAST>(v.grids[v.geoid], lo, s.lat, undulation))
                        s.alt -= undulation;
        }
        for (int layer = 0; layer < v.n_layers; layer++) {
                const int end = v.layer_first[layer + 1];
                int data_index = 0;
                for (int j = v.layer_first[layer]; j < end; j++, data_index++) {
                        const tamd_meta mt = v.metas[j];
                        double elevation;
                        TileFault f = { -1, 0, 0 };
                        const int inside = d_source_elevation<FAST>(v, mt, s.lat, s.lon, elevation, f);
                        if (inside < 0) { /* the layers cannot be told without that tile */
                                s.fault = f;
                                s.m = -1, s.k = -1;
                                return;
                        }
                        if (s.slot < 0) s.slot = f.centre;
                        if (inside == 0) continue;
                        elevation += mt.offset; /* [ref stepper.c:737] */
                        s.k = data_index;
                        if (elevation >= s.alt) { /* [ref stepper.c:690-694] */
                                s.m = layer;
                                s.e1 = elevation;
                                return;
                        }
                        s.m = layer + 1; /* [ref stepper.c:695-699] */
                        s.e0 = elevation;
                        break;
                }
        }
}

template <int MODE, bool FAST = false, bool TABLE = true>
__device__ __forceinline__ void d_sample(const tamd_view & v, const OneCtx & ctx, double x,
    double y, double z, Sample & s, CellCache * cache = nullptr)
{
        if (FAST)
                f_to_geodetic(x, y, z, s.lat, s.lon, s.alt);
        else
                d_to_geodetic(x, y, z, s.lat, s.lon, s.alt);
        d_classify<MODE, FAST, TABLE>(v, ctx, s, cache);
}

/* A sample of a ray that carries a line: at (x, y, z), which is parameter sl
 * of the line.  Taken from the line if it serves; else by the closed form,
 * which lays a new line through the point (origin there: the caller re-bases
 * its path parameter).  Returns true in that case.  Which of the two happens
 * depends on the ray's own line and sample only. */
template <int MODE>
__device__ __forceinline__ bool f_line_try(const tamd_view & v, const OneCtx & ctx,
    const RayLine & line, double sl, Sample & s, CellCache * cache, bool bracketed = false)
{
        bool serves = line.valid && (fabs(sl) <= kLineRange);
        if (serves) {
                f_line_eval(line, sl, s.lat, s.lon, s.alt);
                d_classify<MODE, true>(v, ctx, s, cache);
                serves = f_line_serves(line, sl, fmin(fabs(s.alt - s.e0), fabs(s.alt - s.e1)), bracketed);
        }
        return serves;
}

template <int MODE>
__device__ __forceinline__ void f_line_relay(const tamd_view & v, const OneCtx & ctx,
    double x, double y, double z, double dx, double dy, double dz, RayLine & line, Sample & s,
    CellCache * cache)
{
        f_to_geodetic(x, y, z, s.lat, s.lon, s.alt, &line, dx, dy, dz);
        d_classify<MODE, true>(v, ctx, s, cache);
}

template <int MODE>
__device__ __forceinline__ bool f_sample_on_line(const tamd_view & v, const OneCtx & ctx,
    double x, double y, double z, double dx, double dy, double dz, RayLine & line, double sl,
    Sample & s, CellCache * cache)
{
        const bool serves = f_line_try<MODE>(v, ctx, line, sl, s, cache);
        if (!serves) f_line_relay<MODE>(v, ctx, x, y, z, dx, dy, dz, line, s, cache);
        return !serves;
}

/* Where a fast trace samples next inside the bracket [ds0, ds1] of a crossing
 * [ref stepper.c:840-860 halves it, 27 times from a metre to 1e-8 m].
 *
 * While the bracket is wider than kBracketHalve, at its midpoint: the sample the
 * reference takes, so that the trace takes the reference's decisions where the
 * bracket may hold several crossings.  On rough ground it does: a step is 0.4 x
 * the clearance below the ray, and ground that rises faster than that along the
 * ray (a spike, a ridge thinner than the step, the wall of an HGT void) is crossed
 * twice or more within it.  Halving and false position then end on different
 * crossings, metres to kilometres apart -- on the rough tiles of
 * tests/rough_cases.py, false position from the step's full bracket ended on
 * another crossing than the reference for 55 of 10^4 rays of C2's recipe over the
 * void tile and for up to 13 % of the rays aimed at a void's edge.
 * Below kBracketHalve = 0.1 m the ground along the ray is one piece of a
 * bilinear cell (a parabola in the ray's parameter) or two, joined at a cell's
 * edge: to meet it twice within 0.1 m the ray has to pass within |f''| (0.05 m)^2
 * of a hollow or crest of that parabola, or within |slope change| x 0.05 m of a
 * cell's edge -- millimetres to centimetres on SRTM-like ground, decimetres on
 * the 200 m per-node noise of the rough tile, where a replay of this rule over the
 * oracle's samples found no such bracket among 44 000 rays: that is grazing, and
 * there either answer is one.
 *
 * Below kBracketHalve: false position.  c0, c1: the clearances (distance to the
 * nearest boundary, >= 0) of the samples at the two ends -- over a bracket this
 * narrow both measure the same boundary: the crossing is where they interpolate
 * to zero (with the Illinois rule: the clearance of an end that has stayed put
 * while the other moved twice by false position is halved, or a bent surface
 * would keep every sample on one side).  The sample is taken 0.4e-8 m to the side
 * of that estimate whose end is the farther one, so that once the estimate is
 * good the two ends close in from both sides: two such samples and the bracket is
 * 0.8e-8 m wide, where the reference's test ends it too, around the same crossing
 * (both brackets hold it, both are below 1e-8 m: the end points agree to that).
 * A bracket stays a bracket whatever the estimate is worth (a cell's edge, another
 * layer nearby, a first clearance that was only guessed); after kBracketPatience
 * samples in all the midpoint takes over again. */
constexpr double kBracketHalve = 0.1;
constexpr int kBracketPatience = 64;
__device__ __forceinline__ bool f_bracket_halves(double ds0, double ds1) { return ds1 - ds0 > kBracketHalve; }
__device__ __forceinline__ double f_bracket_point(double ds0, double ds1, double c0, double c1,
    int taken)
{
        const double w = ds1 - ds0;
        const double sum = c0 + c1;
        double t = 0.5 * (ds0 + ds1);
        if ((taken < kBracketPatience) && !f_bracket_halves(ds0, ds1) && (sum > 0.) && (sum < 1e30) &&
            (w > 2.5e-8)) {
                const double r = ds0 + w * (c0 / sum);
                const double aim = ((r - ds0) >= (ds1 - r)) ? r - 0.4e-8 : r + 0.4e-8;
                t = fmin(fmax(aim, ds0 + 0.25e-8), ds1 - 0.25e-8);
        }
        return t;
}

/* b + d t, a ray's next position [ref stepper.c:824, :862-863].  The reference rounds
 * the product and then the sum; the fast arithmetic of a trace fuses them.  The
 * sum's rounding (an ulp of 6.4e6 m: 9e-10 m) is what accumulates into the drift
 * that kLineDrift prices, the same either way; the product's (1e-16 of the step)
 * changes which way the sum rounds once in 1e7 steps. */
template <bool FAST>
__device__ __forceinline__ double d_along(double b, double d, double t)
{
        return FAST ? __builtin_fma(d, t, b) : b + d * t;
}

/* [ref stepper.c:799-813] tentative step length from the last sample */
__device__ __forceinline__ double d_step_length(
    const tamd_view & v, double alt, double e0, double e1, int m)
{
        double ds = 0.;
        if (m != 0) {
                const double dsi = fabs(alt - e0);
                if ((dsi < ds) || (ds <= 0.)) ds = dsi;
        }
        if (m != v.n_layers) {
                const double dsi = fabs(alt - e1);
                if ((dsi < ds) || (ds <= 0.)) ds = dsi;
        }
        ds *= v.slope;
        if (ds < v.resolution) ds = v.resolution;
        return ds;
}


/* ---- counter-based random directions (scattering harness, config C5) ------
 * Philox-4x32-10 (Salmon et al., SC'11): counter = (ray id, stream), key =
 * seed.  One block of four 32-bit words gives two 53-bit uniforms, mapped to
 * an isotropic unit vector.  Any (ray, stream) pair can be regenerated
 * anywhere, so shards need no shared RNG state. */
__device__ __forceinline__ void philox4x32_10(unsigned c[4], unsigned k0, unsigned k1)
{
        for (int round = 0; round < 10; round++) {
                const unsigned long long p0 = 0xD2511F53ull * c[0];
                const unsigned long long p1 = 0xCD9E8D57ull * c[2];
                const unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ k0;
                const unsigned n1 = (unsigned)p1;
                const unsigned n2 = (unsigned)(p0 >> 32) ^ c[3] ^ k1;
                const unsigned n3 = (unsigned)p0;
                c[0] = n0, c[1] = n1, c[2] = n2, c[3] = n3;
                k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
        }
}

/* sin and cos of 2 pi u, 0 <= u < 1, to the last ulp or so: the quadrant comes off
 * u exactly (k = round(4 u), r = u - k / 4 in [-1/8, 1/8]: no rounding), the rest is
 * the classic pair of polynomials on [-pi/4, pi/4] (fdlibm's k_sin / k_cos
 * coefficients) and a swap / sign by quadrant.  ~30 instructions where OCML's
 * sin + cos take ~250 with their large-argument paths: the walk kernel draws a
 * direction per step and is bound by the rate its instructions issue at. */
__device__ __forceinline__ void d_sincos_2pi(double u, double & s, double & c)
{
        const double k = __builtin_rint(4. * u); /* 0 .. 4 */
        const double t = 6.283185307179586 * __builtin_fma(-0.25, k, u);
        const double z = t * t;
        double ps = 1.58969099521155010221e-10;
        ps = __builtin_fma(ps, z, -2.50507602534068634195e-08);
        ps = __builtin_fma(ps, z, 2.75573137070700676789e-06);
        ps = __builtin_fma(ps, z, -1.98412698298579493134e-04);
        ps = __builtin_fma(ps, z, 8.33333333332248946124e-03);
        ps = __builtin_fma(ps, z, -1.66666666666666324348e-01);
        const double sn = __builtin_fma(t * z, ps, t);
        double pc = -1.13596475577881948265e-11;
        pc = __builtin_fma(pc, z, 2.08757232129817482790e-09);
        pc = __builtin_fma(pc, z, -2.75573143513906633035e-07);
        pc = __builtin_fma(pc, z, 2.48015872894767294178e-05);
        pc = __builtin_fma(pc, z, -1.38888888888741095749e-03);
        pc = __builtin_fma(pc, z, 4.16666666666666019037e-02);
        const double cs = __builtin_fma(z * z, pc, __builtin_fma(-0.5, z, 1.));
        const int q = (int)k & 3;
        /* 2 pi u = q pi / 2 + t */
        s = (q == 0) ? sn : ((q == 1) ? cs : ((q == 2) ? -sn : -cs));
        c = (q == 0) ? cs : ((q == 1) ? -sn : ((q == 2) ? -cs : sn));
}

/* the isotropic unit vector of (ray id, stream; seed): see k_isotropic */
__device__ __forceinline__ void d_isotropic(ull id, ull stream, ull seed, double & x, double & y, double & z)
{
        unsigned c[4] = { (unsigned)id, (unsigned)(id >> 32), (unsigned)stream, (unsigned)(stream >> 32) };
        philox4x32_10(c, (unsigned)seed, (unsigned)(seed >> 32));
        const double scale = 1. / 9007199254740992.; /* 2^-53 */
        const double u1 = (double)(((ull)(c[0] >> 5) << 26) | (c[1] >> 6)) * scale;
        const double u2 = (double)(((ull)(c[2] >> 5) << 26) | (c[3] >> 6)) * scale;
        const double ct = 2. * u1 - 1.;
        const double st = sqrt(1. - ct * ct);
        double sp, cp;
        d_sincos_2pi(u2, sp, cp);
        x = st * cp, y = st * sp, z = ct;
}

/* ======================================================================== */
/*                          the device stepper API                          */
/* ======================================================================== */

/* the arithmetic: the values of turtle_amd_math_set (enum turtle_amd_math) */
enum { FAST = 0, STRICT = 1 };
/* the kernel modes of a view (view.geometry.mode) */
enum { GENERIC = TAMD_MODE_GENERIC, ONE_MAP = TAMD_MODE_ONE_MAP, ONE_STACK = TAMD_MODE_ONE_STACK };

/* Host side: calls f(std::integral_constant<int, MODE>()) for the mode of the view, so that a
 * launcher instantiates its kernel per mode as the library's do.  false, and f is not called,
 * for a view that this header cannot read (turtle_amd_view_ok). */
template <class F>
inline bool dispatch(const turtle_amd_view & view, F && f)
{
        if (!turtle_amd_view_ok(&view)) return false;
        switch (view.geometry.mode) {
        case TAMD_MODE_ONE_MAP:
                f(std::integral_constant<int, ONE_MAP>());
                return true;
        case TAMD_MODE_ONE_STACK:
                f(std::integral_constant<int, ONE_STACK>());
                return true;
        case TAMD_MODE_GENERIC:
                f(std::integral_constant<int, GENERIC>());
                return true;
        }
        return false;
}

/* What every call below reads the geometry through: the view, and -- in the one-map and
 * one-stack modes -- the descriptor of its single data source, read ONCE (wave-uniform: scalar
 * registers) instead of per sample.  Construct it at the top of the kernel. */
template <int MODE, int MATH>
struct Geometry {
        tamd_view v;
        OneCtx ctx;
        __device__ __forceinline__ explicit Geometry(const turtle_amd_view & view) : Geometry(view.geometry) {}
        /* (the library's own kernels take the tables bare) */
        __device__ __forceinline__ explicit Geometry(const tamd_view & geometry) : v(geometry)
        {
                ctx.slots = nullptr; /* (the LDS table of tile pointers is the library's kernels' own) */
                if (MODE != GENERIC) {
                        const tamd_meta mt = v.metas[0];
                        ctx.offset = mt.offset;
                        if (MODE == ONE_MAP) ctx.grid = v.grids[mt.src];
                        if (MODE == ONE_STACK) ctx.stack = v.stacks[mt.src];
                }
        }
};

/* The last cell and tile a lane looked up (FAST, one-map / one-stack: a ray stays in a cell for
 * several samples).  Part of a ray's state; nothing of it decides a result. */
struct Cell : CellCache {
        __device__ __forceinline__ Cell() : CellCache{ ~0u, 0u, 0u, -1, nullptr } {}
};

/* What turtle_stepper_step publishes, and what the next step() resumes from, as the reference
 * resumes from its `last` sample [ref stepper.c:708-710, :780-875]. */
struct State {
        double latitude, longitude, altitude;
        double elevation[2]; /* the bounding elevations; +-DBL_MAX where there is none; 0, 0 outside the data */
        int index[2];        /* medium (layer), data; -1, -1 outside the data */
        double step_length;  /* sample(): the tentative length of the next step; step(): the length taken */
        Cell cell;
};

template <int MODE, int MATH>
__device__ __forceinline__ void d_sample_at(const Geometry<MODE, MATH> & g, double x, double y, double z,
    Sample & s, Cell & cell)
{
        CellCache * cache = ((MATH == FAST) && (MODE != GENERIC)) ? &cell : nullptr;
        d_sample<MODE, MATH == FAST, false>(g.v, g.ctx, x, y, z, s, cache);
}

/* turtle_stepper_step(stepper, position, NULL, ...) [ref stepper.c:780-796]: the layers at `pos` */
template <int MODE, int MATH>
__device__ __forceinline__ void sample(const Geometry<MODE, MATH> & g, const double pos[3], State & st)
{
        Sample s;
        d_sample_at(g, pos[0], pos[1], pos[2], s, st.cell);
        st.latitude = s.lat, st.longitude = s.lon, st.altitude = s.alt;
        /* (outside the data the call publishes 0, 0) */
        st.elevation[0] = (s.m >= 0) ? s.e0 : 0., st.elevation[1] = (s.m >= 0) ? s.e1 : 0.;
        st.index[0] = s.m, st.index[1] = s.k;
        st.step_length = d_step_length(g.v, s.alt, s.e0, s.e1, s.m);
}

/* One turtle_stepper_step with a direction, resumed from `st` (of sample() or of the last
 * step()) [ref stepper.c:799-875]: the tentative step; where the medium changed there, the
 * bracket halved in place to 1e-8 m, the ray going on from the halving's last sample of the new
 * medium [ref stepper.c:849-858].  `pos` moves; `st` becomes what the call publishes (step_length:
 * the length taken).  Divergent: a lane that halves (~27 samples) holds its wave.  A ray outside
 * the data (st.index[0] < 0) takes no step: false. */
template <int MODE, int MATH>
__device__ __forceinline__ bool step(const Geometry<MODE, MATH> & g, State & st, double pos[3], const double dir[3])
{
        if (st.index[0] < 0) return false;
        const double ds = d_step_length(g.v, st.altitude, st.elevation[0], st.elevation[1], st.index[0]);
        const double bx = pos[0] + dir[0] * ds, by = pos[1] + dir[1] * ds, bz = pos[2] + dir[2] * ds;
        Sample s;
        d_sample_at(g, bx, by, bz, s, st.cell);
        double taken = ds;
        pos[0] = bx, pos[1] = by, pos[2] = bz;
        if (s.m != st.index[0]) { /* [ref stepper.c:836-864] */
                double ds0 = -ds, ds1 = 0.;
                int halvings = 0;
                do {
                        const double t = 0.5 * (ds0 + ds1);
                        Sample h;
                        d_sample_at(g, bx + dir[0] * t, by + dir[1] * t, bz + dir[2] * t, h, st.cell);
                        if (h.m == st.index[0])
                                ds0 = t;
                        else
                                ds1 = t, s = h;
                        halvings++;
                } while ((ds1 - ds0 > 1E-08) && !(halvings > 1200));
                pos[0] = bx + dir[0] * ds1, pos[1] = by + dir[1] * ds1, pos[2] = bz + dir[2] * ds1;
                taken = ds + ds1;
        }
        st.latitude = s.lat, st.longitude = s.lon, st.altitude = s.alt;
        /* (outside the data the call publishes 0, 0) */
        st.elevation[0] = (s.m >= 0) ? s.e0 : 0., st.elevation[1] = (s.m >= 0) ? s.e1 : 0.;
        st.index[0] = s.m, st.index[1] = s.k;
        st.step_length = taken;
        return true;
}

/* ---- the normal of a layer's top surface (turtle_stepper_normal_n) ---------- */

/* the step of the central differences that carry a projected map's gradient (metres per map
 * metre) over to degrees: d(x, y) / d(latitude, longitude) of the forward projection */
constexpr double kNormalDelta = 1e-3;

/* Elevation and gradient (per degree; 0 on entry) of one data of a layer: 1 inside, 0 outside
 * (z, glat, glon are then meaningless), kTileFault with `f` filled in.  PROJECTED: the data may
 * be a projected map (the generic instance alone: d_project is out of line). */
template <bool PROJECTED>
__device__ __forceinline__ int d_source_slope(const tamd_view & v, const tamd_meta & mt, double latitude,
    double longitude, double & z, double & glat, double & glon, TileFault & f)
{
        glat = glon = 0.;
        if (mt.kind == TAMD_FLAT) {
                z = 0.;
                return 1;
        }
        if (mt.kind == TAMD_MAP) {
                const tamd_grid & g = v.grids[mt.src];
                if (PROJECTED && (g.proj.type >= 0)) {
                        double x, y, gx = 0., gy = 0.;
                        d_project(g.proj, latitude, longitude, x, y);
                        if (!d_grid_elevation(g, x, y, z)) return 0;
                        d_grid_gradient<true>(g, x, y, gx, gy);
                        /* the chain rule, in this operand order (turtle_amd.h states it) */
                        const double d = kNormalDelta;
                        double xp, yp, xm, ym;
                        d_project(g.proj, latitude + d, longitude, xp, yp);
                        d_project(g.proj, latitude - d, longitude, xm, ym);
                        glat = gx * (xp - xm) / (2. * d) + gy * (yp - ym) / (2. * d);
                        d_project(g.proj, latitude, longitude + d, xp, yp);
                        d_project(g.proj, latitude, longitude - d, xm, ym);
                        glon = gx * (xp - xm) / (2. * d) + gy * (yp - ym) / (2. * d);
                        return 1;
                }
                if (!d_grid_elevation(g, longitude, latitude, z)) return 0;
                d_grid_gradient<true>(g, longitude, latitude, glon, glat);
                return 1;
        }
        /* a stack: the tile that answers for the elevation answers for the gradient
         * [ref stack.c:338-388]; x = longitude, y = latitude */
        const int tile = d_stack_tile(v, v.stacks[mt.src], latitude, longitude, f);
        if (tile < 0) return (tile == kTileFault) ? kTileFault : 0;
        const tamd_grid & g = v.grids[tile];
        if (!d_grid_elevation(g, longitude, latitude, z)) return 0;
        d_grid_gradient<true>(g, longitude, latitude, glon, glat);
        return 1;
}

/* The unit normal, towards increasing altitude, of the surface (latitude, longitude) ->
 * from_geodetic(latitude, longitude, hs(latitude, longitude)) where its height is hs and its
 * slopes are glat, glon per degree.  Its tangents are A E + glon U and B N + glat U, with (E, N,
 * U) the local east, north, up [ref ecef.c:136-154] and A, B the metres per degree of longitude
 * and latitude at that height.  pole: no east term (there is no east at a pole). */
__device__ __forceinline__ void d_surface_normal(double latitude, double longitude, double hs, double glat,
    double glon, bool pole, double n[3])
{
        const double lambda = longitude * kPi / 180.;
        const double phi = latitude * kPi / 180.;
        const double sl = sin(lambda), cl = cos(lambda);
        const double sp = sin(phi), cp = cos(phi);
        const double e[3] = { -sl, cl, 0. };
        const double nn[3] = { -cl * sp, -sl * sp, cp };
        const double u[3] = { cl * cp, sl * cp, sp };
        const double g = 1. - kE * kE * sp * sp;
        const double Rn = kA / sqrt(g);
        const double Rm = Rn * (1. - kE * kE) / g;
        const double A = (Rn + hs) * cp * kPi / 180.;
        const double B = (Rm + hs) * kPi / 180.;
        const double a = glon / A, b = glat / B;
        double w[3];
        for (int i = 0; i < 3; i++) w[i] = pole ? u[i] - b * nn[i] : u[i] - a * e[i] - b * nn[i];
        const double norm = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
        for (int i = 0; i < 3; i++) n[i] = w[i] / norm;
}

/* The normal of the top surface of `layer` above or below `pos`, whatever the altitude of `pos`:
 * one point of turtle_stepper_normal_n (turtle_amd.h has the definition as a loop).  Returns the
 * rank of the data that answered within the layer, last added first, with n[] set; or -1, n[]
 * untouched, where the layer has no data (or there is no such layer).  After an event of
 * Stepping::trip() that crossed from medium a to medium b, the surface crossed is the top of layer
 * min(a, b).  The arithmetic is always the STRICT one, whatever MATH is.  `fault`: the library's
 * own kernels over paged stacks (kTileFault comes back, *fault filled in); a view names resident
 * tiles only. */
template <int MODE, int MATH>
__device__ __forceinline__ int normal(const Geometry<MODE, MATH> & g, const double pos[3], int layer,
    double n[3], TileFault * fault = nullptr)
{
        double latitude, longitude, altitude;
        d_to_geodetic(pos[0], pos[1], pos[2], latitude, longitude, altitude);
        const bool pole = (pos[0] == 0.) && (pos[1] == 0.); /* [ref ecef.c:77-84] */
        if ((layer < 0) || (layer >= g.v.n_layers)) return -1;

        TileFault f = { -1, 0, 0 };
        double z = 0., glat = 0., glon = 0., hs = 0.;
        int found = -1;
        if (MODE == ONE_MAP) {
                if (!d_grid_elevation(g.ctx.grid, longitude, latitude, z)) return -1;
                d_grid_gradient<true>(g.ctx.grid, longitude, latitude, glon, glat);
                hs = z + g.ctx.offset;
                found = 0;
        } else if (MODE == ONE_STACK) {
                const int tile = d_stack_tile(g.v, g.ctx.stack, latitude, longitude, f);
                if (tile == kTileFault) {
                        if (fault != nullptr) *fault = f;
                        return kTileFault;
                }
                if (tile < 0) return -1;
                const tamd_grid & t = g.v.grids[tile];
                if (!d_grid_elevation(t, longitude, latitude, z)) return -1;
                d_grid_gradient<true>(t, longitude, latitude, glon, glat);
                hs = z + g.ctx.offset;
                found = 0;
        } else {
                const int end = g.v.layer_first[layer + 1];
                int di = 0;
                for (int j = g.v.layer_first[layer]; j < end; j++, di++) { /* [ref stepper.c:897-921] */
                        const tamd_meta mt = g.v.metas[j];
                        const int in = d_source_slope<true>(g.v, mt, latitude, longitude, z, glat, glon, f);
                        if (in == kTileFault) {
                                if (fault != nullptr) *fault = f;
                                return kTileFault;
                        }
                        if (in == 0) continue;
                        hs = z + mt.offset;
                        found = di;
                        break;
                }
                if (found < 0) return -1;
                if (g.v.geoid >= 0) { /* [ref stepper.c:905-914]: the undulation lifts and tilts the surface */
                        const tamd_grid & geoid = g.v.grids[g.v.geoid];
                        const double lo = (longitude >= 0) ? longitude : longitude + 360.;
                        double undulation, ugx = 0., ugy = 0.;
                        if (d_grid_elevation(geoid, lo, latitude, undulation)) hs += undulation;
                        if (d_grid_gradient<true>(geoid, lo, latitude, ugx, ugy)) glon += ugx, glat += ugy;
                }
        }
        d_surface_normal(latitude, longitude, hs, glat, glon, pole, n);
        return found;
}

/* ---- column depth along a step in an exponential medium ------------------------
 * The arithmetic of turtle_stepper_advance_exp_n (include/turtle_amd.h states the loop), for a
 * caller that steps rays inside its own kernel.  Over a step of length ds from altitude a0 to a1,
 * in a medium of density rho0 * exp(-h / H), the altitude is taken as linear in the path: the
 * density f metres into the step is c * exp(w * f), with
 *     c = rho0 * exp(-a0 / H),   w = -((a1 - a0) / H) / ds        (uniform medium: c = rho0, w = 0).
 * column_depth: the depth of the step's first f metres.  column_reach: its inverse, how far into
 * the step the depth R lasts (NaN where the step never spends R: no comparison with it holds).
 * Plain double-precision exp-family functions, whatever the arithmetic of the stepping. */
__device__ __forceinline__ double column_depth(double c, double w, double f)
{
        return (w * f == 0.) ? c * f : c * expm1(w * f) / w;
}
__device__ __forceinline__ double column_reach(double c, double w, double R)
{
        return (w == 0.) ? R / c : log1p(R * w / c) / w;
}

/* ---- column depth along a step through a density grid --------------------------
 * The walk of turtle_stepper_advance_grid_n (include/turtle_amd.h states it piece by piece), for a
 * caller that steps rays inside its own kernel: the depth of the first L metres of the straight
 * line p0 + dir * f, begun in medium m where the density is rho_out outside the box G and the
 * voxel's inside it, stopped where the depth reaches R.  -> x: the depth of [0, L] (not stopped);
 * f: where the walk ended (L, or the point where R was reached); stopped.  A voxel of density 0
 * never stops the walk and nothing divides by it.  The line is straight in ECEF and so are the
 * box's axes: the sum is exact, one term a voxel met.  The axes' state (s, t, the index, the next
 * face) is kept in named registers and picked by selects, never by a runtime index: nothing goes
 * to scratch.  A face's distance is computed from the voxel's index each time: nothing accumulates.
 * The voxel index is clamped on entry and tested at every move: no load leaves the grid. */
struct GridDepth {
        double x, f;
        bool stopped;
};

__device__ __forceinline__ GridDepth grid_depth(const turtle_amd_grid_view & G, double rho_out, int m,
    double p0x, double p0y, double p0z, double dx, double dy, double dz, double L, double R)
{
        GridDepth out = { 0., L, false };
        double acc = 0.;
        /* one piece (a, b, rho) of [0, L]: true where it stops the walk */
        const auto piece = [&](double a, double b, double rho) {
                const double x = rho * (b - a);
                if ((x > 0.) && (acc + x >= R)) {
                        out.f = a + (R - acc) / rho, out.stopped = true;
                        return true;
                }
                acc += x;
                return false;
        };
        double f = 0.;
        if (m == G.medium) {
                const double rx = p0x - G.origin[0], ry = p0y - G.origin[1], rz = p0z - G.origin[2];
                const double s0 = G.axis[0][0] * rx + G.axis[0][1] * ry + G.axis[0][2] * rz;
                const double s1 = G.axis[1][0] * rx + G.axis[1][1] * ry + G.axis[1][2] * rz;
                const double s2 = G.axis[2][0] * rx + G.axis[2][1] * ry + G.axis[2][2] * rz;
                const double t0 = G.axis[0][0] * dx + G.axis[0][1] * dy + G.axis[0][2] * dz;
                const double t1 = G.axis[1][0] * dx + G.axis[1][1] * dy + G.axis[1][2] * dz;
                const double t2 = G.axis[2][0] * dx + G.axis[2][1] * dy + G.axis[2][2] * dz;
                /* the slab test: [f0, f1] of [0, L] lies in the box */
                double f0 = 0., f1 = L;
                bool hit = true;
                const auto slab = [&](double s, double t, int n, double size) {
                        const double E = n * size;
                        if (t == 0.) {
                                if (!((s >= 0.) && (s < E))) hit = false;
                        } else {
                                double u = (0. - s) / t, v = (E - s) / t;
                                if (u > v) {
                                        const double swap = u;
                                        u = v, v = swap;
                                }
                                if (u > f0) f0 = u;
                                if (v < f1) f1 = v;
                        }
                };
                slab(s0, t0, G.n[0], G.size[0]);
                slab(s1, t1, G.n[1], G.size[1]);
                slab(s2, t2, G.n[2], G.size[2]);
                if (hit && (f0 < f1)) {
                        if (piece(0., f0, rho_out)) return out;
                        const auto enter = [&](double s, double t, int n, double size) {
                                const double c = floor((s + f0 * t) / size);
                                return (c > 0.) ? ((c < n - 1) ? (int)c : n - 1) : 0; /* (NaN: 0) */
                        };
                        const auto face = [](int i, double s, double t, double size) {
                                return (t == 0.) ? HUGE_VAL : ((i + ((t > 0.) ? 1 : 0)) * size - s) / t;
                        };
                        int i0 = enter(s0, t0, G.n[0], G.size[0]), i1 = enter(s1, t1, G.n[1], G.size[1]),
                            i2 = enter(s2, t2, G.n[2], G.size[2]);
                        double n0 = face(i0, s0, t0, G.size[0]), n1 = face(i1, s1, t1, G.size[1]),
                               n2 = face(i2, s2, t2, G.size[2]);
                        f = f0;
                        for (;;) {
                                /* the axis of the nearest face (ties: the lowest) */
                                const int a = ((n0 <= n1) && (n0 <= n2)) ? 0 : ((n1 <= n2) ? 1 : 2);
                                const double na = (a == 0) ? n0 : ((a == 1) ? n1 : n2);
                                double g = (na < f1) ? na : f1;
                                if (g < f) g = f; /* (no piece is negative) */
                                if (piece(f, g, G.density[((long)i2 * G.n[1] + i1) * G.n[0] + i0])) return out;
                                f = g;
                                if (!(na < f1)) break;
                                const double ta = (a == 0) ? t0 : ((a == 1) ? t1 : t2);
                                const double sa = (a == 0) ? s0 : ((a == 1) ? s1 : s2);
                                const double za = (a == 0) ? G.size[0] : ((a == 1) ? G.size[1] : G.size[2]);
                                const int ca = (a == 0) ? G.n[0] : ((a == 1) ? G.n[1] : G.n[2]);
                                const int ia = ((a == 0) ? i0 : ((a == 1) ? i1 : i2)) + ((ta > 0.) ? 1 : -1);
                                if ((ia < 0) || (ia >= ca)) break;
                                const double nn = face(ia, sa, ta, za);
                                i0 = (a == 0) ? ia : i0, i1 = (a == 1) ? ia : i1, i2 = (a == 2) ? ia : i2;
                                n0 = (a == 0) ? nn : n0, n1 = (a == 1) ? nn : n1, n2 = (a == 2) ? nn : n2;
                        }
                }
        }
        piece(f, L, rho_out); /* what lies past the box, or all of it */
        out.x = acc;
        return out;
}

/* ---- the step machine of Stepping::trip() below and of the library's k_walk ----
 * One sample per live lane and trip, at q = B + d * t: the origin itself (ST_INIT, the callers'
 * own business), a tentative step (ST_STEP: t = ds), or one halving of a crossing (ST_BISECT:
 * t = (ds0 + ds1) / 2 about B, the tentative position that crossed).  (k_traverse keeps a copy
 * of its own, for the reason of speed given there.) */
enum { ST_INIT = 0, ST_STEP = 1, ST_BISECT = 2 };

/* What a ray keeps while a crossing is located: the bracket, and the halving's last sample of the
 * other medium, which the ray goes on from [ref stepper.c:849-858]. */
struct Bisection {
        double ds0, ds1;
        double b_alt, b_e0, b_e1;
        int bm, bk, halvings;
};
struct StepOutcome {
        bool accept;  /* a ST_STEP sample in the ray's medium: the step stands, B is its end */
        bool located; /* the bracket is closed: the crossing is at B + d * ds1 [ref stepper.c:861-863] */
};

/* The bookkeeping of one sample `s` of a ray in medium m whose tentative step is ds, as selects.
 * A ST_STEP sample moves B to q; one of another medium opens or narrows the bracket (1e-8 m, or
 * 1200 halvings: the guard).  What an accepted step and a located crossing mean to the ray is the
 * caller's, who sets the state back to ST_STEP after a located crossing. */
__device__ __forceinline__ StepOutcome step_or_bisect(Bisection & b, int & state, double & bx, double & by,
    double & bz, int m, double ds, double t, double qx, double qy, double qz, const Sample & s)
{
        const bool stepping = (state == ST_STEP);
        const bool same = (s.m == m);
        const bool accept = stepping & same;
        const bool cross = stepping & !same;
        const bool other = !same;
        bx = stepping ? qx : bx, by = stepping ? qy : by, bz = stepping ? qz : bz;
        b.bm = other ? s.m : b.bm, b.bk = other ? s.k : b.bk;
        b.b_alt = other ? s.alt : b.b_alt, b.b_e0 = other ? s.e0 : b.b_e0, b.b_e1 = other ? s.e1 : b.b_e1;
        b.ds0 = cross ? -ds : ((!stepping & same) ? t : b.ds0);
        b.ds1 = cross ? 0. : ((!stepping & other) ? t : b.ds1);
        b.halvings = stepping ? 0 : b.halvings + 1;
        state = cross ? ST_BISECT : state;
        const bool located = (state == ST_BISECT) & !cross &
            (!(b.ds1 - b.ds0 > 1E-08) | (b.halvings > 1200));
        return { accept, located };
}

/* what a trip() reports */
enum Event {
        NONE = 0,     /* nothing yet: the ray is halving a crossing, or is not live */
        ORIGIN = 1,   /* the origin was sampled (after start()): the ray stands on its first sample */
        STEP = 2,     /* a step was accepted: `length` long, in the medium the ray was in */
        CROSSING = 3, /* a crossing was located: the ray left medium `from` and stands in index[0],
                       * `length` is the step's full length up to the crossing */
        LEFT = 4      /* the ray left the data (index[0] < 0), by a crossing (`from`, `length` as for
                       * CROSSING) or at its origin (from = -1, length = 0); it is no longer live */
};

/* One ray per lane, stepped one SAMPLE at a time.  trip() evaluates exactly one sample for a
 * live lane -- the origin's, a tentative step's, or one halving of a crossing -- with the
 * bookkeeping as selects, so a wave whose lanes are at different points of their steps runs the
 * expensive part with a full exec mask.  Between events the caller may redirect() the ray (a
 * scattering), stop() it, or start() / resume() another one in the lane.  Same arithmetic on
 * the same values as step(): same bits.
 *
 * Per lane: position and direction (6 doubles), the sample it stands on (3 doubles, 2 ints),
 * the bracket and the halving's last sample of the other medium (6 doubles, 3 ints), the state
 * and, FAST in the one-map / one-stack modes, the cell cache (3 words, and a slot and a pointer
 * over a stack): what k_traverse keeps. */
template <int MODE, int MATH>
struct Stepping {
        double x[3], d[3];   /* position and direction (any length: steps are in units of it) */
        double altitude;     /* the sample the ray stands on: what turtle_stepper_step publishes */
        double elevation[2]; /* (after LEFT: -+DBL_MAX, where the batch calls publish 0, 0) */
        int index[2];
        double length;       /* of the last event */
        int from;            /* of the last event: the medium left */
        bool live;

        __device__ __forceinline__ Stepping() : live(false), state_(ST_INIT) {}

        /* a new ray: the next trip() samples its origin */
        __device__ __forceinline__ void start(const double pos[3], const double dir[3])
        {
                x[0] = pos[0], x[1] = pos[1], x[2] = pos[2];
                d[0] = dir[0], d[1] = dir[1], d[2] = dir[2];
                index[0] = index[1] = -1, length = 0., from = -1;
                state_ = ST_INIT, live = true;
        }

        /* a ray whose sample is known (of sample(), step(), a batch call): the next trip() steps */
        __device__ __forceinline__ void resume(const Geometry<MODE, MATH> & g, const double pos[3],
            const double dir[3], double alt, double e0, double e1, int medium, int data)
        {
                x[0] = pos[0], x[1] = pos[1], x[2] = pos[2];
                d[0] = dir[0], d[1] = dir[1], d[2] = dir[2];
                altitude = alt, elevation[0] = e0, elevation[1] = e1, index[0] = medium, index[1] = data;
                length = 0., from = -1;
                state_ = ST_STEP, live = (medium >= 0);
                ds_ = d_step_length(g.v, alt, e0, e1, medium);
        }

        /* after an event: the direction of the next step */
        __device__ __forceinline__ void redirect(double dx, double dy, double dz) { d[0] = dx, d[1] = dy, d[2] = dz; }
        __device__ __forceinline__ void stop() { live = false; }
        /* the tentative length of the next step (after an event) */
        __device__ __forceinline__ double tentative() const { return ds_; }

        __device__ __forceinline__ int trip(const Geometry<MODE, MATH> & g)
        {
                int event = NONE;
                if (live) {
                        /* ---- one sample at q = B + d * t (the origin itself first) ---- */
                        const bool init = (state_ == ST_INIT);
                        const bool stepping = (state_ == ST_STEP);
                        const double t = stepping ? ds_ : 0.5 * (b_.ds0 + b_.ds1);
                        const double qx = init ? x[0] : x[0] + d[0] * t, qy = init ? x[1] : x[1] + d[1] * t,
                                     qz = init ? x[2] : x[2] + d[2] * t;
                        Sample s;
                        d_sample_at(g, qx, qy, qz, s, cell_);
                        if (init) { /* [ref stepper.c:780-796] */
                                index[0] = s.m, index[1] = s.k;
                                altitude = s.alt, elevation[0] = s.e0, elevation[1] = s.e1;
                                state_ = ST_STEP;
                                event = ORIGIN;
                        } else {
                                const StepOutcome o = step_or_bisect(b_, state_, x[0], x[1], x[2], index[0], ds_, t, qx, qy, qz, s);
                                if (o.accept) {
                                        length = ds_, from = index[0], index[1] = s.k;
                                        altitude = s.alt, elevation[0] = s.e0, elevation[1] = s.e1;
                                        event = STEP;
                                }
                                if (o.located) { /* [ref stepper.c:861-863] */
                                        x[0] = x[0] + d[0] * b_.ds1, x[1] = x[1] + d[1] * b_.ds1, x[2] = x[2] + d[2] * b_.ds1;
                                        length = ds_ + b_.ds1, from = index[0];
                                        index[0] = b_.bm, index[1] = b_.bk;
                                        altitude = b_.b_alt, elevation[0] = b_.b_e0, elevation[1] = b_.b_e1;
                                        state_ = ST_STEP;
                                        event = CROSSING;
                                }
                        }
                        if (event != NONE) {
                                if (index[0] < 0)
                                        event = LEFT, live = false;
                                else
                                        ds_ = d_step_length(g.v, altitude, elevation[0], elevation[1], index[0]);
                        }
                }
                return event;
        }

private:
        int state_;
        double ds_;
        Bisection b_;
        Cell cell_;
};

/* The isotropic unit vector of Philox-4x32-10(ray, stream; seed): element `ray` of
 * turtle_amd_isotropic_n(seed, stream), and the direction turtle_stepper_scatter_n gives ray
 * `first + r` at generation `stream`. */
__device__ __forceinline__ void isotropic(unsigned long long ray, unsigned long long stream,
    unsigned long long seed, double dir[3])
{
        d_isotropic(ray, stream, seed, dir[0], dir[1], dir[2]);
}

#pragma clang diagnostic pop

} /* namespace turtle_amd_device */

#endif /* __HIPCC__ */
#endif
