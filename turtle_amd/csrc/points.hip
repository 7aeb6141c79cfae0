/*
 * points.hip -- the kernels over batches of points, one point a thread, and their launchers.
 * The arithmetic contract and the citations [ref FILE:LINE] are device.hip's (see its header).
 *
 *   k_ecef_*        batch ECEF transforms              [ref ecef.c:41-207]
 *   k_project       batch map projections
 *   k_elevation     batch bilinear lookup, map/stack   [ref map.c:229-277, stack.c:300-361]
 *   k_gradient      batch gradients
 *   k_position      batch turtle_stepper_position      [ref stepper.c:877-931]
 *   k_normal        batch normals of a layer's top surface (turtle_stepper_normal_n)
 */
#include <hip/hip_runtime.h>

#include <cfloat>

#include "device_common.h"
#include "device_launch.h"

namespace {

__global__ void k_ecef_from_geodetic(long n, const double * __restrict__ lat,
    const double * __restrict__ lon, const double * __restrict__ elev,
    double * __restrict__ ecef)
{
        for (long r = blockIdx.x * (long)blockDim.x + threadIdx.x; r < n;
             r += (long)gridDim.x * blockDim.x) {
                double x, y, z;
                d_from_geodetic(lat[r], lon[r], elev[r], x, y, z);
                ecef[3 * r] = x, ecef[3 * r + 1] = y, ecef[3 * r + 2] = z;
        }
}

template <bool FAST>
__global__ void k_ecef_to_geodetic(long n, const double * __restrict__ ecef,
    double * __restrict__ lat, double * __restrict__ lon, double * __restrict__ alt)
{
        for (long r = blockIdx.x * (long)blockDim.x + threadIdx.x; r < n;
             r += (long)gridDim.x * blockDim.x) {
                double la, lo, al;
                if (FAST)
                        f_to_geodetic(ecef[3 * r], ecef[3 * r + 1], ecef[3 * r + 2], la, lo, al);
                else
                        d_to_geodetic(ecef[3 * r], ecef[3 * r + 1], ecef[3 * r + 2], la, lo, al);
                if (lat) lat[r] = la;
                if (lon) lon[r] = lo;
                if (alt) alt[r] = al;
        }
}

/* [ref ecef.c:160-176] */
__global__ void k_ecef_from_horizontal(long n, const double * __restrict__ lat,
    const double * __restrict__ lon, const double * __restrict__ az_,
    const double * __restrict__ el_, double * __restrict__ dir)
{
        for (long r = blockIdx.x * (long)blockDim.x + threadIdx.x; r < n;
             r += (long)gridDim.x * blockDim.x) {
                double e[3], nn[3], u[3];
                d_enu(lat[r], lon[r], e, nn, u);
                const double az = az_[r] * kPi / 180.;
                const double el = el_[r] * kPi / 180.;
                const double ce = cos(el);
                const double q0 = ce * sin(az), q1 = ce * cos(az), q2 = sin(el);
                for (int i = 0; i < 3; i++)
                        dir[3 * r + i] = q0 * e[i] + q1 * nn[i] + q2 * u[i];
        }
}

/* [ref ecef.c:178-207] */
__global__ void k_ecef_to_horizontal(long n, const double * __restrict__ lat,
    const double * __restrict__ lon, const double * __restrict__ dir,
    double * __restrict__ az, double * __restrict__ el)
{
        for (long r = blockIdx.x * (long)blockDim.x + threadIdx.x; r < n;
             r += (long)gridDim.x * blockDim.x) {
                double e[3], nn[3], u[3];
                d_enu(lat[r], lon[r], e, nn, u);
                const double d0 = dir[3 * r], d1 = dir[3 * r + 1], d2 = dir[3 * r + 2];
                const double x = e[0] * d0 + e[1] * d1 + e[2] * d2;
                const double y = nn[0] * d0 + nn[1] * d1 + nn[2] * d2;
                const double z = u[0] * d0 + u[1] * d1 + u[2] * d2;
                double rr = d0 * d0 + d1 * d1 + d2 * d2;
                if (rr <= FLT_EPSILON) continue; /* outputs untouched [ref ecef.c:194] */
                rr = sqrt(rr);
                if (az) az[r] = atan2(x, y) * 180. / kPi;
                if (el) {
                        const double arg = z / rr;
                        el[r] = (arg > 1.) ? 90. :
                                             ((arg < -1.) ? -90. : asin(arg) * 180. / kPi);
                }
        }
}

/* Elevation of n points on the view's first meta.  For a MAP the arguments
 * are (x, y) [ref map.c:380-385]; for a STACK (latitude, longitude)
 * [ref stack.c:338-361]. */
__global__ void k_elevation(tamd_view v, long n, const double * __restrict__ a,
    const double * __restrict__ b, double * __restrict__ z, int * __restrict__ inside, Paging pg)
{
        const tamd_meta mt = v.metas[0];
        PAGED_ITEMS(pg, n, i0, r)
        {
                int in = 0;
                TileFault f = { -1, 0, 0 };
                if (r >= 0) {
                        double zz = 0.;
                        if (mt.kind == TAMD_MAP)
                                in = d_grid_elevation(v.grids[mt.src], a[r], b[r], zz) ? 1 : 0;
                        else
                                in = d_stack_elevation(v, v.stacks[mt.src], a[r], b[r], zz, f);
                        if (in >= 0) f.centre = -1;
                        if (in >= 0) {
                                /* an outside point leaves a MAP's z untouched in the
                                 * reference and zeroes a STACK's; report 0 for both */
                                z[r] = in ? zz : 0.;
                                inside[r] = in;
                        }
                }
                if (pg.faulted != nullptr) page_fault(pg, f, r);
        }
}

/* Gradient of n points on the view's first meta: a MAP takes (x, y) and
 * returns (gx, gy) [ref map.c:387-392]; a STACK takes (latitude, longitude)
 * and returns (glat, glon) [ref stack.c:364-388].  Outputs are in-out. */
__global__ void k_gradient(tamd_view v, long n, const double * __restrict__ a,
    const double * __restrict__ b, double * __restrict__ ga, double * __restrict__ gb,
    int * __restrict__ inside, Paging pg)
{
        const tamd_meta mt = v.metas[0];
        PAGED_ITEMS(pg, n, i0, r)
        {
                int tile = 0;
                TileFault f = { -1, 0, 0 };
                if (r >= 0) {
                        bool in = false;
                        if (mt.kind == TAMD_MAP) {
                                double gx = ga[r], gy = gb[r];
                                in = d_grid_gradient(v.grids[mt.src], a[r], b[r], gx, gy);
                                ga[r] = gx, gb[r] = gy;
                        } else {
                                tile = d_stack_tile(v, v.stacks[mt.src], a[r], b[r], f);
                                if (tile != kTileFault) f.centre = -1;
                                if (tile == -1) {
                                        ga[r] = gb[r] = 0.; /* [ref stack.c:378-382] */
                                } else if (tile >= 0) {
                                        double glat = ga[r], glon = gb[r];
                                        /* x = longitude, y = latitude; gx -> glon, gy -> glat */
                                        in = d_grid_gradient(v.grids[tile], b[r], a[r], glon, glat);
                                        ga[r] = glat, gb[r] = glon;
                                }
                        }
                        if (tile != kTileFault) inside[r] = in ? 1 : 0;
                }
                if (pg.faulted != nullptr) page_fault(pg, f, r);
        }
}

/* [ref stepper.c:877-931] */
__global__ void k_position(tamd_view v, long n, const double * __restrict__ lat,
    const double * __restrict__ lon, const double * __restrict__ height, int layer,
    double * __restrict__ pos, int * __restrict__ data_index, Paging pg)
{
        PAGED_ITEMS(pg, n, i0, r)
        {
                TileFault fault = { -1, 0, 0 };
                if (r >= 0) {
                        const double la = lat[r], lo = lon[r];
                        int found = -1, di = 0;
                        double elevation = 0.;
                        const int end = v.layer_first[layer + 1];
                        for (int j = v.layer_first[layer]; j < end; j++, di++) {
                                const tamd_meta mt = v.metas[j];
                                TileFault f;
                                const int in = d_source_elevation(v, mt, la, lo, elevation, f);
                                if (in < 0) {
                                        fault = f;
                                        break;
                                }
                                if (in == 0) continue;
                                elevation += mt.offset;
                                if (v.geoid >= 0) { /* [ref stepper.c:905-914] */
                                        double undulation;
                                        const double l360 = (lo >= 0) ? lo : lo + 360.;
                                        if (d_grid_elevation(
                                                v.grids[v.geoid], l360, la, undulation))
                                                elevation += undulation;
                                }
                                found = di;
                                break;
                        }
                        if (fault.centre < 0) {
                                data_index[r] = found;
                                if (found >= 0) {
                                        double x, y, z;
                                        d_from_geodetic(la, lo, elevation + height[r], x, y, z);
                                        pos[3 * r] = x, pos[3 * r + 1] = y, pos[3 * r + 2] = z;
                                }
                        }
                }
                if (pg.faulted != nullptr) page_fault(pg, fault, r);
        }
}

/* turtle_stepper_normal_n: the normal of the top of layer[r] above or below pos[r], one point per
 * lane; the arithmetic is normal()'s of turtle_amd_device.h, always the strict one.  A point with
 * no data there (or no such layer) gets data_index -1 and keeps its row of `out`. */
template <int MODE>
__global__ void __launch_bounds__(256) k_normal(tamd_view v, long n, const double * __restrict__ pos,
    const int * __restrict__ layer, double * __restrict__ out, int * __restrict__ data_index, Paging pg)
{
        const Geometry<MODE, STRICT> geo(v);
        PAGED_ITEMS(pg, n, i0, r)
        {
                TileFault fault = { -1, 0, 0 };
                if (r >= 0) {
                        const double p[3] = { pos[3 * r], pos[3 * r + 1], pos[3 * r + 2] };
                        double w[3];
                        TileFault f = { -1, 0, 0 };
                        const int found = normal(geo, p, layer[r], w, &f);
                        if (found == kTileFault) {
                                fault = f;
                        } else {
                                data_index[r] = found;
                                if (found >= 0) out[3 * r] = w[0], out[3 * r + 1] = w[1], out[3 * r + 2] = w[2];
                        }
                }
                if (pg.faulted != nullptr) page_fault(pg, fault, r);
        }
}
} /* namespace */

extern "C" int tamd_k_ecef_from_geodetic(long n, const double * lat,
    const double * lon, const double * elev, double * ecef)
{
        return launch_items("k_ecef_from_geodetic", k_ecef_from_geodetic, n, 0, n, lat, lon, elev, ecef);
}

extern "C" int tamd_k_ecef_to_geodetic(
    long n, const double * ecef, double * lat, double * lon, double * alt)
{
        return with_math(g_math_strict, [&](auto fast) {
                return launch_items("k_ecef_to_geodetic", k_ecef_to_geodetic<decltype(fast)::value>, n, 0, n,
                    ecef, lat, lon, alt);
        });
}

extern "C" int tamd_k_ecef_from_horizontal(long n, const double * lat,
    const double * lon, const double * az, const double * el, double * dir)
{
        return launch_items("k_ecef_from_horizontal", k_ecef_from_horizontal, n, 0, n, lat, lon, az, el, dir);
}

extern "C" int tamd_k_ecef_to_horizontal(long n, const double * lat,
    const double * lon, const double * dir, double * az, double * el)
{
        return launch_items("k_ecef_to_horizontal", k_ecef_to_horizontal, n, 0, n, lat, lon, dir, az, el);
}

extern "C" int tamd_k_elevation(struct tamd_view view, long n, const double * a,
    const double * b, double * z, int * inside, struct tamd_paging pg)
{
        return launch_items("k_elevation", k_elevation, n, 0, view, n, a, b, z, inside, pg);
}

extern "C" int tamd_k_gradient(struct tamd_view view, long n, const double * a,
    const double * b, double * ga, double * gb, int * inside, struct tamd_paging pg)
{
        return launch_items("k_gradient", k_gradient, n, 0, view, n, a, b, ga, gb, inside, pg);
}

extern "C" int tamd_k_position(struct tamd_view view, long n, const double * lat,
    const double * lon, const double * height, int layer, double * pos,
    int * data_index, struct tamd_paging pg)
{
        return launch_items("k_position", k_position, n, 0, view, n, lat, lon, height, layer, pos,
            data_index, pg);
}

extern "C" int tamd_k_normal(struct tamd_view view, long n, const double * pos, const int * layer,
    double * normal, int * data_index, struct tamd_paging pg)
{
        return with_mode(view.mode, [&](auto mode) {
                return launch_items("k_normal", k_normal<decltype(mode)::value>, n, 0, view, n, pos, layer,
                    normal, data_index, pg);
        });
}
