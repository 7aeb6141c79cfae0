/*
 * sight.hip -- lines of sight over a layer's top, one wave a line, and their launchers.  The
 * arithmetic contract and the citations [ref FILE:LINE] are device.hip's (see its header).
 *
 *   k_horizon       the skyline around observers, one wave per line of sight: the highest of a
 *                   line's samples of a layer's top (turtle_stepper_horizon_n)
 *   k_viewshed      which samples of those lines the observer sees: a wave-wide prefix maximum
 *                   over chunks of 64 samples (turtle_stepper_viewshed_n)
 *   k_clearance     the least height of the chord from an observer to a target above a layer's
 *                   top, one wave per line (turtle_stepper_clearance_n)
 */
#include <hip/hip_runtime.h>

#include <cfloat>

#include "device_common.h"
#include "device_launch.h"

namespace {

/* The top of `layer` under (la, lo) as turtle_stepper_position finds it [ref stepper.c:892-914]:
 * the layer's data last added first, the offset, the geoid -- k_position's arithmetic, always the
 * strict one.  false where no data answers; a tile that is not resident answers nothing (the
 * callers run over resident geometry). */
template <int MODE>
__device__ __forceinline__ bool d_layer_top(const tamd_view & v, const OneCtx & ctx, int layer, double la,
    double lo, double & elevation)
{
        TileFault f;
        if (MODE == TAMD_MODE_ONE_MAP) {
                if (!d_grid_elevation<false>(ctx.grid, lo, la, elevation)) return false;
                elevation += ctx.offset;
                return true;
        }
        if (MODE == TAMD_MODE_ONE_STACK) {
                if (d_stack_elevation<false>(v, ctx.stack, la, lo, elevation, f) <= 0) return false;
                elevation += ctx.offset;
                return true;
        }
        const int end = v.layer_first[layer + 1];
        for (int j = v.layer_first[layer]; j < end; j++) {
                const tamd_meta mt = v.metas[j];
                const int in = d_source_elevation(v, mt, la, lo, elevation, f);
                if (in < 0) return false;
                if (in == 0) continue;
                elevation += mt.offset;
                if (v.geoid >= 0) {
                        double undulation;
                        const double l360 = (lo >= 0) ? lo : lo + 360.;
                        if (d_grid_elevation(v.grids[v.geoid], l360, la, undulation)) elevation += undulation;
                }
                return true;
        }
        return false;
}

/* A line of sight of turtle_stepper_horizon_n and _viewshed_n: line a of observer r. */
struct SightLine {
        double p0, p1, p2; /* the observer */
        double u[3];       /* its vertical */
        double h[3];       /* the line's horizontal unit vector: the sample at distance s lies under p + s h */
};

/* The preamble of both kernels: the observer's geodetic coordinates, its frame, and h from the
 * azimuth.  Wave-uniform, computed by every lane.  FAST: the to_geodetic transform only. */
template <bool FAST>
__device__ __forceinline__ void d_sight_line(const double * __restrict__ pos,
    const double * __restrict__ azimuth, long r, int a, SightLine & line)
{
        const double p0 = pos[3 * r], p1 = pos[3 * r + 1], p2 = pos[3 * r + 2];
        double lat0, lon0, alt0;
        if (FAST)
                f_to_geodetic(p0, p1, p2, lat0, lon0, alt0);
        else
                d_to_geodetic(p0, p1, p2, lat0, lon0, alt0);
        double e[3], nn[3];
        d_enu(lat0, lon0, e, nn, line.u);
        { /* turtle_ecef_from_horizontal at elevation 0 [ref ecef.c:160-176] */
                const double az = azimuth[a] * kPi / 180.;
                const double el = 0. * kPi / 180.;
                const double ce = cos(el);
                const double q0 = ce * sin(az), q1 = ce * cos(az), q2 = sin(el);
                for (int j = 0; j < 3; j++) line.h[j] = q0 * e[j] + q1 * nn[j] + q2 * line.u[j];
        }
        line.p0 = p0, line.p1 = p1, line.p2 = p2;
}

/* One sample of a line: the sine of the elevation angle of the layer's top under p + s h as the
 * observer p sees it (`ground`, at `range`), and of the point `height` above it (`target`; the
 * ground's own at height 0).  false where the definition skips the sample: no data there, or a
 * point at the observer itself [ref ecef.c:194].  FAST: the to_geodetic transform only;
 * everything else is the strict arithmetic.
 *
 * CLOSED_LON is the one deliberate difference between the two calls ("The seam"): in
 * FAST arithmetic, true takes the sample's longitude from the closed form's atan2 [ref ecef.c:86],
 * false keeps the fast transform's; STRICT has the closed form's either way.  k_viewshed passes
 * true: a line due north or south of an observer on a whole degree runs ALONG a seam of the tiles,
 * the last ulp of the longitude then says which tile answers -- beside a missing tile, whether a
 * sample has data at all -- and the call reports every sample, so with the reference's expression
 * its flags are the reference's there too.  k_horizon passes false: such a sample changes a
 * skyline only if it was the winner, and its FAST outputs stay what they were.
 *
 * RANGE: `range` is returned (k_horizon); without it (k_viewshed) the parameter is left alone.  The
 * operations are the same, sqrt then `/` (DESIGN 3.14 has what the switch is worth). */
template <int MODE, bool FAST, bool CLOSED_LON, bool RANGE>
__device__ __forceinline__ bool d_sight_sample(const tamd_view & v, const OneCtx & ctx, int layer,
    const SightLine & line, double s, double height, double & ground, double & target, double & range)
{
        const double p0 = line.p0, p1 = line.p1, p2 = line.p2;
        const double x = p0 + s * line.h[0], y = p1 + s * line.h[1], z = p2 + s * line.h[2];
        double la, lo, al, top;
        if (FAST) {
                f_to_geodetic(x, y, z, la, lo, al);
                if (CLOSED_LON && ((x != 0.) || (y != 0.))) lo = atan2(y, x) * 180. / kPi;
        } else
                d_to_geodetic(x, y, z, la, lo, al);
        if (!d_layer_top<MODE>(v, ctx, layer, la, lo, top)) return false;
        double g0, g1, g2;
        d_from_geodetic(la, lo, top + 0., g0, g1, g2);
        double d0 = g0 - p0, d1 = g1 - p1, d2 = g2 - p2;
        double rr = d0 * d0 + d1 * d1 + d2 * d2;
        if (rr <= FLT_EPSILON) return false;
        if (RANGE) {
                range = sqrt(rr);
                ground = (line.u[0] * d0 + line.u[1] * d1 + line.u[2] * d2) / range;
        } else
                ground = (line.u[0] * d0 + line.u[1] * d1 + line.u[2] * d2) / sqrt(rr);
        if (height == 0.) {
                target = ground;
                return true;
        }
        d_from_geodetic(la, lo, top + height, g0, g1, g2);
        d0 = g0 - p0, d1 = g1 - p1, d2 = g2 - p2;
        rr = d0 * d0 + d1 * d1 + d2 * d2;
        if (rr <= FLT_EPSILON) return false;
        target = (line.u[0] * d0 + line.u[1] * d1 + line.u[2] * d2) / sqrt(rr);
        return true;
}

/* turtle_stepper_horizon_n: the skyline around observers.  One WAVE per item i = r * n_az + a
 * (line a of observer r), four items a block; lane l takes the samples k = l, l + 64, ... of the
 * line and keeps its own best (sine of the elevation angle, k + 1, range); the wave then reduces
 * the 64 triples with a butterfly of shuffles under the order "larger sine, then smaller k", which
 * is what the strict `>` of the sequential loop gives, and lane 0 writes.  The observer's preamble
 * (its geodetic coordinates, the frame, the horizontal unit vector) is wave-uniform and computed by
 * every lane.  FAST: the two to_geodetic transforms only; everything else is the strict
 * arithmetic.  No paging: the geometry is resident. */
template <int MODE, bool FAST>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) k_horizon(tamd_view v, int n_items, int n_az, int n_d,
    const double * __restrict__ pos, const double * __restrict__ azimuth,
    const double * __restrict__ distance, int layer, double * __restrict__ elevation,
    int * __restrict__ sample, double * __restrict__ range)
{
        OneCtx ctx;
        d_load_ctx<MODE, false>(v, ctx);
        const int lane = (int)(threadIdx.x & 63);
        const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
        for (long i = blockIdx.x * 4L + wave; i < (long)n_items; i += (long)gridDim.x * 4L) {
                const long r = i / n_az;
                const int a = (int)(i - r * n_az);
                SightLine line;
                d_sight_line<FAST>(pos, azimuth, r, a, line);

                double best = -HUGE_VAL, best_range = 0.;
                int best_k = 0;
                for (int k = lane; k < n_d; k += 64) {
                        /* (set: left undefined where the sample is skipped, they cost 12 to 24 B of scratch) */
                        double arg = 0., same = 0., rr = 0.;
                        if (!d_sight_sample<MODE, FAST, false, true>(v, ctx, layer, line, distance[k], 0., arg, same, rr))
                                continue;
                        if (arg > best) best = arg, best_k = k + 1, best_range = rr; /* (a NaN never wins) */
                }
                for (int off = 32; off > 0; off >>= 1) {
                        const double o_best = __shfl_xor(best, off, 64);
                        const double o_range = __shfl_xor(best_range, off, 64);
                        const int o_k = __shfl_xor(best_k, off, 64);
                        /* (a lane without a sample holds (-inf, 0): it never wins, and loses to any) */
                        if ((o_best > best) || ((o_best == best) && (o_k != 0) && (o_k < best_k)))
                                best = o_best, best_k = o_k, best_range = o_range;
                }
                if (lane == 0) {
                        sample[i] = best_k;
                        if (best_k != 0) {
                                elevation[i] = (best > 1.) ? 90. : ((best < -1.) ? -90. : asin(best) * 180. / kPi);
                                if (range != nullptr) range[i] = best_range;
                        }
                }
        }
}

/* turtle_stepper_viewshed_n: which samples of a line the observer sees.  One WAVE per item
 * i = r * n_az + a as in k_horizon, four items a block, but a line is swept in CHUNKS of 64
 * consecutive samples, k = base + lane: sample k is seen iff the target's sine is not below the
 * maximum of the ground's sines of the samples before it, a prefix maximum.  Per chunk every lane
 * evaluates its sample; an inclusive Hillis-Steele scan over the lanes (__shfl_up by 1 .. 32)
 * gives the maximum up to each lane, the value one lane below (and `carry`, the maximum of the
 * chunks before, wave-uniform) the horizon in front of it.  The chunk loop's bound is wave-uniform
 * and nothing branches around the scan: a lane past the end, a skipped sample and a NaN contribute
 * -HUGE_VAL.  A maximum rounds nothing, and of equal values (+0 and -0) the earlier one is kept
 * as the sequential `>` keeps it: the outputs are the sequential loop's bits.  Lane l writes
 * element base + l of each output; no LDS, no atomics, no scratch. */
template <int MODE, bool FAST>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) k_viewshed(tamd_view v, int n_items, int n_az, int n_d,
    const double * __restrict__ pos, const double * __restrict__ azimuth,
    const double * __restrict__ distance, int layer, double height, signed char * __restrict__ visible,
    double * __restrict__ sine, double * __restrict__ horizon, int * __restrict__ n_visible)
{
        OneCtx ctx;
        d_load_ctx<MODE, false>(v, ctx);
        const int lane = (int)(threadIdx.x & 63);
        const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
        for (long i = blockIdx.x * 4L + wave; i < (long)n_items; i += (long)gridDim.x * 4L) {
                const long r = i / n_az;
                const int a = (int)(i - r * n_az);
                SightLine line;
                d_sight_line<FAST>(pos, azimuth, r, a, line);

                const size_t first = (size_t)i * (size_t)n_d;
                double carry = -HUGE_VAL;
                int count = 0;
                for (int base = 0; base < n_d; base += 64) { /* (wave-uniform: every lane reaches every shuffle) */
                        const int k = base + lane;
                        const bool in = k < n_d;
                        double ground = -HUGE_VAL, target = -HUGE_VAL;
                        bool data = false;
                        if (in) {
                                double rr; /* (RANGE false: not written) */
                                data = d_sight_sample<MODE, FAST, true, false>(v, ctx, layer, line, distance[k], height,
                                    ground, target, rr);
                        }
                        /* (ground == ground: a NaN never raises the horizon) */
                        double inclusive = (data && (ground == ground)) ? ground : -HUGE_VAL;
                        for (int off = 1; off < 64; off <<= 1) {
                                const double lower = __shfl_up(inclusive, off, 64);
                                if (lane >= off) inclusive = (inclusive > lower) ? inclusive : lower;
                        }
                        double before = __shfl_up(inclusive, 1, 64);
                        if (lane == 0) before = -HUGE_VAL;
                        before = (before > carry) ? before : carry;
                        const double last = __shfl(inclusive, 63, 64);
                        carry = (last > carry) ? last : carry;
                        const bool seen = data && (target >= before); /* (a NaN is never seen; grazing is) */
                        count += __popcll(__ballot(seen));
                        if (in) {
                                visible[first + k] = data ? (signed char)seen : (signed char)-1;
                                if (sine != nullptr) sine[first + k] = data ? target : __builtin_nan("");
                                if (horizon != nullptr) horizon[first + k] = before;
                        }
                }
                if ((n_visible != nullptr) && (lane == 0)) n_visible[i] = count;
        }
}

/* turtle_stepper_clearance_n: the minimum clearance of the straight chord from an observer to a
 * target above a layer's top.  One WAVE per item (i = r * n_t + t, or i = r with PAIRED), four
 * items a block, as in k_horizon; lane l takes the samples k = l, l + 64, ... at the fractions
 * fraction[k] of the chord and keeps its own (least clearance, k + 1, number of samples with
 * data); the wave reduces the 64 pairs with a butterfly of shuffles under the order "smaller
 * clearance, then smaller k", which is what the strict `<` of the sequential loop gives, sums the
 * counts, and lane 0 writes.  The chord's ends and their difference are wave-uniform.  A sample's
 * transform is d_sight_sample's with CLOSED_LON (FAST: latitude from the fast transform, longitude
 * from the closed form's atan2, so that a sample has data where the reference says it has);
 * everything else is the strict arithmetic.  The ground under the sample (d_from_geodetic) and the
 * sample's vertical (d_enu's u) are written with the same expressions of the same latitude and
 * longitude: one set of sines and cosines serves both.  No paging: the geometry is resident. */
template <int MODE, bool FAST>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) k_clearance(tamd_view v, int n_items, int n_t, int paired,
    int n_f, const double * __restrict__ observer, const double * __restrict__ target,
    const double * __restrict__ fraction, int layer, double * __restrict__ clearance,
    int * __restrict__ sample, int * __restrict__ n_data)
{
        OneCtx ctx;
        d_load_ctx<MODE, false>(v, ctx);
        const int lane = (int)(threadIdx.x & 63);
        const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
        for (long i = blockIdx.x * 4L + wave; i < (long)n_items; i += (long)gridDim.x * 4L) {
                const long r = paired ? i : i / n_t;
                const long t = paired ? i : i - r * n_t;
                const double p0 = observer[3 * r], p1 = observer[3 * r + 1], p2 = observer[3 * r + 2];
                const double d0 = target[3 * t] - p0, d1 = target[3 * t + 1] - p1, d2 = target[3 * t + 2] - p2;

                double best = HUGE_VAL;
                int best_k = 0, count = 0;
                for (int k = lane; k < n_f; k += 64) {
                        const double f = fraction[k];
                        const double x = p0 + f * d0, y = p1 + f * d1, z = p2 + f * d2;
                        double la, lo, al, top;
                        if (FAST) {
                                f_to_geodetic(x, y, z, la, lo, al);
                                if ((x != 0.) || (y != 0.)) lo = atan2(y, x) * 180. / kPi;
                        } else
                                d_to_geodetic(x, y, z, la, lo, al);
                        if (!d_layer_top<MODE>(v, ctx, layer, la, lo, top)) continue;
                        count++;
                        double g0, g1, g2, e[3], nn[3], u[3];
                        d_from_geodetic(la, lo, top + 0., g0, g1, g2);
                        d_enu(la, lo, e, nn, u);
                        const double c = u[0] * (x - g0) + u[1] * (y - g1) + u[2] * (z - g2);
                        if (c < best) best = c, best_k = k + 1; /* (a NaN never wins) */
                }
                for (int off = 32; off > 0; off >>= 1) {
                        const double o_best = __shfl_xor(best, off, 64);
                        const int o_k = __shfl_xor(best_k, off, 64);
                        count += __shfl_xor(count, off, 64);
                        /* (a lane without a winner holds (+inf, 0): it never wins, and loses to any) */
                        if ((o_best < best) || ((o_best == best) && (o_k != 0) && (o_k < best_k)))
                                best = o_best, best_k = o_k;
                }
                if (lane == 0) {
                        sample[i] = best_k;
                        if (n_data != nullptr) n_data[i] = count;
                        if (best_k != 0) clearance[i] = best;
                }
        }
}
} /* namespace */

/* A kernel over n_items = observers x azimuths lines of sight, one wave each, four to a block:
 * `launch(mode, fast, grid)` names the instance and passes its arguments. */
template <class Launch>
static int launch_sight(struct tamd_view view, int n_items, int n_azimuths, int n_distances, Launch launch)
{
        if (tamd_dev_init()) return 1;
        if ((n_items <= 0) || (n_azimuths <= 0) || (n_distances <= 0)) return 0;
        return with_mode(view.mode, [&](auto mode) {
                return with_math(g_math_strict,
                    [&](auto fast) { return launch(mode, fast, grid_for(64L * n_items, 256)); });
        });
}

extern "C" int tamd_k_horizon(struct tamd_view view, int n_items, int n_azimuths, int n_distances,
    const double * pos, const double * azimuth, const double * distance, int layer, double * elevation,
    int * sample, double * range)
{
        return launch_sight(view, n_items, n_azimuths, n_distances, [&](auto mode, auto fast, auto grid) {
                return launch_blocks("k_horizon", k_horizon<decltype(mode)::value, decltype(fast)::value>, grid, 0,
                    view, n_items, n_azimuths, n_distances, pos, azimuth, distance, layer, elevation, sample, range);
        });
}

/* the same lines, every sample of each written: visible [n_items][n_distances] and the rest */
extern "C" int tamd_k_viewshed(struct tamd_view view, int n_items, int n_azimuths, int n_distances,
    const double * pos, const double * azimuth, const double * distance, int layer, double target_height,
    signed char * visible, double * sine, double * horizon, int * n_visible)
{
        return launch_sight(view, n_items, n_azimuths, n_distances, [&](auto mode, auto fast, auto grid) {
                return launch_blocks("k_viewshed", k_viewshed<decltype(mode)::value, decltype(fast)::value>, grid, 0,
                    view, n_items, n_azimuths, n_distances, pos, azimuth, distance, layer, target_height, visible,
                    sine, horizon, n_visible);
        });
}

/* chords, not fans: n_items lines from observers to targets (item r * n_targets + t, or r alone
 * where paired), the minimum over n_fractions samples of each */
extern "C" int tamd_k_clearance(struct tamd_view view, int n_items, int n_targets, int paired, int n_fractions,
    const double * observer, const double * target, const double * fraction, int layer, double * clearance,
    int * sample, int * n_data)
{
        return launch_sight(view, n_items, n_targets, n_fractions, [&](auto mode, auto fast, auto grid) {
                return launch_blocks("k_clearance", k_clearance<decltype(mode)::value, decltype(fast)::value>, grid, 0,
                    view, n_items, n_targets, paired, n_fractions, observer, target, fraction, layer, clearance,
                    sample, n_data);
        });
}
