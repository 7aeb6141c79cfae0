/*
 * rays.hip -- a ray per lane through every medium, from its origin to its end, and the launchers.
 * The arithmetic contract and the citations [ref FILE:LINE] are device.hip's (see its header).
 *
 *   k_traverse      a line of sight per ray through every medium, every tile resident
 *                   (turtle_stepper_traverse_n; <REC>: turtle_stepper_crossings_n)
 *   k_advance       the same advanced by a column-depth budget (turtle_stepper_advance_n; <LAW>:
 *                   _advance_exp_n; <GRID>: _advance_grid_n)
 *   k_traverse_gen, k_crossings_gen   a traverse over paged stacks: the accounting after each
 *                   generation of k_step + k_bisect (device.hip)
 */
#include <hip/hip_runtime.h>

#include <cmath>
#include <type_traits>

#include "device_common.h"
#include "device_launch.h"

namespace {

/* ---- a line of sight per ray ------------------------------------------------
 *
 * turtle_stepper_traverse_n over a geometry with every tile resident: the loop
 * of examples/example-stepper.c:128-140 [ref], one ray per lane from its origin
 * sample to its last step.  k_walk's state machine (one sample per live lane and
 * trip, STEP and BISECT bookkeeping as selects, the crossing located by halving
 * and the ray going on in the new medium from the bisection's last sample) with
 * a fixed direction, a third state for the origin sample (ST_INIT: q = B), the
 * ceiling compared with the altitude turtle_stepper_step publishes (the step's
 * sample after an accepted step, b_alt after a located crossing), and the path
 * summed per medium: the running sum of the medium the ray is in is kept in a
 * register, stored to length[m][r] when a crossing is located and the new
 * medium's total loaded from length[m'][r] -- one load and one store a crossing,
 * the reference's order of additions, and registers independent of the number
 * of media.  Every lane ends through max_steps, the halving guard or the queue
 * running dry.
 * The kernel keeps its OWN copy of the refill loop (queue_refill, device_common.h) and of the select
 * block (step_or_bisect, turtle_amd_device.h), expression for expression: built on the shared ones its
 * 12 instances kept their resources and their results, but scripts/exp_traverse.py measured
 * three of four figures outside the margin (profiles/step_machine_ab.txt).  A change to either
 * has to be made here too; tests/test_gpu_device_api.py and test_gpu_step_machine.py hold this
 * copy to Stepping::trip(), which runs the shared one, bit for bit. */
struct TraverseIO {
        const double * __restrict__ dir;
        double * __restrict__ length; /* [media][n], zeroed by the driver; or NULL */
        int * __restrict__ n_steps;   /* or NULL */
        int * __restrict__ n_cross;   /* or NULL */
        double ceiling;
        int max_steps;
};

/* REC (turtle_stepper_crossings_n): one more register, the ray's total path `tot`, summed as len
 * is (an accepted step's ds, a located crossing's ds + ds1), and each located crossing stored into
 * slot `crossings` of the [capacity][n] arrays (the new position, tot, {m, bm}) before the count
 * goes up.  Nothing else changes: the same decisions and additions, the same bits as REC = false,
 * whose instances take an empty last argument. */
struct NoCrossings {};
template <bool REC> struct CrossingsArg { typedef NoCrossings type; };
template <> struct CrossingsArg<true> { typedef tamd_crossings type; };

template <int MODE, bool FAST, bool REC>
__global__ void __launch_bounds__(256) k_traverse(tamd_view v, long n, double * __restrict__ pos,
    int * __restrict__ index, TraverseIO io, ull * __restrict__ stats, ull * __restrict__ queue,
    typename CrossingsArg<REC>::type rec)
{
        long pool_next = 0, pool_end = 0; /* wave-uniform */
        bool exhausted = false;            /* wave-uniform */
        OneCtx ctx;
        d_load_ctx<MODE, FAST>(v, ctx);
        CellCache cell = { ~0u, 0u, 0u, -1, nullptr };
        CellCache * cache = (FAST && (MODE != TAMD_MODE_GENERIC)) ? &cell : nullptr;

        long ray = -1;
        bool dead = false;
        int state = ST_INIT, count = 0, crossings = 0;
        double bx = 0, by = 0, bz = 0, dx = 0, dy = 0, dz = 0, len = 0;
        double tot = 0; /* (REC) the path since the origin */
        double ds = 0, ds0 = 0, ds1 = 0;
        double s_alt = 0, s_e0 = 0, s_e1 = 0; /* the sample the ray stands on */
        double b_alt = 0, b_e0 = 0, b_e1 = 0; /* the bisection's last sample of the new medium */
        int m = -1, k = -1, bm = -1, bk = -1, halvings = 0;
        ull my_rays = 0, my_steps = 0, my_samples = 0, my_capped = 0;

        for (;;) {
                /* ---- refill idle lanes from the queue (queue_refill's loop, spelt out) ---- */
                for (;;) {
                        const bool need = (ray < 0) && !dead;
                        const ull mask = __ballot(need);
                        if (mask == 0) break;
                        if (pool_next >= pool_end) {
                                if (exhausted) {
                                        if (need) dead = true;
                                        break;
                                }
                                ull base = 0;
                                if ((threadIdx.x & 63) == 0) base = atomicAdd(queue, (ull)kChunk);
                                base = __shfl(base, 0, 64);
                                pool_next = (long)base;
                                pool_end = min((long)base + kChunk, n);
                                if ((long)base >= n) {
                                        exhausted = true;
                                        pool_next = pool_end = 0;
                                }
                                continue;
                        }
                        const long avail = pool_end - pool_next;
                        const int rank = lane_rank(mask);
                        if (need && (rank < avail)) {
                                ray = pool_next + rank;
                                bx = pos[3 * ray], by = pos[3 * ray + 1], bz = pos[3 * ray + 2];
                                dx = io.dir[3 * ray], dy = io.dir[3 * ray + 1], dz = io.dir[3 * ray + 2];
                                state = ST_INIT, count = 0, crossings = 0, len = 0.;
                                if constexpr (REC) tot = 0.;
                        }
                        pool_next += min((long)__popcll(mask), avail);
                }
                if (__ballot(ray >= 0) == 0) break; /* (a lane that drew nothing is dead: so are all) */
                if (ray >= 0) {
                        /* ---- one sample at q = B + d * t (the origin itself first) ---- */
                        const bool init = (state == ST_INIT);
                        const bool stepping = (state == ST_STEP);
                        const double t = stepping ? ds : 0.5 * (ds0 + ds1);
                        const double qx = init ? bx : bx + dx * t, qy = init ? by : by + dy * t,
                                     qz = init ? bz : bz + dz * t;
                        Sample s;
                        d_sample<MODE, FAST>(v, ctx, qx, qy, qz, s, cache);
                        my_samples++;
                        bool ended = false;
                        if (init) { /* [ref stepper.c:780-796] the loop's first call */
                                m = s.m, k = s.k;
                                s_alt = s.alt, s_e0 = s.e0, s_e1 = s.e1;
                                state = ST_STEP;
                                ended = true;
                        } else {
                                /* ---- bookkeeping: step_or_bisect()'s selects, spelt out ---- */
                                const bool same = (s.m == m);
                                const bool accept = stepping & same;
                                const bool cross = stepping & !same;
                                const bool other = !same;
                                bx = stepping ? qx : bx, by = stepping ? qy : by, bz = stepping ? qz : bz;
                                bm = other ? s.m : bm, bk = other ? s.k : bk;
                                b_alt = other ? s.alt : b_alt, b_e0 = other ? s.e0 : b_e0, b_e1 = other ? s.e1 : b_e1;
                                ds0 = cross ? -ds : ((!stepping & same) ? t : ds0);
                                ds1 = cross ? 0. : ((!stepping & other) ? t : ds1);
                                halvings = stepping ? 0 : halvings + 1;
                                state = cross ? ST_BISECT : state;
                                my_steps += stepping ? 1 : 0;
                                const bool located = (state == ST_BISECT) & !cross &
                                    (!(ds1 - ds0 > 1E-08) | (halvings > 1200));
                                ended = accept;
                                if (accept) {
                                        len += ds, k = s.k;
                                        s_alt = s.alt, s_e0 = s.e0, s_e1 = s.e1;
                                        if constexpr (REC) tot += ds;
                                }
                                if (located) { /* [ref stepper.c:861-863] */
                                        bx = bx + dx * ds1, by = by + dy * ds1, bz = bz + dz * ds1;
                                        len += ds + ds1;
                                        if constexpr (REC) {
                                                tot += ds + ds1;
                                                if (crossings < rec.capacity) { /* slot [crossings][ray] */
                                                        const long c = (long)crossings * n + ray;
                                                        if (rec.point != nullptr)
                                                                rec.point[3 * c] = bx, rec.point[3 * c + 1] = by,
                                                                rec.point[3 * c + 2] = bz;
                                                        if (rec.distance != nullptr) rec.distance[c] = tot;
                                                        if (rec.media != nullptr)
                                                                rec.media[2 * c] = m, rec.media[2 * c + 1] = bm;
                                                }
                                        }
                                        /* the sum of the medium left goes out, the new one's comes in */
                                        if (io.length != nullptr) {
                                                io.length[(long)m * n + ray] = len;
                                                len = (bm >= 0) ? io.length[(long)bm * n + ray] : 0.;
                                        }
                                        m = bm, k = bk;
                                        s_alt = b_alt, s_e0 = b_e0, s_e1 = b_e1;
                                        crossings++;
                                        state = ST_STEP;
                                        ended = true;
                                }
                                count += ended ? 1 : 0;
                        }
                        if (ended) { /* a step is over (or the origin sampled): the loop's test */
                                const bool low = (m >= 0) && (s_alt < io.ceiling);
                                if (!low || (count >= io.max_steps)) {
                                        pos[3 * ray] = bx, pos[3 * ray + 1] = by, pos[3 * ray + 2] = bz;
                                        index[2 * ray] = m, index[2 * ray + 1] = k;
                                        if ((io.length != nullptr) && (m >= 0)) io.length[(long)m * n + ray] = len;
                                        if (io.n_steps != nullptr) io.n_steps[ray] = count;
                                        if (io.n_cross != nullptr) io.n_cross[ray] = crossings;
                                        my_rays++;
                                        my_capped += low ? 1 : 0;
                                        ray = -1;
                                } else {
                                        ds = d_step_length(v, s_alt, s_e0, s_e1, m);
                                }
                        }
                }
        }
        block_tally(stats, my_rays, my_steps, my_samples, my_capped);
}

/* ---- a ray advanced by a column-depth budget ----------------------------------
 *
 * turtle_stepper_advance_n over a geometry with every tile resident: traverse_n's
 * loop (include/turtle_amd.h states it), one ray per lane, with two more ways to
 * end: the column depth X = sum of density[medium] x step has reached the ray's
 * budget B, or the path d its limit M.  Built on the shared machine as k_walk is
 * (queue_refill, step_or_bisect), with k_traverse's third state for the origin
 * sample.  An EVENT is an accepted step or a located crossing: there, and only
 * there, the lane does the definition's bookkeeping with the density of the medium
 * the step started in (read from density[] when the ray enters a medium: a load at
 * every step sat on each lane's chain); while it halves a crossing
 * nothing is tested, and the step's full length ds + ds1 is one value
 * (k_traverse<REC>'s tot += ds + ds1: the same bits).  A step that would reach B or
 * M is cut short: the ray ends at p0 + dir * f, p0 the position the step began at.
 * A lane keeps X, d, B, M and that density over what a k_traverse lane keeps; p0
 * costs nothing: for an accepted step it is the trip's own starting point, and
 * while a crossing is halved it lies in the registers of the sample the ray stood
 * on, which is dead by then.  The tests after an event are traverse's in
 * traverse's order with the two budget tests between them; with B = inf and no M
 * they never fire: the bits of k_traverse.
 *
 * LAW (turtle_stepper_advance_exp_n with scale heights): the density of medium m at
 * altitude h is density[m] * exp(-h / scale_height[m]), the altitude taken as linear
 * in the path within a step.  A LAW lane keeps two values more: ih, the reciprocal of
 * its medium's scale height (0: the medium is uniform), read with rho when the ray
 * enters a medium; and a0, the altitude its step began at, for the time a crossing is
 * halved (s_alt holds p0x then; for an accepted step a0 is still in s_alt at the
 * event).  exp, expm1 and log1p run at events only, the plain double-precision
 * functions in either arithmetic, and a lane whose medium is uniform branches past
 * them: its bits are those of the instance without the law.  The step's depth and its
 * inverse are turtle_amd_device.h's column_depth and column_reach.
 *
 * GRID (turtle_stepper_advance_grid_n): inside a box of voxels the density of ONE
 * medium is the voxel's.  At an event a lane whose medium is the grid's walks the
 * step's segment p0 + dir * [0, L] voxel by voxel (turtle_amd_device.h's grid_depth:
 * the one copy of the arithmetic), L being the step's length or what the distance
 * limit leaves of it; the walk itself stops where the budget runs out, so the far
 * cut and the depth cut come out of one walk.  p0 is where the kernel keeps it
 * anyway (above).  A lane in another medium branches past the walk inside
 * grid_depth: one piece at rho.  The grid's scalars ride in the kernel argument
 * (scalar registers); the voxel loads are the only new memory traffic.  The walk's
 * state lives inside the event only. */
struct AdvanceIO {
        const double * __restrict__ dir;
        const double * __restrict__ density;  /* [media] */
        const double * __restrict__ budget;   /* [n] */
        const double * __restrict__ dist_max; /* [n] or NULL */
        double * __restrict__ depth;          /* or NULL */
        double * __restrict__ distance;       /* or NULL */
        int * __restrict__ n_steps;           /* or NULL */
        int * __restrict__ status;
        double ceiling;
        int max_steps;
};
struct AdvanceLawIO : AdvanceIO {
        const double * __restrict__ scale_height; /* [media] */
};
struct AdvanceGridIO : AdvanceIO {
        turtle_amd_grid_view grid;
};

/* what a LAW lane keeps of its medium's scale height H: 1 / H, and 0 for the uniform H = HUGE_VAL */
__device__ __forceinline__ double d_inverse_scale(double H) { return (H == HUGE_VAL) ? 0. : 1. / H; }

template <int MODE, bool FAST, bool LAW = false, bool GRID = false>
__global__ void __launch_bounds__(256) k_advance(tamd_view v, long n, double * __restrict__ pos,
    int * __restrict__ index,
    std::conditional_t<GRID, AdvanceGridIO, std::conditional_t<LAW, AdvanceLawIO, AdvanceIO>> io,
    ull * __restrict__ stats, ull * __restrict__ queue)
{
        static_assert(!(LAW && GRID), "a grid together with scale heights is not offered");
        RayQueue q;
        OneCtx ctx;
        d_load_ctx<MODE, FAST>(v, ctx);
        CellCache cell = { ~0u, 0u, 0u, -1, nullptr };
        CellCache * cache = (FAST && (MODE != TAMD_MODE_GENERIC)) ? &cell : nullptr;

        long ray = -1;
        bool dead = false;
        int state = ST_INIT, count = 0;
        double bx = 0, by = 0, bz = 0, dx = 0, dy = 0, dz = 0;
        double X = 0, d = 0, B = 0, M = 0;
        double rho = 0; /* density[m]: read when the ray enters a medium, not at every step */
        double ih = 0, a0 = 0; /* (LAW) 1 / scale_height[m], or 0: uniform; the altitude a halved step began at */
        double ds = 0;
        /* the sample the ray stands on -- and, while it halves a crossing (ds is set, the sample
         * no longer needed: an event replaces it), the position p0 its step began at */
        double s_alt = 0, s_e0 = 0, s_e1 = 0;
        Bisection b = { 0., 0., 0., 0., 0., -1, -1, 0 };
        int m = -1, k = -1;
        ull my_rays = 0, my_steps = 0, my_samples = 0, my_capped = 0;

        for (;;) {
                queue_refill(q, queue, kChunk, n, ray, dead, [&] {
                        bx = pos[3 * ray], by = pos[3 * ray + 1], bz = pos[3 * ray + 2];
                        dx = io.dir[3 * ray], dy = io.dir[3 * ray + 1], dz = io.dir[3 * ray + 2];
                        B = io.budget[ray];
                        M = (io.dist_max != nullptr) ? io.dist_max[ray] : HUGE_VAL;
                        state = ST_INIT, count = 0, X = 0., d = 0.;
                });
                if (__ballot(ray >= 0) == 0) break; /* (a lane that drew nothing is dead: so are all) */
                if (ray >= 0) {
                        /* ---- one sample at q = B + d * t (the origin itself first) ---- */
                        const bool init = (state == ST_INIT);
                        const bool stepping = (state == ST_STEP);
                        const double t = stepping ? ds : 0.5 * (b.ds0 + b.ds1);
                        const double qx = init ? bx : bx + dx * t, qy = init ? by : by + dy * t,
                                     qz = init ? bz : bz + dz * t;
                        Sample s;
                        d_sample<MODE, FAST>(v, ctx, qx, qy, qz, s, cache);
                        my_samples++;
                        bool event = false;
                        int status = -1; /* set: the ray ends */
                        if (init) { /* [ref stepper.c:780-796] the loop's first call */
                                m = s.m, k = s.k;
                                s_alt = s.alt, s_e0 = s.e0, s_e1 = s.e1;
                                if (m >= 0) rho = io.density[m];
                                if constexpr (LAW) {
                                        if (m >= 0) ih = d_inverse_scale(io.scale_height[m]);
                                }
                                state = ST_STEP;
                                event = true;
                        } else {
                                /* ---- bookkeeping: the step machine of turtle_amd_device.h ---- */
                                const double ox = bx, oy = by, oz = bz; /* (stepping: where the step begins) */
                                const StepOutcome o = step_or_bisect(b, state, bx, by, bz, m, ds, t, qx, qy, qz, s);
                                my_steps += stepping ? 1 : 0;
                                event = o.accept | o.located;
                                if constexpr (LAW) {
                                        if (stepping & !o.accept) a0 = s_alt;
                                }
                                if (stepping & !o.accept) s_alt = ox, s_e0 = oy, s_e1 = oz; /* p0, kept for the halving */
                                if (event) {
                                        const double p0x = o.accept ? ox : s_alt, p0y = o.accept ? oy : s_e0,
                                                     p0z = o.accept ? oz : s_e1;
                                        /* the step's full length, in the medium m it started in */
                                        const double len = o.located ? ds + b.ds1 : ds;
                                        double x = rho * len;
                                        double c = rho, w = 0.; /* the step's law: column_depth(c, w, f) */
                                        if constexpr (LAW) {
                                                if (ih != 0.) {
                                                        const double h0 = o.accept ? s_alt : a0;
                                                        const double h1 = o.accept ? s.alt : b.b_alt;
                                                        c = rho * exp(-h0 * ih);
                                                        w = -((h1 - h0) * ih) / len;
                                                        x = column_depth(c, w, len);
                                                }
                                        }
                                        GridDepth walk = { 0., 0., false };
                                        if constexpr (GRID) {
                                                /* one walk over what the limit leaves of the step: its depth, or where
                                                 * the budget runs out inside it (walk.f: there, or the whole of L) */
                                                double L = (d + len >= M) ? M - d : len;
                                                if (L > len) L = len;
                                                walk = grid_depth(io.grid, rho, m, p0x, p0y, p0z, dx, dy, dz, L, B - X);
                                                x = walk.x;
                                        }
                                        const bool spent = GRID ? walk.stopped : (X + x >= B), far = (d + len >= M);
                                        count++;
                                        if (spent | far) { /* the step is cut short, inside medium m */
                                                if constexpr (GRID) {
                                                        const double f = walk.f;
                                                        status = spent ? TURTLE_AMD_ADVANCE_SPENT : TURTLE_AMD_ADVANCE_DISTANCE;
                                                        bx = p0x + dx * f, by = p0y + dy * f, bz = p0z + dz * f;
                                                        X = spent ? B : X + x;
                                                        d = spent ? d + f : M;
                                                } else {
                                                        double f = far ? M - d : len;
                                                        status = far ? TURTLE_AMD_ADVANCE_DISTANCE : TURTLE_AMD_ADVANCE_SPENT;
                                                        if (spent) {
                                                                const double fs = LAW ? column_reach(c, w, B - X) : (B - X) / rho;
                                                                if (fs <= f) f = fs, status = TURTLE_AMD_ADVANCE_SPENT;
                                                        }
                                                        if (f > len) f = len; /* (a rounding guard) */
                                                        bx = p0x + dx * f, by = p0y + dy * f, bz = p0z + dz * f;
                                                        const bool by_depth = (status == TURTLE_AMD_ADVANCE_SPENT);
                                                        X = by_depth ? B : X + (LAW ? column_depth(c, w, f) : rho * f);
                                                        d = by_depth ? d + f : M;
                                                }
                                        } else {
                                                X += x, d += len;
                                                if (o.accept) {
                                                        k = s.k;
                                                        s_alt = s.alt, s_e0 = s.e0, s_e1 = s.e1;
                                                } else { /* [ref stepper.c:861-863] */
                                                        bx = bx + dx * b.ds1, by = by + dy * b.ds1, bz = bz + dz * b.ds1;
                                                        m = b.bm, k = b.bk;
                                                        s_alt = b.b_alt, s_e0 = b.b_e0, s_e1 = b.b_e1;
                                                        if (m >= 0) rho = io.density[m];
                                                        if constexpr (LAW) {
                                                                if (m >= 0) ih = d_inverse_scale(io.scale_height[m]);
                                                        }
                                                }
                                        }
                                        state = ST_STEP;
                                }
                        }
                        if (event) { /* a step is over (or the origin sampled): the loop's tests */
                                if (status < 0) {
                                        if (m < 0) status = TURTLE_AMD_ADVANCE_LEFT;
                                        else if (!(X < B)) status = TURTLE_AMD_ADVANCE_SPENT;
                                        else if (!(d < M)) status = TURTLE_AMD_ADVANCE_DISTANCE;
                                        /* (s_alt, s_e0, s_e1: after an event always the sample again, never p0) */
                                        else if (!(s_alt < io.ceiling)) status = TURTLE_AMD_ADVANCE_CEILING;
                                        else if (count >= io.max_steps) status = TURTLE_AMD_ADVANCE_MAX_STEPS;
                                }
                                if (status >= 0) {
                                        pos[3 * ray] = bx, pos[3 * ray + 1] = by, pos[3 * ray + 2] = bz;
                                        index[2 * ray] = m, index[2 * ray + 1] = k;
                                        if (io.depth != nullptr) io.depth[ray] = X;
                                        if (io.distance != nullptr) io.distance[ray] = d;
                                        if (io.n_steps != nullptr) io.n_steps[ray] = count;
                                        io.status[ray] = status;
                                        my_rays++;
                                        my_capped += (status == TURTLE_AMD_ADVANCE_MAX_STEPS) ? 1 : 0;
                                        ray = -1;
                                } else {
                                        ds = d_step_length(v, s_alt, s_e0, s_e1, m);
                                }
                        }
                }
        }
        block_tally(stats, my_rays, my_steps, my_samples, my_capped);
}

/* After one generation of a paged traverse (or, `first`, after the origins were
 * sampled): the step each live ray took added to the sum of the medium it
 * started in, the loop's test, and the rays it ends taken out of the stepping
 * (live_index[r][0] = -1; their results are in index).  medium[r]: the medium a
 * live ray is in, -1 once it is done. */
__global__ void k_traverse_gen(long n, int first, const double * __restrict__ alt,
    const double * __restrict__ step, int * __restrict__ live_index, int * __restrict__ medium,
    int * __restrict__ index, double * __restrict__ length, int * __restrict__ n_steps,
    int * __restrict__ n_cross, double ceiling, int max_steps, ull * __restrict__ counters)
{
        ull my_rays = 0, my_steps = 0, my_capped = 0, my_live = 0;
        for (long r = blockIdx.x * (long)blockDim.x + threadIdx.x; r < n;
             r += (long)gridDim.x * blockDim.x) {
                const int m1 = live_index[2 * r];
                int count = 0;
                if (first) {
                        n_steps[r] = 0, n_cross[r] = 0;
                } else {
                        const int m0 = medium[r];
                        if (m0 < 0) continue; /* done earlier */
                        if (length != nullptr) length[(long)m0 * n + r] += step[r];
                        count = n_steps[r] + 1;
                        n_steps[r] = count;
                        n_cross[r] += (m1 != m0) ? 1 : 0;
                        my_steps++;
                }
                index[2 * r] = m1, index[2 * r + 1] = live_index[2 * r + 1];
                const bool low = (m1 >= 0) && (alt[r] < ceiling);
                if (!low || (count >= max_steps)) {
                        medium[r] = -1, live_index[2 * r] = -1;
                        my_rays++;
                        my_capped += low ? 1 : 0;
                } else {
                        medium[r] = m1;
                        my_live++;
                }
        }
        block_tally(counters, my_rays, my_steps, my_capped, my_live);
}

/* A paged turtle_stepper_crossings_n, after a generation's steps and before its k_traverse_gen
 * (which still holds the medium each live ray started in, and its crossing count): the step added
 * to the ray's running total, and a ray whose medium changed (m1 != m0) records its new position,
 * that total and {m0, m1} in slot n_cross[r].  k_traverse<REC>'s additions: the same bits. */
__global__ void k_crossings_gen(long n, const double * __restrict__ pos, const double * __restrict__ step,
    const int * __restrict__ live_index, const int * __restrict__ medium, const int * __restrict__ n_cross,
    double * __restrict__ total, tamd_crossings rec)
{
        for (long r = blockIdx.x * (long)blockDim.x + threadIdx.x; r < n;
             r += (long)gridDim.x * blockDim.x) {
                const int m0 = medium[r];
                if (m0 < 0) continue; /* done earlier */
                const double tot = total[r] + step[r];
                total[r] = tot;
                const int m1 = live_index[2 * r];
                if ((m1 != m0) && (n_cross[r] < rec.capacity)) {
                        const long c = (long)n_cross[r] * n + r;
                        if (rec.point != nullptr)
                                rec.point[3 * c] = pos[3 * r], rec.point[3 * c + 1] = pos[3 * r + 1],
                                rec.point[3 * c + 2] = pos[3 * r + 2];
                        if (rec.distance != nullptr) rec.distance[c] = tot;
                        if (rec.media != nullptr) rec.media[2 * c] = m0, rec.media[2 * c + 1] = m1;
                }
        }
}
} /* namespace */

template <int MODE, bool REC>
static int launch_traverse(const tamd_view & view, long n, double * pos, int * index, const TraverseIO & io,
    ull * stats, ull * queue, bool strict, typename CrossingsArg<REC>::type rec)
{
        return with_math(strict, [&](auto fast) {
                const auto kernel = k_traverse<MODE, decltype(fast)::value, REC>;
                return launch_blocks("k_traverse", kernel, persistent_blocks(kernel, n), 0, view, n, pos, index, io,
                    stats, queue, rec);
        });
}

/* A whole traverse in one launch (k_traverse): every tile resident, nothing listed */
extern "C" int tamd_k_traverse(struct tamd_view view, long n, double * pos, const double * dir,
    double ceiling, int max_steps, int * index, double * length, int * n_steps, int * n_cross,
    const struct tamd_crossings * rec, unsigned long long * stats, unsigned long long * queue)
{
        if (tamd_dev_init()) return 1;
        if (zero_words(stats, 4, queue, 1)) return 1;
        if (n <= 0) return 0;
        const TraverseIO io = { dir, length, n_steps, n_cross, ceiling, max_steps };
        const bool strict = strict_math(view);
        return with_mode(view.mode, [&](auto mode) {
                constexpr int MODE = decltype(mode)::value;
                if (rec != nullptr)
                        return launch_traverse<MODE, true>(view, n, pos, index, io, stats, queue, strict, *rec);
                return launch_traverse<MODE, false>(view, n, pos, index, io, stats, queue, strict, NoCrossings());
        });
}

/* A whole advance in one launch (k_advance): every tile resident, nothing listed.  scale_height
 * NULL: the instances without the law; grid (host memory, its density a device pointer) not NULL:
 * the grid instances */
extern "C" int tamd_k_advance(struct tamd_view view, long n, double * pos, const double * dir,
    const double * density, const double * scale_height, const struct turtle_amd_grid_view * grid,
    const double * budget, const double * distance_max,
    double ceiling, int max_steps, int * index, double * depth, double * distance, int * n_steps, int * status,
    unsigned long long * stats, unsigned long long * queue)
{
        if (tamd_dev_init()) return 1;
        if (zero_words(stats, 4, queue, 1)) return 1;
        if (n <= 0) return 0;
        const AdvanceIO io = { dir, density, budget, distance_max, depth, distance, n_steps, status, ceiling,
                max_steps };
        const bool strict = strict_math(view);
        return with_mode(view.mode, [&](auto mode) {
                return with_math(strict, [&](auto fast) {
                        if (scale_height != nullptr) {
                                AdvanceLawIO law;
                                static_cast<AdvanceIO &>(law) = io;
                                law.scale_height = scale_height;
                                const auto kernel = k_advance<decltype(mode)::value, decltype(fast)::value, true>;
                                return launch_blocks("k_advance", kernel, persistent_blocks(kernel, n), 0, view, n,
                                    pos, index, law, stats, queue);
                        }
                        if (grid != nullptr) {
                                AdvanceGridIO g;
                                static_cast<AdvanceIO &>(g) = io;
                                g.grid = *grid;
                                const auto kernel = k_advance<decltype(mode)::value, decltype(fast)::value, false, true>;
                                return launch_blocks("k_advance", kernel, persistent_blocks(kernel, n), 0, view, n,
                                    pos, index, g, stats, queue);
                        }
                        const auto kernel = k_advance<decltype(mode)::value, decltype(fast)::value>;
                        return launch_blocks("k_advance", kernel, persistent_blocks(kernel, n), 0, view, n, pos,
                            index, io, stats, queue);
                });
        });
}

extern "C" int tamd_k_traverse_gen(long n, int first, const double * alt, const double * step,
    int * live_index, int * medium, int * index, double * length, int * n_steps, int * n_cross,
    double ceiling, int max_steps, unsigned long long * counters)
{
        return launch_items("k_traverse_gen", k_traverse_gen, n, 0, n, first, alt, step, live_index, medium,
            index, length, n_steps, n_cross, ceiling, max_steps, counters);
}

extern "C" int tamd_k_crossings_gen(long n, const double * pos, const double * step, const int * live_index,
    const int * medium, const int * n_cross, double * total, struct tamd_crossings rec)
{
        return launch_items("k_crossings_gen", k_crossings_gen, n, 0, n, pos, step, live_index, medium, n_cross,
            total, rec);
}
