/*
 * device.hip -- the hot unit of the gfx950 device layer of libturtle_amd: the kernels
 * of a trace, of a batch of single steps and of a scattering walk, the small ones
 * around them, and the layer that launches them.  The other families have a unit
 * each (points.hip, maps.hip, sight.hip, rays.hip); what the units share is in
 * device_common.h and device_launch.h.  (The calling thread's device, stream and
 * memory: runtime.hip.)  Written for CDNA4 (wave64); no other target is supported.
 *
 * Arithmetic contract: the kernels evaluate the reference's expressions in
 * the reference's operand order in IEEE fp64 (every unit is compiled with
 * -ffp-contract=off, so no FMA is formed across the reference's roundings).
 * +, -, *, / and sqrt are correctly rounded on gfx950, so they agree bit for
 * bit with the x86 reference; sin/cos/asin/acos/atan2 come from ROCm's OCML
 * and may differ from glibc in the last ulp, which is the only source of
 * GPU/CPU differences (<= 1e-9 relative on a path length; the parity bar is
 * 1e-6).  Citations [ref FILE:LINE] are paths under the reference tree.
 *
 * The trace kernel also has a FAST arithmetic (default), a two-phase launch and
 * a cubic Taylor line along each long ray: see the comments at f_to_geodetic,
 * RayLine, PhaseIO and k_trace, and DESIGN.md 3.1.
 *
 * Kernels (one thread = one ray; all are fp64 VALU work with a 4-node
 * 16-bit gather per sample, see DESIGN.md for the roofline of each):
 *   k_step          batch turtle_stepper_step [ref stepper.c:780-875]: the sample and
 *   k_step_fast     the tentative step; rays that crossed a boundary are listed
 *                   (k_step_fast: the fast-math body of the one-map / one-stack
 *                   modes held to 128 registers)
 *   k_bisect        ... and bisected here, packed [ref stepper.c:836-864]
 *   k_trace         persistent-wave trace-to-boundary loop (the hot kernel: trace_body)
 *   k_first         a fast trace's first closed-form steps, flat: a ray a lane
 *   k_cross         the crossings a trace's passes listed, located by halving
 *   k_ray_cells     the cell each ray starts over: the key a large trace orders its rays by
 *   k_walk          a whole scattering walk per ray, in registers (turtle_stepper_scatter_n)
 *   k_isotropic, k_philox   Philox-4x32-10: isotropic directions, raw words (scattering harness)
 *   k_order_count, k_order_place   a trace's hand-over list in the order of its one-byte keys: a
 *                   counting sort between the two passes
 *   k_tally         hit counts + path-length histogram (uint64, exact): a block a CU at the most
 */
#include <hip/hip_runtime.h>
#include <hipcub/device/device_radix_sort.hpp> /* (RoomSort's alone: no other unit pays for it) */

#include <cfloat>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "device_common.h"
#include "device_launch.h"
#include "trace_room.h"

namespace {

/* ======================================================================== */
/*                                 kernels                                  */
/* ======================================================================== */

/* Where a batch of single steps takes its directions from: an array, or -- a
 * scattering walk (turtle_stepper_scatter_n) -- Philox(first + ray, stream; seed)
 * drawn in the kernel (the 48 bytes a ray's direction costs to write and read
 * back are a third of what a step moves); and what it adds up per ray. */
struct StepWalk {
        int on;
        ull seed, stream;
        long first;
        double * length; /* += the length of the step */
        int * steps;     /* += 1 */
};

/* What a batch of single steps defers to its second pass: the rays that
 * crossed a boundary (~2-5 % of them), and the tentative length of each. */
struct CrossList {
        int * ray;      /* NULL: the step kernel bisects in place */
        double * ds;
        ull * count;
        int * other;    /* traces: the medium and data index of the sample that crossed,
                         * packed (cross_pack); batches of single steps: NULL */
};

/* A trace's list of crossings in two parts, so that the lined pass's own waves can locate the
 * first while its long rays go on (trace_body, "the crossings under the tail"): L1, the front
 * of the arrays, counted by CrossList.count -- phase A's crossings and what a wave of the lined
 * pass lists until it learns that the queue is dry; L2, the same arrays from the far end, counted
 * by l2_count -- what it lists from then on.  n_dry counts the waves that have learnt it: once it
 * equals the waves of the grid nobody adds to L1 any more, and a wave that has run out of rays
 * locates L1 by tickets of 64 entries drawn from l1_next.  k_cross takes the rest.  NULL: one
 * list, all of it left to k_cross. */
constexpr int kQ = TAMD_TRACE_COUNTER_STRIDE; /* words between two counters of a trace (internal.h) */
constexpr int kQTail = 4 * kQ;
struct CrossTail {
        ull * words; /* the three counters, kQ words apart */
        /* (the lined pass finds them kQTail words behind its queue's counter and is told by a flag
         * to look: TRACE_CROSS_TAIL -- its kernel has no register to spare for a pointer) */
        __device__ __forceinline__ ull * n_dry() const { return words; }
        __device__ __forceinline__ ull * l1_next() const { return words + kQ; }
        __device__ __forceinline__ ull * l2_count() const { return words + 2 * kQ; }
};

/* (medium, data index) of a sample, each -1 .. 65 534, in one int */
__device__ __forceinline__ int cross_pack(int m, int k) { return (m + 1) | ((k + 1) << 16); }
__device__ __forceinline__ void cross_unpack(int packed, int & m, int & k)
{
        m = (packed & 0xffff) - 1, k = (int)((unsigned)packed >> 16) - 1;
}

/* One turtle_stepper_step per thread [ref stepper.c:780-875].  With a direction
 * a step is one sample at the tentative position -- and, for the few rays whose
 * medium changed there, a ~27-sample bisection.  Run inside this kernel that
 * loop would idle the other lanes of every wave that holds such a ray (nearly
 * all of them do), so the kernel only LISTS those rays (position moved to the
 * tentative point, medium unchanged) and k_bisect finishes them, packed: a batch
 * of n single steps costs n + 27 x (rays that crossed) samples, all at full
 * lane occupancy, and exposes n-way parallelism to the gathers (a scattering
 * Monte-Carlo over a 2.6 GB mosaic is bound by their latency).
 * stats (or NULL): rays, steps, samples, steps that did not cross. */
template <int MODE, bool FAST>
__device__ __forceinline__ void step_items(const tamd_view & v, long n,
    double * __restrict__ pos, const double * __restrict__ dir,
    double * __restrict__ lat, double * __restrict__ lon, double * __restrict__ alt,
    double * __restrict__ elev, double * __restrict__ step, int * __restrict__ index,
    int flags, CrossList cross, Paging pg, ull * __restrict__ stats, StepWalk walk)
{
        OneCtx ctx;
        d_load_ctx<MODE, FAST>(v, ctx);
        const bool directed = (dir != nullptr) || walk.on;
        ull my_rays = 0, my_steps = 0, my_samples = 0, my_plain = 0;
        PAGED_ITEMS(pg, n, i0, r) /* whole waves go round: see the listings */
        {
                bool listed = false;
                double listed_ds = 0.;
                TileFault fault = { -1, 0, 0 }; /* tiles to page in: the ray is left as it is, and listed */
                int home = -1;
                /* TAMD_STEP_COMPACT (turtle_stepper_walk_n): all a step resumes from, besides the
                 * medium, is the tentative length the last sample gave it [ref stepper.c:799-813:
                 * what the cached sample is read for] -- `alt` holds THAT, one double in and one
                 * out, and the altitude and the two elevations (24 B in, 24 B out) stay in
                 * registers.  The same function of the same values, evaluated when the sample is
                 * taken instead of when the next step begins: the same bits. */
                const bool compact = (flags & TAMD_STEP_COMPACT) != 0;
                double ds_given = -1.;
                /* a walk: a ray that has left the data takes no further step (nor does a
                 * ray a paged traverse has finished) */
                if ((walk.on || (flags & TAMD_STEP_LIVE)) && (r >= 0) && (index[2 * r] < 0)) r = -1;
                if (r >= 0) {
                double px = pos[3 * r], py = pos[3 * r + 1], pz = pos[3 * r + 2];
                Sample s;
                if ((flags & TURTLE_AMD_STEP_RESUME) && directed && (index[2 * r] >= 0)) {
                        /* the caller hands back the sample of this position
                         * [ref stepper.c:708-710, :745-748]; its latitude and
                         * longitude are not read: whatever becomes of the step,
                         * the ones published are the new sample's */
                        s.lat = 0., s.lon = 0.;
                        if (compact) {
                                ds_given = alt[r];
                                s.alt = 0., s.e0 = -DBL_MAX, s.e1 = DBL_MAX;
                        } else {
                                s.alt = alt[r];
                                s.e0 = elev[2 * r], s.e1 = elev[2 * r + 1];
                        }
                        s.m = index[2 * r], s.k = index[2 * r + 1];
                } else {
                        d_sample<MODE, FAST>(v, ctx, px, py, pz, s);
                        my_samples++;
                        fault = s.fault;
                        home = s.slot;
                        /* a ray handed back as having left the data has left it, as the
                         * reference's cache would answer [ref stepper.c:708-710, :791-796]: it
                         * stands within the 1e-8 m of the bisection that located its exit, where
                         * an ulp of the fast transform can tell this sample otherwise -- and the
                         * ray would walk back in */
                        if ((flags & TURTLE_AMD_STEP_RESUME) && directed && (fault.centre < 0)) s.m = -1, s.k = -1;
                }

                double ds = 0.;
                if ((s.m >= 0) && (fault.centre < 0)) {
                        ds = (ds_given >= 0.) ? ds_given : d_step_length(v, s.alt, s.e0, s.e1, s.m);
                        if (directed) {
                                double dx, dy, dz;
                                if (walk.on)
                                        d_isotropic((ull)(walk.first + r), walk.stream, walk.seed, dx, dy, dz);
                                else
                                        dx = dir[3 * r], dy = dir[3 * r + 1], dz = dir[3 * r + 2];
                                px += dx * ds, py += dy * ds, pz += dz * ds;
                                const int medium0 = s.m, data0 = s.k;
                                Sample s1;
                                d_sample<MODE, FAST>(v, ctx, px, py, pz, s1);
                                my_samples++, my_steps++;
                                fault = s1.fault;
                                if (fault.centre >= 0) {
                                        /* nothing */
                                } else if (s1.m == medium0) {
                                        s = s1;
                                        my_plain++;
                                } else if (cross.ray != nullptr) {
                                        /* [ref stepper.c:832-838] the second pass
                                         * starts from here: position moved, the
                                         * medium and data index still the old ones */
                                        listed = true, listed_ds = ds;
                                        s.m = medium0, s.k = data0;
                                } else { /* [ref stepper.c:832-864] */
                                        double ds0 = -ds, ds1 = 0.;
                                        s = s1;
                                        while (ds1 - ds0 > 1E-08) {
                                                const double ds2 = 0.5 * (ds0 + ds1);
                                                Sample s2;
                                                d_sample<MODE, FAST>(v, ctx, px + dx * ds2,
                                                    py + dy * ds2, pz + dz * ds2, s2);
                                                my_samples++;
                                                if (s2.fault.centre >= 0) {
                                                        fault = s2.fault;
                                                        break;
                                                }
                                                if (s2.m == medium0)
                                                        ds0 = ds2;
                                                else {
                                                        ds1 = ds2;
                                                        s = s2;
                                                }
                                        }
                                        ds += ds1;
                                        px += dx * ds1, py += dy * ds1, pz += dz * ds1;
                                }
                                if (fault.centre < 0) pos[3 * r] = px, pos[3 * r + 1] = py, pos[3 * r + 2] = pz;
                                /* (a listed ray: k_bisect's, with the length it ends up with) */
                                if (walk.on && !listed && (fault.centre < 0)) walk.length[r] += ds, walk.steps[r] += 1;
                        }
                }
                if (fault.centre >= 0) listed = false;
                if (!listed && (fault.centre < 0)) my_rays++;
                /* sample_publish [ref stepper.c:758-778] (a listed ray: k_bisect's) */
                if (!listed && (fault.centre < 0)) {
                        if (lat) lat[r] = s.lat;
                        if (lon) lon[r] = s.lon;
                        if (alt) alt[r] = !compact ? s.alt : ((s.m >= 0) ? d_step_length(v, s.alt, s.e0, s.e1, s.m) : 0.);
                        if (elev && !compact) {
                                elev[2 * r] = (s.m >= 0) ? s.e0 : 0.;
                                elev[2 * r + 1] = (s.m >= 0) ? s.e1 : 0.;
                        }
                        if (step) step[r] = ds;
                }
                if (fault.centre < 0) index[2 * r] = s.m, index[2 * r + 1] = s.k;
                }
                if (pg.faulted != nullptr) page_fault(pg, fault, r, home);
                /* list the rays that crossed: one atomic per wave */
                if (cross.ray != nullptr) {
                        const ull mask = __ballot(listed);
                        if (mask != 0) {
                                const int leader = __builtin_ctzll(mask);
                                ull base = 0;
                                if ((int)(threadIdx.x & 63) == leader)
                                        base = atomicAdd(cross.count, (ull)__popcll(mask));
                                base = __shfl(base, leader, 64);
                                if (listed) {
                                        const int rank = lane_rank(mask);
                                        cross.ray[base + rank] = (int)r;
                                        cross.ds[base + rank] = listed_ds;
                                }
                        }
                }
        }
        if (stats != nullptr) block_tally(stats, my_rays, my_steps, my_samples, my_plain);
}

/* The kernel proper, once per arithmetic.  A batch of single steps is bound by
 * the latency of its dependent loads (ray state -> nodes), so waves in flight
 * count: the fast-math body of the specialised modes fits 128 registers (4 waves
 * per SIMD instead of 3: -7 %, measured on C5) when told to; the strict one would
 * spill 230 bytes a lane for it (+23 %), and so would the fast body of the
 * generic mode: they are left alone. */
#define STEP_ARGS                                                                              \
        tamd_view v, long n, double * __restrict__ pos, const double * __restrict__ dir,       \
            double * __restrict__ lat, double * __restrict__ lon, double * __restrict__ alt,   \
            double * __restrict__ elev, double * __restrict__ step, int * __restrict__ index,  \
            int flags, CrossList cross, Paging pg, ull * __restrict__ stats, StepWalk walk
#define STEP_PASS v, n, pos, dir, lat, lon, alt, elev, step, index, flags, cross, pg, stats, walk
template <int MODE, bool FAST>
__global__ void __launch_bounds__(256) k_step(STEP_ARGS)
{
        step_items<MODE, FAST>(STEP_PASS);
}
template <int MODE>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) k_step_fast(STEP_ARGS)
{
        step_items<MODE, true>(STEP_PASS);
}
#undef STEP_ARGS
#undef STEP_PASS

/* The second pass of a batch of single steps: the bisection of the listed rays
 * [ref stepper.c:836-864], every lane busy.  The ray's position is the tentative
 * point q, its index the medium it left; the first sample (at q again: the
 * same arithmetic on the same point as in the first pass) is the first
 * candidate for the medium it entered. */
template <int MODE, bool FAST>
__global__ void __launch_bounds__(256) k_bisect(tamd_view v, double * __restrict__ pos,
    const double * __restrict__ dir, double * __restrict__ lat, double * __restrict__ lon,
    double * __restrict__ alt, double * __restrict__ elev, double * __restrict__ step,
    int * __restrict__ index, int flags, CrossList cross, Paging pg, ull * __restrict__ stats, StepWalk walk)
{
        OneCtx ctx;
        d_load_ctx<MODE, FAST>(v, ctx);
        const bool compact = (flags & TAMD_STEP_COMPACT) != 0; /* see step_items */
        const long n = (long)*cross.count;
        ull my_rays = 0, my_samples = 0;
        for (long i0 = blockIdx.x * (long)blockDim.x; i0 < n; i0 += (long)gridDim.x * blockDim.x) {
                const long i = i0 + threadIdx.x; /* whole waves go round (page_fault) */
                TileFault fault = { -1, 0, 0 };
                int home = -1;
                long r = -1;
                if (i < n) {
                r = cross.ray[i];
                double ds = cross.ds[i];
                double px = pos[3 * r], py = pos[3 * r + 1], pz = pos[3 * r + 2];
                double dx, dy, dz;
                if (walk.on)
                        d_isotropic((ull)(walk.first + r), walk.stream, walk.seed, dx, dy, dz);
                else
                        dx = dir[3 * r], dy = dir[3 * r + 1], dz = dir[3 * r + 2];
                const int medium0 = index[2 * r];
                CellCache cell = { ~0u, 0u, 0u, -1, nullptr };
                CellCache * cache = (FAST && (MODE != TAMD_MODE_GENERIC)) ? &cell : nullptr;
                Sample s;
                /* fast math: the bracket is a segment of the ray behind q, so the
                 * ~27 samples come from the line laid at q (see RayLine) */
                RayLine line;
                double at = 0.; /* q's parameter on the line */
                if (FAST) {
                        f_to_geodetic(px, py, pz, s.lat, s.lon, s.alt, &line, dx, dy, dz);
                        d_classify<MODE, true>(v, ctx, s, cache);
                } else
                        d_sample<MODE, false>(v, ctx, px, py, pz, s, cache);
                fault = s.fault;
                home = s.slot;
                double ds0 = -ds, ds1 = 0.;
                int halvings = 0;
                while ((fault.centre < 0) && (ds1 - ds0 > 1E-08) && (halvings++ <= 1200)) {
                        const double ds2 = 0.5 * (ds0 + ds1);
                        Sample s2;
                        if (FAST) {
                                if (f_sample_on_line<MODE>(v, ctx, px + dx * ds2, py + dy * ds2,
                                        pz + dz * ds2, dx, dy, dz, line, at + ds2, s2, cache))
                                        at = -ds2; /* a new line, laid at this sample */
                        } else
                                d_sample<MODE, false>(v, ctx, px + dx * ds2, py + dy * ds2,
                                    pz + dz * ds2, s2, cache);
                        my_samples++;
                        if (s2.fault.centre >= 0) {
                                fault = s2.fault;
                        } else if (s2.m == medium0)
                                ds0 = ds2;
                        else {
                                ds1 = ds2;
                                s = s2;
                        }
                }
                if (fault.centre >= 0) {
                        /* a tile to page in (the bracket straddles a third tile): the
                         * ray goes back before its step and is listed for the next
                         * round, which takes it from k_step again */
                        pos[3 * r] = px - dx * ds, pos[3 * r + 1] = py - dy * ds, pos[3 * r + 2] = pz - dz * ds;
                } else {
                ds += ds1;
                pos[3 * r] = px + dx * ds1, pos[3 * r + 1] = py + dy * ds1, pos[3 * r + 2] = pz + dz * ds1;
                if (lat) lat[r] = s.lat;
                if (lon) lon[r] = s.lon;
                if (alt) alt[r] = !compact ? s.alt : ((s.m >= 0) ? d_step_length(v, s.alt, s.e0, s.e1, s.m) : 0.);
                if (elev && !compact) {
                        elev[2 * r] = (s.m >= 0) ? s.e0 : 0.;
                        elev[2 * r + 1] = (s.m >= 0) ? s.e1 : 0.;
                }
                if (step) step[r] = ds;
                if (walk.on) walk.length[r] += ds, walk.steps[r] += 1;
                index[2 * r] = s.m, index[2 * r + 1] = s.k;
                my_rays++;
                }
                }
                if (pg.faulted != nullptr) page_fault(pg, fault, r, home);
        }
        if (stats != nullptr) block_tally(stats, my_rays, 0, my_samples, 0);
}

/* ---- the hot kernel ---------------------------------------------------- */

#ifndef PAGED_REFILL
#define PAGED_REFILL 24
#endif
constexpr int kPagedRefill = PAGED_REFILL; /* over paged tiles: the free lanes a wave waits for before it takes new rays */
constexpr int kTailChunk = 8; /* ... in the last phase of a fast trace: few, and long */
constexpr int kCreepLanes = 8; /* the creep loop engages at or below this many live lanes */
#ifndef CREEP_UNROLL
#define CREEP_UNROLL 32
#endif
constexpr int kCreepUnroll = CREEP_UNROLL; /* steps per trip of the one-map creep loop */
#ifndef CREEP_BACKOFF
#define CREEP_BACKOFF 8
#endif
constexpr int kCreepBackoff = CREEP_BACKOFF; /* general iterations a busy wave waits after a useless group */
#ifndef TRACE_RELAY_BATCH
#define TRACE_RELAY_BATCH 12
#endif
#ifndef TRACE_RELAY_PATIENCE
#define TRACE_RELAY_PATIENCE 3
#endif
constexpr int kRelayBatch = TRACE_RELAY_BATCH;       /* lanes of a busy wave that a closed form waits for ... */
constexpr int kRelayPatience = TRACE_RELAY_PATIENCE; /* ... at most this many general iterations */

/* Persistent waves; one ray per lane; ONE sample per lane per iteration.
 *
 * A ray alternates between optimistic steps (one sample each) and, once, a
 * ~20-30 sample bisection that locates the boundary it crossed.  Run as the
 * reference writes it (a while loop inside the step) the bisection would
 * idle the other 63 lanes of the wave.  Instead each lane carries a small
 * state machine (INIT -> STEP -> BISECT -> done) and every trip round the loop
 * evaluates exactly one sample for every live lane, whatever its state: the
 * expensive part (ECEF->geodetic + layer lookup) is always executed with a
 * full exec mask, and only the cheap bookkeeping diverges.
 *
 * Every state samples at  q = B + d * t :
 *   INIT    t = 0                      B = the ray's origin
 *   STEP    t = ds (tentative length)  B = last accepted position
 *   BISECT  t = (ds0 + ds1) / 2        B = the tentative position that crossed
 * and a STEP sample always moves B to q (accepted, or the bisection's origin),
 * so the per-lane state is B, d, three step scalars, the path length, the
 * step count and three small integers.  The arithmetic per ray is exactly
 * that of calling turtle_stepper_step in a loop [ref stepper.c:780-875].
 *
 * Finished lanes are refilled from a global ray queue: lanes that need a ray
 * are ranked with ballot/mbcnt, and the wave draws kChunk ray ids at a time
 * with one atomic (wave-aggregated), so the queue sees n / 64 atomics.
 *
 * Results do not depend on which lane runs a ray (rays are independent), so
 * the output is deterministic. */
/* TRACE_CARRY_MEDIUM: the caller knows which medium each ray is in (a trace
 * resumed after a boundary, or after parking) */
/* TRACE_CROSS_TAIL (the fast lined pass over resident data): the crossings go to two lists, and
 * the pass's own waves locate the first (CrossTail) */
enum { TRACE_CARRY_MEDIUM = 1, TRACE_CROSS_TAIL = 2 };

/* ---- a workgroup's pool of rays in LDS (round 4) --------------------------
 *
 * The lined pass alternates two kinds of work that want different lanes: LEAN
 * steps (a ray on its line over one grid: ~45 vector instructions a step, for
 * the lanes whose line and cell still serve) and GENERAL iterations (a closed
 * form that lays a new line, a new ray's first sample, a crossing to list:
 * ~1 000 instructions for the whole wave, whoever needs them).  With a ray
 * fixed to its lane, a group of lean steps ran for the lanes still on their
 * lines while the others waited, and a general iteration for the lanes that
 * needed one while the others took a single step or none: measured on C2
 * (round 3) 45 % of the lanes occupied and 5.6 x the wave-instructions the lean
 * steps alone would take.
 *
 * So the four waves of a block exchange rays through LDS.  Before each piece of
 * work a wave looks at what its lanes hold and at the pool and takes a ROLE:
 *   LEAN     its rays that need a general iteration go to the pool's `service`
 *            list, rays that are `ready` to step come out of the pool into the
 *            free lanes, and the wave runs a group of lean steps, all lanes going;
 *   SERVICE  its ready rays go to the pool's `ready` list, rays that wait for a
 *            general iteration come out of the pool (then new rays from the
 *            batch's queue), and the wave runs one general iteration for a full
 *            wave of rays that need it;
 *   AS IS    (the end of a pass: the batch's queue is dry and this wave and the
 *            pool hold less than a wave of rays) nothing goes to the pool, rays
 *            left there come out, and the wave does what it did before round 4.
 * A ray is a record of 27 words (position, direction, path length, step, its
 * line, its cell's nodes, its counters); records move under one lock a block
 * (held for the copy: a few hundred cycles, four waves).  Which lane or wave
 * takes a step of a ray never changed a bit of it (the same functions on the
 * same values), and does not now: `test_ray_pool_changes_no_bit`.
 *
 * A kernel must always end: a wave leaves when the batch's queue is dry, its
 * lanes are empty and so is the pool -- a ray in the pool was put there by a
 * wave that is still running and looks at the pool again before it leaves. */
#ifndef TRACE_POOL
#define TRACE_POOL 1
#endif
#ifndef TRACE_POOL_SLOTS
#define TRACE_POOL_SLOTS 192
#endif
#ifndef TRACE_POOL_LEAN_MIN
#define TRACE_POOL_LEAN_MIN 48
#endif
#ifndef TRACE_POOL_REFILL_FREE
#define TRACE_POOL_REFILL_FREE 64
#endif
/* -DTRACE_POOL_STATS: what the waves of a pooled pass do, summed over the launch (a diagnostic
 * build: scripts/exp_pool_stats.py reads the counters) */
#ifdef TRACE_POOL_STATS
__device__ unsigned long long g_pool_stats[32];
#define PSTAT(i, v) (pstat_[i] += (unsigned long long)(v))
#define PSTAT_CLOCK() __builtin_amdgcn_s_memtime()
#else
#define PSTAT(i, v) ((void)0)
#define PSTAT_CLOCK() 0ull
#endif
constexpr int kPoolSlots = TRACE_POOL_SLOTS;
constexpr int kPoolLeanMin = TRACE_POOL_LEAN_MIN;       /* ready rays for which a wave turns LEAN */
constexpr int kPoolRefillFree = TRACE_POOL_REFILL_FREE; /* free slots below which no new ray is drawn */
constexpr int kPoolDoubles = 23, kPoolInts = 8; /* a ray's record: 216 bytes */
enum { POOL_READY = 0, POOL_SERVICE = 1 };
enum { ROLE_AS_IS = 0, ROLE_LEAN = 1, ROLE_SERVICE = 2 };
struct RayPool {
        double d[kPoolDoubles][kPoolSlots]; /* field by field: a wave's lanes move 64 slots at once */
        int i[kPoolInts][kPoolSlots];
        unsigned short free_slot[kPoolSlots];    /* a stack */
        unsigned short list[2][kPoolSlots];      /* two rings: first in, first out */
        int lock;
        int n_free;
        int head[2], count[2];
};

/* Two-phase launches.  Steps per ray are heavy-tailed (C2: median 163, max
 * 11 327) and a ray's samples are sequential, so a launch lasts as long as its
 * longest ray.  Phase A therefore PARKS any ray that reaches `park_after` steps
 * (its state goes back to the ray arrays, its id to a list) and phase B resumes
 * the parked rays with each ray's line (MODEL; see RayLine), which makes a sample
 * a tenth of the closed form's instructions.
 * Which arithmetic a sample uses depends only on the ray's own step count and
 * positions, never on scheduling: results stay deterministic. */
/* Where a ray's FINAL results go when the passes work on the rays in an order of their own
 * (run_trace, k_ray_cells): the caller's arrays, at the ray's place there.  order_of == NULL: the
 * arrays the passes work on, same place. */
struct RayOut {
        const int * order_of;
        double * pos;
        int * index;
        double * length;
        int * n_steps;
};

struct PhaseIO {
        const int * ids;     /* phase B: the parked ray ids (else NULL: slot == ray) */
        const ull * n_dev;   /* phase B: their number, on the device */
        int * parked;        /* phase A: where to list parked rays (or NULL) */
        ull * n_parked;
        int park_after;      /* hand a ray over to the next phase at this step count (<= 0: never) */
        int accumulate;      /* 1 (phase B): length / n_steps continue from the arrays; 2 (a
                              * later round of a paged geometry): the tentative step too */
        Paging pg;           /* where to list the rays that need a tile paged in (or NULLs) */
        int drain_lanes;     /* phase A: hand over when the queue is dry and the wave is down
                              * to this many rays */
        int line_after;      /* phases B, C: the step count from which a ray steps on its
                              * line (see LINED) */
        int chunk;           /* rays a wave draws from the queue at once */
        int creep_lanes;     /* the creep loop engages at or below this many live lanes */
        int dense_go;        /* ... and above, while at least this many lanes step on (0: never) */
        CrossList cross;     /* CROSS: where to list the rays whose step crossed a boundary */
        /* the sorted hand-over (phase A -> B): the list is filled from both ends -- the
         * rays expected to go on for long from the front, the others from the back --
         * and read front first (see where phase A parks) */
        ull * n_parked_back;    /* A: the number of rays listed from the back (or NULL: one end) */
        const ull * n_dev_back; /* B: the same, to read the list */
        double * ds_mark;       /* A: a ray's step length at step mark_at */
        int mark_at;
        float long_if;          /* A: to the front, if expected to take more further steps than this */
        int pool;               /* B: the waves of a block exchange rays through LDS (RayPool) */
        RayOut out;             /* where a ray that ENDS in this pass leaves its results */
        /* A, rays in an order of the library's own: a new ray comes from the caller's arrays
         * (`out.order_of` says from which place) and leaves its direction in dir_copy for the passes
         * that follow */
        const double * pos_in, * dir_in;
        const int * index_in;
        double * dir_copy;
        unsigned char * sort_key; /* A: the key the hand-over list is ordered by before B reads it, per
                                 * place on the list (or NULL: B reads it as it was filled) */
};

/* CROSS: a ray whose step crossed a boundary is not bisected here (ST_BISECT
 * does not exist then: ~11-27 further samples of ONE lane, each a whole general
 * iteration of its wave -- measured on C2's lined pass: 65 % of the wave-cycles
 * for 15 % of the samples) but handed over as it stands at the tentative point --
 * position, the medium it left, path length and step count in the ray arrays;
 * its id, the tentative length and the medium the sample found in ph.cross -- and
 * k_cross locates every crossing of the batch afterwards, in full waves.  The
 * lane takes a new ray at once.
 *
 * The crossings under the tail (TAIL: the fast lined pass over resident data; CrossTail).  The
 * lined pass's queue is dry after a third of the pass and the rest of it is ever fewer waves with
 * the batch's longest rays, while the crossings -- packed, independent work -- waited for the last
 * of them.  A wave that has run out of rays now locates them before it leaves, if it can know that
 * the list it reads is complete: a wave lists into L1 until it learns that the queue is dry (from
 * its own refill, or from a look at the queue's counter every kTailPeek general iterations), then
 * releases what it has written, adds one to n_dry and lists into L2 from then on.  n_dry == the
 * waves of the grid therefore says that L1 and the rays on it are final and visible to whoever
 * reads n_dry and then acquires.  A wave that finds less leaves as it always did: nothing waits
 * for another wave, and a block that starts late makes the count complete later, never wrongly.
 * The locating waves run one priority level below the tracing ones, so that a long ray's wave on
 * the same SIMD issues first.  The same statements on the same values as k_cross (cross_locate),
 * the same additions to the totals: which kernel located a crossing changes no bit. */
constexpr int kTailPeek = 16;
template <int MODE, bool FAST, bool PAGED>
__device__ __forceinline__ void cross_locate(const tamd_view & v, const OneCtx & ctx, double * __restrict__ pos,
    const double * __restrict__ dir, int * __restrict__ index, double * __restrict__ length,
    int * __restrict__ n_steps, const CrossList & cross, const Paging & pg, const RayOut & out, long first,
    long stride, int lane, long hi, ull & my_rays, ull & my_samples);

template <int MODE, bool FAST, bool MODEL, bool PAGED, bool CROSS, bool POOL = false>
__device__ __forceinline__ void trace_body(const tamd_view & v, long n,
    double * __restrict__ pos, const double * __restrict__ dir, int max_steps,
    int * __restrict__ index, double * __restrict__ length, int * __restrict__ n_steps,
    int flags, const PhaseIO & ph, ull * __restrict__ stats, ull * __restrict__ queue)
{
        const long capacity = n; /* of the lists ph.ids, ph.parked */
        long n_front = n;
        if (ph.n_dev != nullptr) {
                n_front = (long)*ph.n_dev;
                n = n_front + ((ph.n_dev_back != nullptr) ? (long)*ph.n_dev_back : 0);
        }
        /* MODEL: besides its accumulated position B (bx, by, bz: the reference's
         * roundings, in every phase: see kLineTau0) a ray on its line carries
         * line.s, the path length from the point where the line was laid to B */
        RayLine line;
        line.valid = false, line.s = 0., line.tau = kLineTau0;
        /* Which arithmetic a sample uses depends on the ray's step count alone:
         * below ph.line_after the closed form at the accumulated position, as in
         * phase A; from there on the ray's line.  Phase A can then hand a ray over
         * at ANY step (it does, when the queue runs dry: see `drain`) without
         * changing a bit of the result.  LINED: this lane's ray is on its line. */
        bool lined_ = false;
#define LINED (MODEL && lined_)
        /* tiles to page in: stacks only, and only where some are not resident (the
         * bookkeeping costs a wave per SIMD in the one-stack kernel) */
        constexpr bool CAN_FAULT = PAGED && (MODE != TAMD_MODE_ONE_MAP);
        long pool_next = 0, pool_end = 0; /* wave-uniform */
        int creep_wait = 0;                /* wave-uniform: general iterations before a busy wave tries lean steps again */
        int relay_wait = 0;                /* general iterations that lanes of a busy wave have waited for a closed form */
        bool exhausted = false;            /* wave-uniform */
        /* (not the pooled instances: with the locating inlined they need 20 and 12 bytes more scratch a lane) */
        constexpr bool TAIL = MODEL && CROSS && FAST && !PAGED && !POOL &&
            ((MODE == TAMD_MODE_ONE_MAP) || (MODE == TAMD_MODE_ONE_STACK));
        int tail_peek = 0;                 /* wave-uniform, TAIL: general iterations since the last look at the
                                            * queue; -1 once the wave has added itself to n_dry */
        OneCtx ctx;
        d_load_ctx<MODE, FAST>(v, ctx);
        CellCache cell = { ~0u, 0u, 0u, -1, nullptr };
        const CrossTail tail = { queue + kQTail };
        if constexpr (TAIL)
                if (flags & TRACE_CROSS_TAIL) __builtin_amdgcn_s_setprio(1);

        long ray = -1;
        bool dead = false;
        int state = ST_INIT, count = 0, count0 = 0;
        double bx = 0, by = 0, bz = 0, dx = 0, dy = 0, dz = 0, len = 0;
        double ds = 0, ds0 = 0, ds1 = 0;
        double c0 = 0, c1 = 0; /* FAST: the clearances at the two ends of the bracket (f_bracket_point) */
        int m = -1, k = -1, bm = -1, bk = -1, halvings = 0;
        int home = -1; /* CAN_FAULT: the tile of the ray's last sample (see Sample.slot) */
        ull my_rays = 0, my_steps = 0, my_samples = 0, my_capped = 0;

        /* ---- the block's pool of rays (see RayPool) ---- */
        constexpr bool POOLED = POOL && (TRACE_POOL != 0) && FAST && MODEL && CROSS && !PAGED &&
            ((MODE == TAMD_MODE_ONE_MAP) || (MODE == TAMD_MODE_ONE_STACK));
        typedef __attribute__((address_space(3))) RayPool * lds_pool_t;
        lds_pool_t P = nullptr;
        bool pooled = false;   /* block-uniform */
        bool stopped_ = false; /* this lane's ray left a group of lean steps: it needs a general iteration */
        int role = ROLE_AS_IS; /* wave-uniform */
        bool pool_empty = true; /* wave-uniform: nothing was left in the pool at the last look */
        int pool_free = kPoolSlots;
        int idle_trips = 0;
#ifdef TRACE_POOL_STATS
        unsigned long long pstat_[24] = { 0 };
#endif
        if constexpr (POOLED) {
                __shared__ RayPool pool_;
                P = (lds_pool_t)&pool_;
                pooled = (ph.pool > 0) && ((MODE == TAMD_MODE_ONE_MAP) || ctx.stack.regular);
                if (pooled) {
                        for (int t = threadIdx.x; t < kPoolSlots; t += 256) P->free_slot[t] = (unsigned short)t;
                        if (threadIdx.x == 0) {
                                P->lock = 0, P->n_free = kPoolSlots;
                                P->head[0] = P->head[1] = 0, P->count[0] = P->count[1] = 0;
                        }
                        __syncthreads();
                }
        }
        /* One look at the pool: the wave takes its role and rays change places.  Whole wave. */
        auto pool_exchange = [&]() {
                if constexpr (POOLED) {
                        const bool has = (ray >= 0);
                        const bool ready = has & !stopped_ & (state == ST_STEP) & lined_ & line.valid &
                            (cell.id != ~0u) & (count + kCreepUnroll < max_steps);
                        const bool waits = has & !ready;
                        const int r_own = __popcll(__ballot(ready)), s_own = __popcll(__ballot(waits));
                        const int e_own = 64 - r_own - s_own;
                        const unsigned long long t_in = PSTAT_CLOCK();
                        (void)t_in;
                        /* the lock: one lane asks, the wave waits */
                        if ((threadIdx.x & 63) == 0) {
                                /* (bounded: a kernel must always end, whatever went wrong) */
                                int expected = 0;
                                for (int spin = 0; (spin < (1 << 22)) &&
                                     !__hip_atomic_compare_exchange_strong(&P->lock, &expected, 1, __ATOMIC_ACQUIRE,
                                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); spin++) {
                                        expected = 0;
                                        __builtin_amdgcn_s_sleep(2);
                                }
                        }
                        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
                        PSTAT(16, PSTAT_CLOCK() - t_in);
                        const int F = __builtin_amdgcn_readfirstlane(P->n_free);
                        const int R = __builtin_amdgcn_readfirstlane(P->count[POOL_READY]);
                        const int S = __builtin_amdgcn_readfirstlane(P->count[POOL_SERVICE]);
                        const int head_r = __builtin_amdgcn_readfirstlane(P->head[POOL_READY]);
                        const int head_s = __builtin_amdgcn_readfirstlane(P->head[POOL_SERVICE]);
                        /* what each role would have to work on */
                        const int lean_out = min(s_own, F), lean_in = min(R, e_own + lean_out);
                        const int lean_n = r_own + lean_in;
                        const int serv_out = min(r_own, F), serv_in = min(S, e_own + serv_out);
                        const int serv_n = s_own + serv_in;
                        if (exhausted && (r_own + s_own + R + S < 64))
                                role = ROLE_AS_IS;
                        else if ((lean_n >= kPoolLeanMin) || (exhausted && (lean_n > serv_n)))
                                role = ROLE_LEAN;
                        else
                                role = ROLE_SERVICE;
                        /* who goes */
                        const bool goes = (role == ROLE_LEAN) ? waits : ((role == ROLE_SERVICE) ? ready : false);
                        const int n_out = (role == ROLE_LEAN) ? lean_out : ((role == ROLE_SERVICE) ? serv_out : 0);
                        const int out_kind = (role == ROLE_LEAN) ? POOL_SERVICE : POOL_READY;
                        const int out_rank = lane_rank(__ballot(goes));
                        const bool push = goes & (out_rank < n_out);
                        int out_slot = 0;
                        if (push) out_slot = P->free_slot[F - 1 - out_rank];
                        /* who comes: into the lanes that are or become free -- ready rays for a
                         * lean wave, waiting ones for a serving wave, either kind at the end */
                        const bool free_lane = !has | push;
                        const int in_rank = lane_rank(__ballot(free_lane));
                        int n_in_r = 0, n_in_s = 0;
                        if (role == ROLE_LEAN) n_in_r = lean_in;
                        if (role == ROLE_SERVICE) n_in_s = serv_in;
                        if (role == ROLE_AS_IS) n_in_r = min(R, e_own), n_in_s = min(S, e_own - n_in_r);
                        const bool pull_r = free_lane & (in_rank < n_in_r);
                        const bool pull_s = free_lane & !pull_r & (in_rank < n_in_r + n_in_s);
                        int in_slot = 0;
                        if (pull_r) in_slot = P->list[POOL_READY][(head_r + in_rank) % kPoolSlots];
                        if (pull_s) in_slot = P->list[POOL_SERVICE][(head_s + in_rank - n_in_r) % kPoolSlots];
                        if (push) {
                                const int q = out_slot;
                                P->d[0][q] = bx, P->d[1][q] = by, P->d[2][q] = bz;
                                P->d[3][q] = dx, P->d[4][q] = dy, P->d[5][q] = dz;
                                P->d[6][q] = len, P->d[7][q] = ds, P->d[8][q] = line.s;
                                P->d[9][q] = line.lat[0], P->d[10][q] = line.lat[1], P->d[11][q] = line.lat[2], P->d[12][q] = line.lat[3];
                                P->d[13][q] = line.lon[0], P->d[14][q] = line.lon[1], P->d[15][q] = line.lon[2], P->d[16][q] = line.lon[3];
                                P->d[17][q] = line.alt[0], P->d[18][q] = line.alt[1], P->d[19][q] = line.alt[2], P->d[20][q] = line.alt[3];
                                P->d[21][q] = line.k4, P->d[22][q] = line.tau;
                                P->i[0][q] = (int)ray, P->i[1][q] = count, P->i[2][q] = m, P->i[3][q] = k;
                                P->i[4][q] = state | (lined_ ? 4 : 0) | (line.valid ? 8 : 0) | (stopped_ ? 16 : 0);
                                P->i[5][q] = (int)cell.id, P->i[6][q] = (int)cell.lo, P->i[7][q] = (int)cell.hi;
                                /* the steps a ray took are counted by the wave that took them */
                                my_steps += (ull)(count - count0);
                                ray = -1;
                        }
                        if (pull_r | pull_s) {
                                const int q = in_slot;
                                bx = P->d[0][q], by = P->d[1][q], bz = P->d[2][q];
                                dx = P->d[3][q], dy = P->d[4][q], dz = P->d[5][q];
                                len = P->d[6][q], ds = P->d[7][q], line.s = P->d[8][q];
                                line.lat[0] = P->d[9][q], line.lat[1] = P->d[10][q], line.lat[2] = P->d[11][q], line.lat[3] = P->d[12][q];
                                line.lon[0] = P->d[13][q], line.lon[1] = P->d[14][q], line.lon[2] = P->d[15][q], line.lon[3] = P->d[16][q];
                                line.alt[0] = P->d[17][q], line.alt[1] = P->d[18][q], line.alt[2] = P->d[19][q], line.alt[3] = P->d[20][q];
                                line.k4 = P->d[21][q], line.tau = P->d[22][q];
                                ray = P->i[0][q], count = P->i[1][q], m = P->i[2][q], k = P->i[3][q];
                                count0 = count;
                                const int bits = P->i[4][q];
                                state = bits & 3, lined_ = (bits & 4) != 0, line.valid = (bits & 8) != 0, stopped_ = (bits & 16) != 0;
                                cell.id = (unsigned)P->i[5][q], cell.lo = (unsigned)P->i[6][q], cell.hi = (unsigned)P->i[7][q];
                        }
                        /* the lists: slots that were read are free again, the ones written are listed */
                        const int n_in = n_in_r + n_in_s;
                        if (pull_r | pull_s) P->free_slot[F - n_out + in_rank] = (unsigned short)in_slot;
                        /* (a ring's tail is where it was: what came out of it came from its head) */
                        const int tail = ((out_kind == POOL_READY) ? head_r + R : head_s + S) + out_rank;
                        if (push) P->list[out_kind][tail % kPoolSlots] = (unsigned short)out_slot;
                        if ((threadIdx.x & 63) == 0) {
                                P->n_free = F - n_out + n_in;
                                P->head[POOL_READY] = (head_r + n_in_r) % kPoolSlots;
                                P->head[POOL_SERVICE] = (head_s + n_in_s) % kPoolSlots;
                                P->count[POOL_READY] = R - n_in_r + ((out_kind == POOL_READY) ? n_out : 0);
                                P->count[POOL_SERVICE] = S - n_in_s + ((out_kind == POOL_SERVICE) ? n_out : 0);
                        }
                        pool_empty = (R - n_in_r + S - n_in_s + n_out) == 0;
                        pool_free = F - n_out + n_in;
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                        if ((threadIdx.x & 63) == 0)
                                __hip_atomic_store(&P->lock, 0, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
                        PSTAT(0, 1), PSTAT((role == ROLE_AS_IS) ? 3 : role, 1), PSTAT(4, PSTAT_CLOCK() - t_in), PSTAT(13, n_out), PSTAT(14, n_in);
                        PSTAT(17, r_own), PSTAT(18, s_own), PSTAT(19, R), PSTAT(20, S);
                }
        };

        for (;;) {
                if (POOLED && pooled) pool_exchange();
                /* ---- refill idle lanes from the queue ---- */
                for (;;) {
                        /* (pooled: a lean wave takes no new ray -- it would wait for a general
                         * iteration -- and a block whose pool is nearly full has rays enough) */
                        if (POOLED && pooled && ((role == ROLE_LEAN) || (pool_free < kPoolRefillFree))) break;
                        const bool need = (ray < 0) && !dead;
                        const ull mask = __ballot(need);
                        if (mask == 0) break;
                        /* Over paged tiles a new ray may need one that is not resident: its first
                         * sample then takes the exact lookup, with its dependent loads, and the
                         * ray leaves for the list -- a trip that costs the whole wave six times a
                         * plain one.  With half the tiles away half of the new rays do, and if a
                         * wave took new rays whenever a lane was free EVERY trip of it would be
                         * such a one (C3 with 8 of 16 tiles: the closed-form pass 28 ms for
                         * 6.4): the free lanes wait until there are kPagedRefill of them. */
                        if (CAN_FAULT && (ph.pg.faulted != nullptr) && !exhausted &&
                            (__popcll(mask) < kPagedRefill) && (__ballot(ray >= 0) != 0))
                                break;
                        if (pool_next >= pool_end) {
                                if (exhausted) {
                                        if (need) dead = true;
                                        break;
                                }
                                ull base = 0;
                                if ((threadIdx.x & 63) == 0)
                                        base = atomicAdd(queue, (ull)ph.chunk);
                                base = __shfl(base, 0, 64);
                                pool_next = (long)base;
                                pool_end = min((long)base + ph.chunk, n);
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
                                if (ph.ids != nullptr)
                                        ray = ph.ids[(ray < n_front) ? ray : capacity - 1 - (ray - n_front)];
                                if (MODEL) line.valid = false, line.s = 0., line.tau = kLineTau0;
                                stopped_ = false;
                                if (!MODEL && (ph.dir_copy != nullptr)) {
                                        /* (the rays in the library's order: see PhaseIO) */
                                        const long src = ph.out.order_of[ray];
                                        bx = ph.pos_in[3 * src], by = ph.pos_in[3 * src + 1], bz = ph.pos_in[3 * src + 2];
                                        dx = ph.dir_in[3 * src], dy = ph.dir_in[3 * src + 1], dz = ph.dir_in[3 * src + 2];
                                        ph.dir_copy[3 * ray] = dx, ph.dir_copy[3 * ray + 1] = dy, ph.dir_copy[3 * ray + 2] = dz;
                                        if (flags & TRACE_CARRY_MEDIUM)
                                                index[2 * ray] = ph.index_in[2 * src], index[2 * ray + 1] = ph.index_in[2 * src + 1];
                                } else {
                                        bx = pos[3 * ray], by = pos[3 * ray + 1], bz = pos[3 * ray + 2];
                                        dx = dir[3 * ray], dy = dir[3 * ray + 1], dz = dir[3 * ray + 2];
                                }
                                len = 0., count = 0, state = ST_INIT;
                                if (ph.accumulate) len = length[ray], count = n_steps[ray];
                                count0 = count;
                                lined_ = MODEL && (count >= ph.line_after);
                                if (CAN_FAULT && (ph.accumulate == 2)) {
                                        /* a ray that waited for a tile: it carries on
                                         * with the step it was about to take (a fresh
                                         * sample of its position could need the tile it
                                         * came from, which may be gone) */
                                        const double w = ph.pg.tentative[ray];
                                        if (w >= 0.) {
                                                state = ST_STEP, ds = w;
                                                m = index[2 * ray], k = index[2 * ray + 1];
                                        }
                                }
                        }
                        pool_next += min((long)__popcll(mask), avail);
                }
                /* ---- TAIL: the moment the wave learns that the queue is dry (once) ---- */
                if constexpr (TAIL) {
                        if ((flags & TRACE_CROSS_TAIL) && (tail_peek >= 0)) {
                                /* (wave-uniform, and the compiler is told so: the counter stays scalar) */
                                bool dry = __builtin_amdgcn_readfirstlane((int)exhausted) != 0;
                                if (!dry && (++tail_peek >= kTailPeek)) {
                                        /* (a wave that holds its rays never asks the queue) */
                                        tail_peek = 0;
                                        const ull drawn = __hip_atomic_load(queue, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                        dry = __builtin_amdgcn_readfirstlane((int)(drawn >= (ull)n)) != 0;
                                }
                                if (dry) {
                                        /* what the wave listed into L1, and those rays' state: released
                                         * BEFORE the add that says so (the wait: the fence's own may be
                                         * dropped where the compiler thinks nothing is in flight) */
                                        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                                        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                                        if ((threadIdx.x & 63) == 0)
                                                __hip_atomic_fetch_add(tail.n_dry(), 1ull, __ATOMIC_RELAXED,
                                                    __HIP_MEMORY_SCOPE_AGENT);
                                        tail_peek = -1;
                                }
                        }
                }
                if (__ballot(ray >= 0) == 0) {
                        if (!(POOLED && pooled)) break;
                        /* pooled: the wave leaves when the queue is dry and the pool was empty at
                         * its last look; else it looks again (a kernel must always end: a wave that
                         * finds nothing a million times over leaves too -- its rays, if any were
                         * left, are then missing from the totals, which the callers check) */
                        if ((exhausted && pool_empty) || (++idle_trips > 1000000)) break;
                        if (role == ROLE_LEAN) role = ROLE_SERVICE; /* (cannot be: a lean wave has rays) */
                        __builtin_amdgcn_s_sleep(8);
                        continue;
                }
                idle_trips = 0;
                /* ---- creep loop (phase B, sparse waves) ---------------------------
                 * What is left at the end of a launch is a handful of rays
                 * skimming the ground with ~0.5 m steps for thousands of steps.
                 * While every live lane of the wave is such a ray -- stepping on
                 * its line -- a step needs no state machine: this loop does just
                 * that (laying a new line or fetching a new cell when needed),
                 * and hands any lane that needs more (a boundary, the step cap,
                 * another state) back to the general iteration below WITHOUT
                 * having committed that step.  It calls the same functions on
                 * the same values as the general path, so results do not depend
                 * on whether it engaged. */
                if (MODEL && (MODE != TAMD_MODE_ONE_MAP) &&
                    !((MODE == TAMD_MODE_ONE_STACK) && ctx.stack.regular) && /* -> the lean loop below */
                    (__popcll(__ballot(ray >= 0)) <= ph.creep_lanes)) {
                        for (int it = 0; it < 4096; it++) {
                                bool fail = false;
                                double qx = 0, qy = 0, qz = 0;
                                Sample s;
                                if (ray >= 0) {
                                        fail = (state != ST_STEP) || (count + 1 >= max_steps) || !lined_;
                                        if (!fail) {
                                                const double sl = line.s + ds;
                                                qx = d_along<FAST>(bx, dx, ds), qy = d_along<FAST>(by, dy, ds), qz = d_along<FAST>(bz, dz, ds);
                                                /* a new line starts at q: B is at -ds on it */
                                                if (f_sample_on_line<MODE>(v, ctx, qx, qy, qz, dx, dy,
                                                        dz, line, sl, s,
                                                        (MODE != TAMD_MODE_GENERIC) ? &cell : nullptr))
                                                        line.s = -ds;
                                                fail = (s.m != m) || (s.fault.centre >= 0);
                                        }
                                }
                                /* a lane that must leave has sampled q but not moved:
                                 * the general iteration samples the same q again, and
                                 * gets the same bits (line and cell now serve q) */
                                if (__ballot(fail) != 0) break;
                                if (ray >= 0) {
                                        bx = qx, by = qy, bz = qz;
                                        line.s += ds;
                                        line.tau += kLineDrift;
                                        len += ds;
                                        count++;
                                        k = s.k;
                                        my_samples++;
                                        ds = d_step_length(v, s.alt, s.e0, s.e1, s.m);
                                }
                        }
                }

                /* ---- lean steps (one map, a regular stack) ------------------------
                 * The lined pass's work horse: a step of a ray on its line over one
                 * grid is the line (nine fused operations), the cell (its four nodes
                 * decoded to the patch's coefficients once per cell; fetched here when
                 * the ray walks into the next one) and the reference's tests -- ~75
                 * vector instructions where a closed-form sample takes a thousand.
                 * A lane that needs anything else (a new line, a crossing and its
                 * bisection, the rim of the grid, the step cap) stops WITHOUT having
                 * committed that step, and a general iteration below takes it: the
                 * same functions on the same values, so results do not depend on
                 * where a step was taken.  "Does any lane have to leave?" is a
                 * wave-wide question (compare, ballot, branch: the vector and
                 * scalar units wait for each other): it is asked once per
                 * kCreepUnroll steps, and a lane that cannot take one of them takes
                 * none of the following.  In a wave of a handful of rays (the end of
                 * a launch: C2's longest ray takes 11 326 steps) the group ends when
                 * any lane stopped; in a busy one the lanes that stopped wait while
                 * dense_go others step on.  The SIMD's issue slots bound this loop
                 * (three waves of it keep the vector unit ~90 % busy): what counts is
                 * the instructions of a step and the share of lanes that take it. */
                const int live = __popcll(__ballot(ray >= 0));
                const bool sparse = (live <= ph.creep_lanes);
                if (creep_wait > 0) creep_wait--;
                if (MODEL &&
                    ((MODE == TAMD_MODE_ONE_MAP) || ((MODE == TAMD_MODE_ONE_STACK) && ctx.stack.regular)) &&
                    (sparse || ((ph.dense_go > 0) && (creep_wait == 0)) || (POOLED && (role == ROLE_LEAN))) &&
                    !(POOLED && (role == ROLE_SERVICE))) {
                        /* one map: the grid.  A regular stack: the tile the cached cell is
                         * in -- the shared tile shape at that tile's origin, computed as
                         * f_stack_elevation computes it; a point `interior` to it (same
                         * guard as there) gets that tile from the directory too */
                        constexpr bool STACK = (MODE == TAMD_MODE_ONE_STACK);
                        const tamd_grid & g = STACK ? ctx.stack.proto : ctx.grid;
                        /* The cached cell, decoded once per entry (and after a trip that
                         * changed it): its origin, its node coordinates as doubles and its
                         * four elevations -- a step then needs no conversion between
                         * integers and doubles (a quarter of the rate of the other
                         * instructions, and on the chain).  Same values as f_grid_locate /
                         * f_grid_blend produce: for an interior point (double)(int)hx ==
                         * trunc(hx), and the clamp of the cell index does nothing.
                         * "Still in the cached cell" is asked of the fractions fx = hx - cx,
                         * fy = hy - cy with a margin of `guard` -- g < f < 1 - g, as a test of f's
                         * upper word against those of g and 1 - g -- so that a point that
                         * passes is `interior` to the grid (or the tile: the guards of
                         * f_grid_locate and f_stack_elevation) whichever cell it is in; the few
                         * within the margin of a cell's edge take the way of a cell change,
                         * which makes that test on the point itself. */
                        constexpr double guard = STACK ? kSeamGuard : 1e-6;
                        /* the upper word of guard, plus one; that of 1 - guard */
                        constexpr unsigned lo_word = STACK ? 0x3e112e0cu : 0x3eb0c6f8u;
                        constexpr unsigned span_words = (STACK ? 0x3fefffffu : 0x3feffffdu) - lo_word;
                        const double mx = (double)(g.nx - 1) - guard, my = (double)(g.ny - 1) - guard;
                        double x0, y0, cx, cy, z00, z10, z01, z11;
                        bool cached;
                        auto decode_nodes = [&]() {
                                if (g.is_signed) {
                                        z00 = (double)(int16_t)(cell.lo & 0xffffu), z10 = (double)((int)cell.lo >> 16);
                                        z01 = (double)(int16_t)(cell.hi & 0xffffu), z11 = (double)((int)cell.hi >> 16);
                                } else {
                                        z00 = (double)(cell.lo & 0xffffu), z10 = (double)(cell.lo >> 16);
                                        z01 = (double)(cell.hi & 0xffffu), z11 = (double)(cell.hi >> 16);
                                }
                                z00 = __builtin_fma(z00, g.dz, g.z0), z10 = __builtin_fma(z10, g.dz, g.z0);
                                z01 = __builtin_fma(z01, g.dz, g.z0), z11 = __builtin_fma(z11, g.dz, g.z0);
                                /* f_patch's coefficients, as f_grid_blend forms them */
                                z11 = (z11 - z10) - (z01 - z00), z10 = z10 - z00, z01 = z01 - z00;
                        };
                        auto decode_cell = [&]() {
                                cached = (cell.id != ~0u);
                                const unsigned slot = STACK ? (cell.id >> 24) : 0u;
                                const unsigned cell_index = STACK ? (cell.id & 0xffffffu) : cell.id;
                                const unsigned tile_y = STACK ? slot / (unsigned)ctx.stack.nlon : 0u;
                                const unsigned tile_x = STACK ? slot - tile_y * (unsigned)ctx.stack.nlon : 0u;
                                x0 = STACK ? ctx.stack.lon0 + (int)tile_x * ctx.stack.dlon : g.x0;
                                y0 = STACK ? ctx.stack.lat0 + (int)tile_y * ctx.stack.dlat : g.y0;
                                const unsigned cell_iy = cached ? cell_index / (unsigned)g.nx : 0u;
                                const unsigned cell_ix = cached ? cell_index - cell_iy * (unsigned)g.nx : 0u;
                                cy = cached ? (double)cell_iy : -1.;
                                cx = cached ? (double)cell_ix : -1.;
                                decode_nodes();
                        };
                        decode_cell();
                        /* The test of a lean step is SUFFICIENT for the step the general
                         * iteration would accept, not equivalent to it -- a lane that fails
                         * it has committed nothing and the general iteration decides: with
                         * t = altitude - elevation and sgn = -1 in the rock, +1 above it,
                         *   sgn t > tau                  => the line serves as to drift and
                         *                                   truncation near the boundary (|t| > tau)
                         *                                   AND the medium is the ray's;
                         *   k4 min(max(|t|, 1), 400) > s^4   => the line serves as to its reach,
                         *                                   which is then below kLineRange too
                         *                                   (kLeanClearance: (5.56e11 x 400)^(1/4) =
                         *                                   3862 m at the equator, where k4 is largest);
                         * and a step within kCreepUnroll of the cap is left to the general
                         * iteration.  Two compares a step decide it where the reference's
                         * tests, one by one, took a dozen and as many scalar instructions
                         * between them: that chain is what a step of a lone wave waits for. */
                        const double sgn = (m == 0) ? -1. : 1.; /* a lane's medium does not change in here */
                        const int count_in = count;
                        const unsigned long long t_lean = PSTAT_CLOCK();
                        (void)t_lean;
                        for (int it = 0; it < 4096; it++) {
                                /* no short-circuits below: every lane computes
                                 * everything (garbage is harmless, nothing is
                                 * committed on failure) and the tests are AND-ed */
                                bool going = (ray >= 0) & (state == ST_STEP) & lined_ & line.valid & cached &
                                    (count + kCreepUnroll < max_steps);
                                PSTAT(5, 1), PSTAT(7, __popcll(__ballot(going)));
#pragma unroll
                                for (int u = 0; u < kCreepUnroll; u++) {
                                        const double sl = line.s + ds;
                                        double lat, lon, alt;
                                        f_line_eval(line, sl, lat, lon, alt);
                                        /* f_grid_locate without its rim fallback */
                                        const double hx = (lon - x0) * g.inv_dx;
                                        const double hy = (lat - y0) * g.inv_dy;
                                        /* still in the cached cell, and not within `guard` of its
                                         * edges <=> guard < hx - cx < 1 - guard and the same in y:
                                         * for a double, "its upper word, unsigned, is in [that of
                                         * guard + 1, that of 1 - guard)" (a negative one has the
                                         * sign bit there, a NaN the exponent's) */
                                        double fx = hx - cx, fy = hy - cy;
                                        if (going & (max(d_upper_word(fx) - lo_word, d_upper_word(fy) - lo_word) >= span_words)) {
                                                /* another cell of the same grid: what
                                                 * f_grid_elevation does on a cache miss */
                                                const double tx = __builtin_trunc(hx), ty = __builtin_trunc(hy);
                                                const int ix = (int)tx, iy = (int)ty; /* (NaN: 0) */
                                                going = (hx > guard) & (hx < mx) & (hy > guard) & (hy < my);
                                                if (going) {
                                                        const unsigned id = (unsigned)iy * (unsigned)g.nx + (unsigned)ix;
                                                        d_cell_fetch(STACK ? ctx.slots[cell.id >> 24] : g.nodes, g.nbx, ix, iy, cell.lo, cell.hi);
                                                        cell.id = STACK ? ((cell.id & 0xff000000u) | id) : id;
                                                        cx = tx, cy = ty;
                                                        fx = hx - tx, fy = hy - ty;
                                                        decode_nodes();
                                                }
                                        }
                                        /* f_grid_blend */
                                        const double elevation = f_patch(z00, z10, z01, z11, fx, fy) + ctx.offset;
                                        const double t = alt - elevation;
                                        const double clearance = fabs(t);
                                        const double s2 = sl * sl;
                                        going = going & (__builtin_fma(sgn, t, -line.tau) > 0.) &
                                            (__builtin_fma(line.k4, fmin(fmax(clearance, 1.), kLeanClearance), -(s2 * s2)) > 0.);
                                        if (going) {
                                                bx = d_along<FAST>(bx, dx, ds), by = d_along<FAST>(by, dy, ds), bz = d_along<FAST>(bz, dz, ds);
                                                line.tau = line.tau + kLineDrift;
                                                line.s = line.s + ds; /* == sl */
                                                len = len + ds;
                                                count++;
                                                /* d_step_length for one surface: both of its
                                                 * cases are |alt - elevation| */
                                                ds = fmax(clearance * v.slope, v.resolution);
                                        }
                                }
                                const bool stopped = (ray >= 0) & !going;
                                const int n_stopped = __popcll(__ballot(stopped));
                                if (n_stopped == 0) continue;
                                if (POOLED && pooled) stopped_ = stopped;
                                if (POOLED && (role == ROLE_LEAN)) break; /* the pool takes them: see RayPool */
                                if (!sparse) {
                                        /* a busy wave: the lanes that stopped wait while
                                         * enough of the others step on (a group of lean
                                         * steps costs a third of a general iteration, which
                                         * then serves every lane that waits at once); where
                                         * the first group already loses most lanes -- rays
                                         * high above the ground, a new cell every step --
                                         * the wave does not try again for a while */
                                        if (live - n_stopped >= ph.dense_go) continue;
                                        if (it == 0) creep_wait = kCreepBackoff;
                                        break;
                                }
                                break;
                        }
                        my_samples += (ull)(count - count_in); /* a lean step is a sample */
                        PSTAT(11, PSTAT_CLOCK() - t_lean), PSTAT(6, wave_sum((ull)(count - count_in)));
                }
                if (POOLED && (role == ROLE_LEAN)) continue; /* back to the pool: no general iteration */

                /* `drain`: once the queue is dry a wave of phase A hands its rays over
                 * as they stand (between two steps) instead of stepping its last few
                 * to the hand-over count with most lanes idle -- measured with the
                 * hand-over at 512 steps: the queue of C2 is dry after 2.4 ms and the
                 * last wave left at 4.5 ms.  Phase B packs them again. */
                const bool drain = !MODEL && (ph.park_after > 0) && exhausted && (ray >= 0) &&
                    (state == ST_STEP) && (__popcll(__ballot(ray >= 0)) <= ph.drain_lanes);
                bool park = drain;
                const unsigned long long t_gen = PSTAT_CLOCK();
                (void)t_gen;
                PSTAT(8, 1), PSTAT(9, __popcll(__ballot(ray >= 0)));
                TileFault fault = { -1, 0, 0 }; /* the tiles to page in, if any */
                double fx = 0, fy = 0, fz = 0; /* where the ray goes back to, then */
                bool defer = false; /* MODEL: the lane waits for a closed form (see below) */
                bool crossed = false; /* CROSS: the step crossed a boundary: the ray goes on the list */
                if ((ray >= 0) && !drain) {
                        /* ---- one sample at q = B + d * t ---- */
                        double t = 0.;
                        if (state == ST_STEP) t = ds;
                        if (!CROSS && (state == ST_BISECT))
                                t = FAST ? f_bracket_point(ds0, ds1, c0, c1, halvings & 0xffff) : 0.5 * (ds0 + ds1);
                        double qx = bx, qy = by, qz = bz;
                        if (state != ST_INIT) /* B + d*0 == B, but d may be garbage */
                                qx = d_along<FAST>(bx, dx, t), qy = d_along<FAST>(by, dy, t), qz = d_along<FAST>(bz, dz, t);

                        Sample s;
                        if (LINED) {
                                /* B's parameter: -t on a new line (its origin is q),
                                 * and a STEP sample then moves B to q */
                                CellCache * const cache = (MODE != TAMD_MODE_GENERIC) ? &cell : nullptr;
                                bool relay = !f_line_try<MODE>(v, ctx, line, line.s + t, s, cache, !CROSS && (state == ST_BISECT));
                                /* A closed form is a thousand instructions for the
                                 * whole wave, whoever needs it: in a busy wave the
                                 * lanes that do (a ray's first sample, a line at its
                                 * end) wait until there are kRelayBatch of them, or
                                 * until only they are left, or kRelayPatience general
                                 * iterations.  Nothing is committed for a lane that
                                 * waits: it takes this very sample again.  (One map: C2
                                 * -2.4 %.  Through a stack the same costs 6-9 %, with 20
                                 * bytes more of scratch in a kernel held to 168 registers.) */
                                if ((MODE == TAMD_MODE_ONE_MAP) && !sparse) {
                                        const int n_need = __popcll(__ballot(relay));
                                        const int n_here = __popcll(__ballot(true));
                                        const int waited = __builtin_amdgcn_readfirstlane(relay_wait);
                                        const bool now = (n_need >= kRelayBatch) | (n_need == n_here) |
                                            (waited >= kRelayPatience);
                                        relay_wait = ((n_need == 0) | now) ? 0 : waited + 1;
                                        defer = relay & !now;
                                        relay = relay & now;
                                }
                                PSTAT(10, __popcll(__ballot(relay)));
                                if (relay) {
                                        f_line_relay<MODE>(v, ctx, qx, qy, qz, dx, dy, dz, line, s, cache);
                                        line.s = -t;
                                }
                                if ((state == ST_STEP) & !defer) line.s += t;
                        } else
                                d_sample<MODE, FAST>(v, ctx, qx, qy, qz, s,
                                    (FAST && (MODE != TAMD_MODE_GENERIC)) ? &cell : nullptr);
                        /* (a ray that phase A handed over before its line starts -- when
                         * its queue ran dry: which rays, depends on the scheduling -- samples
                         * its position again here: not one of the trace's samples, so that
                         * the count is the same from run to run) */
                        my_samples += (defer || (MODEL && !lined_ && (state == ST_INIT))) ? 0 : 1;
                        if (CAN_FAULT && !defer && (s.fault.centre >= 0)) {
                                /* a tile that is not resident: the ray goes back to
                                 * the arrays as it was BEFORE this sample (before the
                                 * crossing step, if it was bisecting: the bracket is
                                 * not kept) and on the list for the next round */
                                fault = s.fault;
                                if (state == ST_INIT) home = -1; /* a new ray: nothing to keep */
                                const double back = (!CROSS && (state == ST_BISECT)) ? ds : 0.;
                                fx = bx - dx * back, fy = by - dy * back, fz = bz - dz * back;
                        }

                        if (POOLED) stopped_ = defer;
                        /* ---- bookkeeping ----
                         * STEP and BISECT are handled together, as selects rather
                         * than branches: in a busy wave every case is present in
                         * some lane on every trip, so branching buys nothing and
                         * costs exec-mask juggling.  Only INIT (once per ray) and
                         * the two endings (located, done) stay branches. */
                        bool done = false, located = false;
                        if (CAN_FAULT && !defer && (fault.centre < 0) && (state == ST_STEP)) home = s.slot;
                        if ((fault.centre >= 0) | defer) {
                                /* nothing: see below */
                        } else if (state == ST_INIT) {
                                m = s.m, k = s.k;
                                ds = (m >= 0) ? d_step_length(v, s.alt, s.e0, s.e1, m) : 0.;
                                if ((flags & TRACE_CARRY_MEDIUM) && (m >= 0)) {
                                        /* The caller knows which medium the ray
                                         * is in; the sample only sizes the step.
                                         * If the two disagree the ray sits ON the
                                         * boundary between them (the bisection
                                         * left it within 1e-8 m): the distance to
                                         * the nearest surface is ~0 and the
                                         * reference's cached sample would give the
                                         * minimum step [ref stepper.c:812-813]. */
                                        const int given = index[2 * ray];
                                        if ((given >= 0) && (given <= v.n_layers) && (given != m)) {
                                                m = given;
                                                ds = v.resolution;
                                        }
                                }
                                state = ST_STEP;
                                done = (m < 0) || (count >= max_steps);
                        } else if (CROSS) {
                                /* every sample is a STEP sample: it stands, or the ray
                                 * goes on the list of the crossings (below) */
                                const bool same = (s.m == m);
                                const double ds_next = d_step_length(v, s.alt, s.e0, s.e1, s.m);
                                bx = qx, by = qy, bz = qz; /* [ref stepper.c:824] */
                                crossed = !same;           /* [ref stepper.c:832-838] */
                                bm = s.m, bk = s.k;
                                if (MODEL) line.tau = same ? line.tau + kLineDrift : line.tau;
                                len = same ? len + ds : len;
                                k = same ? s.k : k;
                                ds = same ? ds_next : ds; /* a crossing keeps the tentative length */
                                count += same ? 1 : 0;
                                const bool capped = same & (count >= max_steps);
                                done = capped;
                                my_capped += capped ? 1 : 0;
                                park = same & !capped & (ph.park_after > 0) & (count >= ph.park_after);
                                if (MODEL && same && !capped && !park && !lined_ &&
                                    (count >= ph.line_after)) {
                                        lined_ = true; /* (see the other branch) */
                                        line.valid = false, line.s = 0.;
                                        state = ST_INIT;
                                }
                        } else {
                                const bool stepping = (state == ST_STEP);
                                const bool same = (s.m == m);
                                const bool accept = stepping & same;   /* the step stands */
                                const bool cross = stepping & !same;   /* [ref stepper.c:832-838] */
                                const bool other = !same;              /* a sample of another medium */
                                const double ds_next = d_step_length(v, s.alt, s.e0, s.e1, s.m);
                                /* a STEP sample always moves B to q */
                                bx = stepping ? qx : bx, by = stepping ? qy : by, bz = stepping ? qz : bz;
                                if (MODEL) line.tau = accept ? line.tau + kLineDrift : line.tau;
                                len = accept ? len + ds : len;
                                k = accept ? s.k : k;
                                bm = other ? s.m : bm, bk = other ? s.k : bk;
                                /* the sample halved the bracket: the Illinois rule waits (f_bracket_point) */
                                const bool halved = !CROSS && !stepping && f_bracket_halves(ds0, ds1);
                                /* the bracket [ref stepper.c:836, :849-858] */
                                ds0 = cross ? -ds : ((!stepping & same) ? t : ds0);
                                ds1 = cross ? 0. : ((!stepping & other) ? t : ds1);
                                int moved_twice = 0; /* bit 16 / 17 of halvings: the last sample moved ds0 / ds1 */
                                if (FAST) {
                                        /* the clearance where the crossing step began is
                                         * what sized it (more, if the resolution did: a guess) */
                                        const double cl = fmin(fabs(s.alt - s.e0), fabs(s.alt - s.e1));
                                        const bool again0 = !stepping & same & ((halvings & 0x10000) != 0);
                                        const bool again1 = !stepping & other & ((halvings & 0x20000) != 0);
                                        c0 = cross ? ds / v.slope : ((!stepping & same) ? cl : (again1 ? 0.5 * c0 : c0));
                                        c1 = (cross | (!stepping & other)) ? cl : (again0 ? 0.5 * c1 : c1);
                                        moved_twice = (stepping | halved) ? 0 : (same ? 0x10000 : 0x20000);
                                }
                                ds = accept ? ds_next : ds; /* a crossing keeps the tentative length */
                                count += accept ? 1 : 0;
                                /* a bracket of finite doubles is below 1e-8 after at
                                 * most ~1100 halvings; the cap only guards against
                                 * non-finite input (a kernel must always end) */
                                halvings = stepping ? 0 : (((halvings & 0xffff) + 1) | moved_twice);
                                state = cross ? ST_BISECT : state;
                                const bool capped = accept & (count >= max_steps);
                                done = capped;
                                my_capped += capped ? 1 : 0;
                                /* on to the next phase (always at the same step count:
                                 * the line a ray lays there is part of its arithmetic) */
                                park = accept & !capped & (ph.park_after > 0) & (count >= ph.park_after);
                                if (MODEL && accept && !capped && !park && !lined_ &&
                                    (count >= ph.line_after)) {
                                        /* phase B: from here on the ray steps on its line,
                                         * laid by a fresh sample of its position -- what a
                                         * ray handed over at this very step goes through */
                                        lined_ = true;
                                        line.valid = false, line.s = 0.;
                                        state = ST_INIT;
                                }
                                located = (state == ST_BISECT) &
                                    (!(ds1 - ds0 > 1E-08) | ((halvings & 0xffff) > 1200));
                        }
                        if (located) { /* [ref stepper.c:861-863] */
                                bx = d_along<FAST>(bx, dx, ds1), by = d_along<FAST>(by, dy, ds1), bz = d_along<FAST>(bz, dz, ds1);
                                len += ds + ds1;
                                count++;
                                m = bm, k = bk;
                                done = true;
                        }
                        if (done) {
                                if (ph.out.order_of != nullptr) { /* to the caller's arrays, the ray's place there */
                                        const long o = ph.out.order_of[ray];
                                        ph.out.pos[3 * o] = bx, ph.out.pos[3 * o + 1] = by, ph.out.pos[3 * o + 2] = bz;
                                        ph.out.index[2 * o] = m, ph.out.index[2 * o + 1] = k;
                                        ph.out.length[o] = len;
                                        ph.out.n_steps[o] = count;
                                } else {
                                        pos[3 * ray] = bx, pos[3 * ray + 1] = by, pos[3 * ray + 2] = bz;
                                        index[2 * ray] = m, index[2 * ray + 1] = k;
                                        if (length) length[ray] = len;
                                        if (n_steps) n_steps[ray] = count;
                                }
                                my_rays++;
                                my_steps += (ull)(count - count0);
                                ray = -1;
                        }
                }
                PSTAT(12, PSTAT_CLOCK() - t_gen);
                /* ---- park over-long rays (phase A; whole wave takes part) ---- */
                if (!MODEL && (ph.ds_mark != nullptr) && (ray >= 0) && (state == ST_STEP) &&
                    (count == ph.mark_at))
                        ph.ds_mark[ray] = ds;
                const ull pmask = __ballot(park);
                if (pmask != 0) {
                        /* Phase A sorts what it hands over.  A launch of phase B ends with
                         * the chip all but empty, waiting for the few rays of thousands of
                         * steps -- the later one of those was drawn from the queue, the
                         * longer.  A ray whose steps shrank from d0 (at step mark_at) to ds
                         * now will, at that rate, be down to the minimum step after
                         *   ln(ds / resolution) / (ln(d0 / ds) / (count - mark_at))
                         * more: a crude figure that tells what matters -- the rays heading
                         * straight for the ground have little there (of C2's rays at step 32
                         * the 40 % below 120 hold none of the 4 % that take over 500 further
                         * steps, nor any of the 0.1 % over 2 000), and they go to the back of
                         * the list.  Where a ray is listed changes when phase B takes it, not
                         * what comes out. */
                        bool back = false;
                        if (!MODEL && (ph.n_parked_back != nullptr) && park && (count > ph.mark_at)) {
                                const float shrink = __logf((float)ph.ds_mark[ray] / (float)ds);
                                const float togo = __logf((float)ds / (float)v.resolution);
                                back = (shrink > 0.f) &&
                                    !(togo * (float)(count - ph.mark_at) > ph.long_if * shrink);
                        }
                        const ull bmask = __ballot(back);
                        const ull fmask = pmask & ~bmask;
                        const int leader = __builtin_ctzll(pmask);
                        ull base = 0, base_back = 0;
                        if ((int)(threadIdx.x & 63) == leader) {
                                if (fmask != 0) base = atomicAdd(ph.n_parked, (ull)__popcll(fmask));
                                if (bmask != 0) base_back = atomicAdd(ph.n_parked_back, (ull)__popcll(bmask));
                        }
                        base = __shfl(base, leader, 64);
                        base_back = __shfl(base_back, leader, 64);
                        if (park) {
                                const ull mine = back ? bmask : fmask;
                                const int rank = lane_rank(mine);
                                const long place = back ? capacity - 1 - (long)(base_back + rank) : (long)(base + rank);
                                ph.parked[place] = (int)ray;
                                if (!MODEL && (ph.sort_key != nullptr)) {
                                        /* The lined pass ends waiting for its longest rays, and the
                                         * later one of those is drawn, the longer: the front of the
                                         * list is ordered by how shallow a ray goes -- the sine of its
                                         * elevation angle, d . up (up ~ B / |B|: the geocentric
                                         * vertical, 0.2 degrees off at most) -- the shallowest first:
                                         * they are the ones that skim the ground for thousands of
                                         * steps (measured by ordering a batch's INPUT that way: C2 3.37
                                         * -> 3.01 ms).  The back of the list (rays that cannot be long)
                                         * keeps its place behind everything: the largest key. */
                                        const double up = __builtin_fma(dx, bx, __builtin_fma(dy, by, dz * bz)) *
                                            __builtin_amdgcn_rsq(__builtin_fma(bx, bx, __builtin_fma(by, by, bz * bz)));
                                        /* (one byte: 253 levels up to 14 degrees -- one pass of the sort;
                                         * 254 is a place nobody filled, 255 the back) */
                                        /* (tried instead: the steps the ray would take over flat ground at
                                         * that angle from its clearance, on a log scale: no better) */
                                        const double scaled = fmin(fabs(up) * 1024., 253.);
                                        ph.sort_key[place] = back ? (unsigned char)255 : (unsigned char)scaled;
                                }
                                pos[3 * ray] = bx, pos[3 * ray + 1] = by, pos[3 * ray + 2] = bz;
                                index[2 * ray] = m, index[2 * ray + 1] = k;
                                length[ray] = len;
                                n_steps[ray] = count;
                                my_steps += (ull)(count - count0);
                                ray = -1;
                        }
                }
                /* ---- list the rays that crossed a boundary (whole wave takes part) ---- */
                if (CROSS) {
                        const ull cmask = __ballot(crossed);
                        if (cmask != 0) {
                                const int leader = __builtin_ctzll(cmask);
                                ull base = 0;
                                /* (TAIL: L2, from the far end, once the wave has said that it lists
                                 * no more into L1 -- a ray crosses once: the two never meet) */
                                const bool far = TAIL && (tail_peek < 0);
                                if ((int)(threadIdx.x & 63) == leader)
                                        base = atomicAdd(far ? tail.l2_count() : ph.cross.count, (ull)__popcll(cmask));
                                base = __shfl(base, leader, 64);
                                if (crossed) {
                                        const int rank = lane_rank(cmask);
                                        const long place = far ? capacity - 1 - (long)(base + rank) : (long)(base + rank);
                                        ph.cross.ray[place] = (int)ray;
                                        ph.cross.ds[place] = ds;
                                        ph.cross.other[place] = cross_pack(bm, bk);
                                        /* B is the tentative point; m, k the medium it left */
                                        pos[3 * ray] = bx, pos[3 * ray + 1] = by, pos[3 * ray + 2] = bz;
                                        index[2 * ray] = m, index[2 * ray + 1] = k;
                                        length[ray] = len;
                                        n_steps[ray] = count;
                                        my_steps += (ull)(count - count0);
                                        ray = -1;
                                }
                        }
                }
                /* ---- list the rays that wait for a tile (whole wave takes part) ---- */
                if (CAN_FAULT && (ph.pg.faulted != nullptr)) {
                        const bool waits = fault.centre >= 0;
                        if (waits) {
                                pos[3 * ray] = fx, pos[3 * ray + 1] = fy, pos[3 * ray + 2] = fz;
                                if (state != ST_INIT) /* else: what the caller gave, or nothing */
                                        index[2 * ray] = m, index[2 * ray + 1] = k;
                                else if (!(flags & TRACE_CARRY_MEDIUM))
                                        index[2 * ray] = -1, index[2 * ray + 1] = -1;
                                if (length) length[ray] = len;
                                if (n_steps) n_steps[ray] = count;
                                /* the step it was about to take (a bisecting ray went
                                 * back before its crossing step: the same one) */
                                ph.pg.tentative[ray] = (state != ST_INIT) ? ds : -1.;
                                my_steps += (ull)(count - count0);
                        }
                        /* a bisecting ray also wants the tile of its crossing sample */
                        page_fault(ph.pg, fault, ray, (!CROSS && (state == ST_BISECT)) ? home : -1);
                        if (waits) ray = -1;
                }
        }

#ifdef TRACE_POOL_STATS
        if (MODEL && ((threadIdx.x & 63) == 0))
                for (int i = 0; i < 24; i++)
                        if (pstat_[i]) atomicAdd(&g_pool_stats[i], pstat_[i]);
#endif
        /* ---- TAIL: the wave has no ray left: if L1 is final it locates L1's crossings ---- */
        if constexpr (TAIL) {
                if (flags & TRACE_CROSS_TAIL) {
                        const int lane = (int)(threadIdx.x & 63);
                        const ull n_dry = __hip_atomic_load(tail.n_dry(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if (__builtin_amdgcn_readfirstlane((int)(n_dry == (ull)gridDim.x * 4) /* blocks of four waves */) != 0) {
                                /* one acquire, ahead of the first load of anything handed over: the
                                 * list's entries and the listed rays' position, medium, length, steps */
                                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                                __builtin_amdgcn_s_setprio(0);
                                const ull l1_ = __hip_atomic_load(ph.cross.count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                                const long l1 = (long)__shfl(l1_, 0, 64);
                                for (;;) {
                                        ull ticket = 0;
                                        if (lane == 0) ticket = atomicAdd(tail.l1_next(), 64ull);
                                        ticket = __shfl(ticket, 0, 64);
                                        if ((long)ticket >= l1) break;
                                        ull got_rays = 0, got_samples = 0;
                                        cross_locate<MODE, true, false>(v, ctx, pos, dir, index, length, n_steps, ph.cross,
                                            ph.pg, ph.out, (long)ticket, 64, lane, min((long)ticket + 64, l1), got_rays,
                                            got_samples);
                                        /* (k_cross's additions: a crossing is a ray and a step) */
                                        my_rays += got_rays, my_steps += got_rays, my_samples += got_samples;
                                }
                        }
                }
        }
        block_tally(stats, my_rays, my_steps, my_samples, my_capped);
}

/* Where a ray STARTS, as one byte: the cell of a 16 x 16 raster over the map or the stack's
 * lattice that holds its origin (rays outside go to the rim's cells).  The trace then takes the
 * rays cell by cell (run_trace: one pass of a radix sort on these keys): the 64 rays of a wave
 * start within a few kilometres of each other and meet the same tiles, the same pages and -- for a
 * while -- the same cache lines.  Ordering a batch's INPUT that way was worth 19 % on C3 (16 tiles,
 * 415 MB: 25.7 -> 20.8 ms), 7 % on C4, 4 % on C5; this does it inside the library, whatever order
 * the caller's rays come in, and leaves the caller's arrays where they are (the passes read the
 * rays through the ordered list of their numbers). */
#ifndef SPATIAL_CELLS
#define SPATIAL_CELLS 16
#endif
#if SPATIAL_CELLS <= 16
#define SPATIAL_KEY_T unsigned char
#define SPATIAL_BITS 8
#else
#define SPATIAL_KEY_T unsigned short
#define SPATIAL_BITS 16
#endif
template <int MODE>
__global__ void k_ray_cells(tamd_view v, long n, const double * __restrict__ pos,
    SPATIAL_KEY_T * __restrict__ key, int * __restrict__ id)
{
        const tamd_meta mt = v.metas[0];
        constexpr int kCells = SPATIAL_CELLS;
        double x0, y0, sx, sy; /* the box: longitude, latitude; cells / its extent */
        if (MODE == TAMD_MODE_ONE_MAP) {
                const tamd_grid & g = v.grids[mt.src];
                x0 = g.x0, y0 = g.y0;
                sx = kCells / (g.dx * (g.nx - 1)), sy = kCells / (g.dy * (g.ny - 1));
        } else {
                const tamd_stack & st = v.stacks[mt.src];
                x0 = st.lon0, y0 = st.lat0;
                sx = kCells / (st.dlon * st.nlon), sy = kCells / (st.dlat * st.nlat);
        }
        for (long r = blockIdx.x * (long)blockDim.x + threadIdx.x; r < n; r += (long)gridDim.x * blockDim.x) {
                double lat, lon, alt;
                f_to_geodetic(pos[3 * r], pos[3 * r + 1], pos[3 * r + 2], lat, lon, alt);
                const int bx = (int)fmin(fmax((lon - x0) * sx, 0.), (double)(kCells - 1));
                const int by = (int)fmin(fmax((lat - y0) * sy, 0.), (double)(kCells - 1)); /* (NaN: 0) */
                key[r] = (SPATIAL_KEY_T)(by * kCells + bx);
                id[r] = (int)r;
        }
}

/* The least waves a SIMD the kernel must fit (registers: 512 / waves).  The lined
 * pass is bound by what the SIMD issues, with a memory wait every few steps: a
 * third wave is worth more than the few values that go to scratch for it (one
 * map: 169 registers -> 168, none; a stack: 188 -> 168 and 64 bytes). */
#ifndef TRACE_LINED_WAVES
#define TRACE_LINED_WAVES 3
#endif
#ifndef TRACE_A_WAVES
#define TRACE_A_WAVES 1
#endif
template <int MODE, bool FAST, bool MODEL, bool PAGED>
constexpr int trace_waves()
{
        return (FAST && MODEL && !PAGED && (MODE != TAMD_MODE_GENERIC)) ? TRACE_LINED_WAVES :
               (FAST && !MODEL && !PAGED && (MODE != TAMD_MODE_GENERIC)) ? TRACE_A_WAVES : 1;
}

template <int MODE, bool FAST, bool MODEL, bool PAGED, bool CROSS, bool POOL = false>
__global__ void __launch_bounds__(256)
__attribute__((amdgpu_waves_per_eu(trace_waves<MODE, FAST, MODEL, PAGED>())))
k_trace(tamd_view v, long n,
    double * __restrict__ pos, const double * __restrict__ dir, int max_steps,
    int * __restrict__ index, double * __restrict__ length, int * __restrict__ n_steps,
    int flags, PhaseIO ph, ull * __restrict__ stats, ull * __restrict__ queue)
{
        trace_body<MODE, FAST, MODEL, PAGED, CROSS, POOL>(v, n, pos, dir, max_steps, index, length, n_steps, flags,
            ph, stats, queue);
}

/* The first pass of a fast trace over one map or one stack, flat: a ray a lane, no queue.
 *
 * Nearly every ray of a batch outlives the hand-over at step `park` (C2: 999 819 of 10^6 take
 * more than 32 steps), so what phase A does is the same in every lane -- the origin sample, `park`
 * closed-form steps, the hand-over -- and the persistent kernel's refill queue, its `drain` and the
 * branches of its state machine serve a divergence that is not there: they cost it a third of its
 * vector instructions (scalar registers spilled to vector lanes and read back inside the step).
 * Here a wave loads its 64 rays, steps them `park` times (or until none is left) and hands over
 * ALL AT ONCE: the rays that ended write their results, the others go on the hand-over list or
 * on the crossings' list L1, exactly as trace_body's phase A leaves them -- the same functions on
 * the same values in the same order, so every result and every total is the same bit for bit;
 * only the order of the lists differs, as it does from run to run anyway.  The places on a list
 * are reserved once per BLOCK (its four waves park at the same moment: a prefix in LDS, then at
 * most three atomics), not per wave.
 * run_trace launches it where the rule there holds; everywhere else k_trace<..., MODEL = false>. */
struct FirstPass {
        int park;               /* the hand-over's step count: 0 < park < max_steps */
        int mark_at;            /* the sorted hand-over, as PhaseIO's: */
        float long_if;
        int * parked;
        ull * n_parked, * n_parked_back; /* (n_parked_back NULL: one end) */
        unsigned char * sort_key;        /* (or NULL) */
        CrossList cross;                 /* L1 */
        /* rays in an order of the library's own (or NULLs: see PhaseIO) */
        const double * pos_in, * dir_in;
        const int * index_in;
        double * dir_copy;
};

/* WAVES: the most waves a SIMD may hold (8: as many as the registers allow; see first_pass_waves) */
template <int MODE, int WAVES>
__global__ void __launch_bounds__(256)
__attribute__((amdgpu_waves_per_eu(1, WAVES)))
k_first(tamd_view v, long n, double * __restrict__ pos, const double * __restrict__ dir, int max_steps,
    int * __restrict__ index, double * __restrict__ length, int * __restrict__ n_steps, int flags,
    FirstPass fp, RayOut out, ull * __restrict__ stats)
{
        __shared__ unsigned wave_n[4][3]; /* [wave][list]: front, back, crossings */
        __shared__ ull block_base[3];
        OneCtx ctx;
        d_load_ctx<MODE, true>(v, ctx);
        CellCache cell = { ~0u, 0u, 0u, -1, nullptr };
        const int wave = (int)(threadIdx.x >> 6);
        ull my_rays = 0, my_steps = 0, my_samples = 0, my_capped = 0;

        /* (block-uniform: every thread of a block meets the barriers below) */
        for (long first = blockIdx.x * 256L; first < n; first += gridDim.x * 256L) {
                const long ray = first + threadIdx.x;
                const bool have = ray < n;
                double bx = 0, by = 0, bz = 0, dx = 0, dy = 0, dz = 0, len = 0, ds = 0, d0 = 0;
                int m = -1, k = -1, bm = -1, bk = -1, count = 0;
                bool done = false, crossed = false;
                if (have) {
                        /* ---- the ray ---- */
                        int given = -1;
                        if (fp.dir_copy != nullptr) {
                                const long src = out.order_of[ray];
                                bx = fp.pos_in[3 * src], by = fp.pos_in[3 * src + 1], bz = fp.pos_in[3 * src + 2];
                                dx = fp.dir_in[3 * src], dy = fp.dir_in[3 * src + 1], dz = fp.dir_in[3 * src + 2];
                                fp.dir_copy[3 * ray] = dx, fp.dir_copy[3 * ray + 1] = dy, fp.dir_copy[3 * ray + 2] = dz;
                                if (flags & TRACE_CARRY_MEDIUM) {
                                        given = fp.index_in[2 * src];
                                        index[2 * ray] = given, index[2 * ray + 1] = fp.index_in[2 * src + 1];
                                }
                        } else {
                                bx = pos[3 * ray], by = pos[3 * ray + 1], bz = pos[3 * ray + 2];
                                dx = dir[3 * ray], dy = dir[3 * ray + 1], dz = dir[3 * ray + 2];
                                if (flags & TRACE_CARRY_MEDIUM) given = index[2 * ray];
                        }
                        /* ---- the origin sample (trace_body's INIT) ---- */
                        Sample s;
                        d_sample<MODE, true>(v, ctx, bx, by, bz, s, &cell);
                        my_samples++;
                        m = s.m, k = s.k;
                        ds = (m >= 0) ? d_step_length(v, s.alt, s.e0, s.e1, m) : 0.;
                        if ((flags & TRACE_CARRY_MEDIUM) && (m >= 0)) {
                                /* (the given medium wins: see trace_body) */
                                if ((given >= 0) && (given <= v.n_layers) && (given != m)) {
                                        m = given;
                                        ds = v.resolution;
                                }
                        }
                        done = (m < 0) || (count >= max_steps);
                        if (fp.mark_at == 0) d0 = ds;
                }
                /* ---- at most `park` closed-form steps (trace_body's CROSS bookkeeping) ---- */
                bool live = have && !done;
                for (int trip = 0; trip < fp.park; trip++) {
                        if (__ballot(live) == 0) break;
                        if (live) {
                                const double qx = d_along<true>(bx, dx, ds), qy = d_along<true>(by, dy, ds),
                                    qz = d_along<true>(bz, dz, ds);
                                Sample s;
                                d_sample<MODE, true>(v, ctx, qx, qy, qz, s, &cell);
                                my_samples++;
                                const bool same = (s.m == m);
                                const double ds_next = d_step_length(v, s.alt, s.e0, s.e1, s.m);
                                bx = qx, by = qy, bz = qz;
                                crossed = !same;
                                bm = s.m, bk = s.k;
                                len = same ? len + ds : len;
                                k = same ? s.k : k;
                                ds = same ? ds_next : ds; /* a crossing keeps the tentative length */
                                count += same ? 1 : 0;
                                const bool capped = same & (count >= max_steps);
                                done = capped;
                                my_capped += capped ? 1 : 0;
                                d0 = (same & (count == fp.mark_at)) ? ds : d0;
                                live = same & !capped & (count < fp.park);
                        }
                }
                /* ---- the hand-over: the whole block, once ---- */
                const bool park = have & !done & !crossed; /* (count == fp.park: the loop's bound) */
                bool back = false;
                if (park && (fp.n_parked_back != nullptr) && (count > fp.mark_at)) {
                        /* (the long-ray predictor: see where trace_body parks) */
                        const float shrink = __logf((float)d0 / (float)ds);
                        const float togo = __logf((float)ds / (float)v.resolution);
                        back = (shrink > 0.f) && !(togo * (float)(count - fp.mark_at) > fp.long_if * shrink);
                }
                const ull bmask = __ballot(back);
                const ull fmask = __ballot(park) & ~bmask;
                const ull cmask = __ballot(crossed);
                if ((threadIdx.x & 63) == 0) {
                        wave_n[wave][0] = (unsigned)__popcll(fmask);
                        wave_n[wave][1] = (unsigned)__popcll(bmask);
                        wave_n[wave][2] = (unsigned)__popcll(cmask);
                }
                __syncthreads();
                if (threadIdx.x < 3) {
                        const ull sum = (ull)wave_n[0][threadIdx.x] + wave_n[1][threadIdx.x] + wave_n[2][threadIdx.x] +
                            wave_n[3][threadIdx.x];
                        ull * const counter = (threadIdx.x == 0) ? fp.n_parked :
                            ((threadIdx.x == 1) ? fp.n_parked_back : fp.cross.count);
                        block_base[threadIdx.x] = (sum != 0) ? atomicAdd(counter, sum) : 0;
                }
                __syncthreads();
                ull base[3];
                for (int l = 0; l < 3; l++) {
                        base[l] = block_base[l];
                        for (int w = 0; w < 3; w++) base[l] += (w < wave) ? wave_n[w][l] : 0u;
                }
                __syncthreads(); /* (the next chunk writes wave_n again) */
                if (done) {
                        if (out.order_of != nullptr) { /* to the caller's arrays, the ray's place there */
                                const long o = out.order_of[ray];
                                out.pos[3 * o] = bx, out.pos[3 * o + 1] = by, out.pos[3 * o + 2] = bz;
                                out.index[2 * o] = m, out.index[2 * o + 1] = k;
                                out.length[o] = len;
                                out.n_steps[o] = count;
                        } else {
                                pos[3 * ray] = bx, pos[3 * ray + 1] = by, pos[3 * ray + 2] = bz;
                                index[2 * ray] = m, index[2 * ray + 1] = k;
                                length[ray] = len;
                                n_steps[ray] = count;
                        }
                        my_rays++;
                        my_steps += (ull)count;
                }
                if (park | crossed) {
                        if (park) {
                                const long place = back ? n - 1 - (long)(base[1] + lane_rank(bmask)) :
                                    (long)(base[0] + lane_rank(fmask));
                                fp.parked[place] = (int)ray;
                                if (fp.sort_key != nullptr) {
                                        /* (how shallow the ray goes: see where trace_body parks) */
                                        const double up = __builtin_fma(dx, bx, __builtin_fma(dy, by, dz * bz)) *
                                            __builtin_amdgcn_rsq(__builtin_fma(bx, bx, __builtin_fma(by, by, bz * bz)));
                                        const double scaled = fmin(fabs(up) * 1024., 253.);
                                        fp.sort_key[place] = back ? (unsigned char)255 : (unsigned char)scaled;
                                }
                        } else {
                                const long place = (long)(base[2] + lane_rank(cmask));
                                fp.cross.ray[place] = (int)ray;
                                fp.cross.ds[place] = ds;
                                fp.cross.other[place] = cross_pack(bm, bk);
                        }
                        /* (a crossing: B is the tentative point; m, k the medium it left) */
                        pos[3 * ray] = bx, pos[3 * ray + 1] = by, pos[3 * ray + 2] = bz;
                        index[2 * ray] = m, index[2 * ray + 1] = k;
                        length[ray] = len;
                        n_steps[ray] = count;
                        my_steps += (ull)count;
                }
        }
        block_tally(stats, my_rays, my_steps, my_samples, my_capped);
}

/* The crossings of a trace, every lane busy: for each listed ray the bracket
 * [-ds, 0] behind its tentative point q is narrowed below 1e-8 m [ref
 * stepper.c:832-864] -- by halving, on closed-form samples, in the reference's
 * arithmetic; in the fast one by false position (f_bracket_point) on the line
 * that the closed form lays AT q: it has no drift (the samples all leave from q)
 * and serves every sample within its reach, ~500 m; beyond, a sample is a closed
 * form that lays the next line.  The first sample is q again: the trace kernel
 * decided there that the medium changed (`other`), by this very closed form or
 * by the ray's line within its error bound of it; where the two disagree (a
 * boundary within 1e-9 m of q) the trace kernel's word stands, so that a listed
 * ray always ends here.  A ray that needs a tile which is not resident goes back
 * before its step and on the pager's list, as in k_trace. */
/* The entries [lo, hi) of the list: the caller's lanes take entry i0 + lane of each round i0 = first,
 * first + stride, ... (whole waves go round: page_fault).  k_cross calls it, a block a round, and
 * so does the lined pass, a wave a ticket (see CrossTail). */
template <int MODE, bool FAST, bool PAGED>
__device__ __forceinline__ void cross_locate(const tamd_view & v, const OneCtx & ctx, double * __restrict__ pos,
    const double * __restrict__ dir, int * __restrict__ index, double * __restrict__ length,
    int * __restrict__ n_steps, const CrossList & cross, const Paging & pg, const RayOut & out, long first,
    long stride, int lane, long hi, ull & my_rays, ull & my_samples)
{
        constexpr bool CAN_FAULT = PAGED && (MODE != TAMD_MODE_ONE_MAP);
        const long n = hi;
        for (long i0 = first; i0 < n; i0 += stride) {
                const long i = i0 + lane;
                TileFault fault = { -1, 0, 0 };
                int home = -1;
                long r = -1;
                if (i < n) {
                        r = cross.ray[i];
                        const double ds = cross.ds[i];
                        int bm, bk;
                        cross_unpack(cross.other[i], bm, bk);
                        const double px = pos[3 * r], py = pos[3 * r + 1], pz = pos[3 * r + 2];
                        const double dx = dir[3 * r], dy = dir[3 * r + 1], dz = dir[3 * r + 2];
                        const int medium0 = index[2 * r];
                        CellCache cell = { ~0u, 0u, 0u, -1, nullptr };
                        CellCache * cache = (FAST && (MODE != TAMD_MODE_GENERIC)) ? &cell : nullptr;
                        Sample s;
                        RayLine line;
                        double at = 0.; /* q's parameter on the line */
                        if (FAST) {
                                f_to_geodetic(px, py, pz, s.lat, s.lon, s.alt, &line, dx, dy, dz);
                                d_classify<MODE, true>(v, ctx, s, cache);
                        } else
                                d_sample<MODE, false>(v, ctx, px, py, pz, s, cache);
                        my_samples++;
                        if (CAN_FAULT) fault = s.fault, home = s.slot;
                        const bool agreed = (fault.centre < 0) && (s.m != medium0);
                        if (agreed) bm = s.m, bk = s.k;
                        double ds0 = -ds, ds1 = 0.;
                        /* the clearances at the two ends (f_bracket_point): the one where
                         * the step began is what sized it (more, if the resolution did) */
                        double c0 = ds / v.slope;
                        double c1 = agreed ? fmin(fabs(s.alt - s.e0), fabs(s.alt - s.e1)) : 0.;
                        int taken = 0, last = 0; /* last: the end the previous sample moved (1: ds0, 2: ds1) */
                        while ((fault.centre < 0) && (ds1 - ds0 > 1E-08) && (taken <= 1200)) {
                                const bool halving = f_bracket_halves(ds0, ds1); /* (no Illinois rule then) */
                                const double t = FAST ? f_bracket_point(ds0, ds1, c0, c1, taken) :
                                                        0.5 * (ds0 + ds1);
                                const double qx = d_along<FAST>(px, dx, t), qy = d_along<FAST>(py, dy, t), qz = d_along<FAST>(pz, dz, t);
                                Sample s2;
                                if (FAST) {
                                        if (!f_line_try<MODE>(v, ctx, line, at + t, s2, cache, true)) {
                                                f_line_relay<MODE>(v, ctx, qx, qy, qz, dx, dy, dz, line, s2, cache);
                                                at = -t; /* a new line, laid at this sample */
                                        }
                                } else
                                        d_sample<MODE, false>(v, ctx, qx, qy, qz, s2, cache);
                                my_samples++, taken++;
                                if (CAN_FAULT && (s2.fault.centre >= 0)) {
                                        fault = s2.fault;
                                } else if (s2.m == medium0) {
                                        ds0 = t;
                                        if (FAST) {
                                                c0 = fmin(fabs(s2.alt - s2.e0), fabs(s2.alt - s2.e1));
                                                if (last == 1) c1 = 0.5 * c1; /* the Illinois rule */
                                                last = halving ? 0 : 1;
                                        }
                                } else {
                                        ds1 = t;
                                        bm = s2.m, bk = s2.k;
                                        if (FAST) {
                                                c1 = fmin(fabs(s2.alt - s2.e0), fabs(s2.alt - s2.e1));
                                                if (last == 2) c0 = 0.5 * c0;
                                                last = halving ? 0 : 2;
                                        }
                                }
                        }
                        if (fault.centre >= 0) {
                                /* back before the step, which the next round takes again */
                                pos[3 * r] = px - dx * ds, pos[3 * r + 1] = py - dy * ds, pos[3 * r + 2] = pz - dz * ds;
                                pg.tentative[r] = ds;
                        } else if (out.order_of != nullptr) { /* (RayOut: the caller's arrays) */
                                const long o = out.order_of[r];
                                out.pos[3 * o] = d_along<FAST>(px, dx, ds1), out.pos[3 * o + 1] = d_along<FAST>(py, dy, ds1),
                                out.pos[3 * o + 2] = d_along<FAST>(pz, dz, ds1);
                                out.index[2 * o] = bm, out.index[2 * o + 1] = bk;
                                out.length[o] = length[r] + (ds + ds1);
                                out.n_steps[o] = n_steps[r] + 1;
                                my_rays++;
                        } else { /* [ref stepper.c:861-863] */
                                pos[3 * r] = d_along<FAST>(px, dx, ds1), pos[3 * r + 1] = d_along<FAST>(py, dy, ds1),
                                pos[3 * r + 2] = d_along<FAST>(pz, dz, ds1);
                                index[2 * r] = bm, index[2 * r + 1] = bk;
                                length[r] = length[r] + (ds + ds1);
                                n_steps[r] = n_steps[r] + 1;
                                my_rays++;
                        }
                }
                if (CAN_FAULT && (pg.faulted != nullptr)) page_fault(pg, fault, r, home);
        }
}

/* What the lined pass left: of the list's front (see CrossTail) the entries from `front.l1_next` on --
 * all of it where no lined pass located any (front.words NULL) -- and the entries at its far end,
 * front.l2_count of them below `capacity`. */
template <int MODE, bool FAST, bool PAGED>
__global__ void __launch_bounds__(256) k_cross(tamd_view v, double * __restrict__ pos,
    const double * __restrict__ dir, int * __restrict__ index, double * __restrict__ length,
    int * __restrict__ n_steps, CrossList cross, Paging pg, ull * __restrict__ stats, RayOut out,
    CrossTail front, long capacity)
{
        OneCtx ctx;
        d_load_ctx<MODE, FAST>(v, ctx);
        const long n = (long)*cross.count;
        const long done = (front.words != nullptr) ? min((long)*front.l1_next(), n) : 0;
        const long n_back = (front.words != nullptr) ? (long)*front.l2_count() : 0;
        const long first = blockIdx.x * (long)blockDim.x, stride = (long)gridDim.x * blockDim.x;
        ull my_rays = 0, my_samples = 0;
#pragma unroll 1
        for (int part = 0; part < 2; part++) { /* (one copy of the body) */
                const long lo = (part == 0) ? done : capacity - n_back, hi = (part == 0) ? n : capacity;
                cross_locate<MODE, FAST, PAGED>(v, ctx, pos, dir, index, length, n_steps, cross, pg, out, lo + first,
                    stride, (int)threadIdx.x, hi, my_rays, my_samples);
        }
        block_tally(stats, my_rays, my_rays, my_samples, 0);
}

/* ---- a whole scattering walk per ray ----------------------------------------
 *
 * turtle_stepper_scatter_n over a geometry with every tile resident: each lane
 * takes a ray through ALL its generations, the ray's state in registers from
 * its first step to its last -- where the generation-by-generation form
 * (k_step + k_bisect per generation) streams 136 bytes of it out and in again
 * at every step, which is what bounds that form.  Same state
 * machine as k_trace, one sample per live lane and trip whatever the lane is
 * doing (stepping, or bisecting a crossing: lanes need not be at the same
 * generation), with two differences: an accepted step ends a generation (a new
 * direction from Philox(first + ray, generation; seed)), and a located crossing
 * does not end the ray but moves it into the medium it entered, from the last
 * sample the bisection took there [ref stepper.c:849-858: that sample is what
 * turtle_stepper_step publishes and caches for the next call].  Same arithmetic
 * on the same values as the generation-by-generation form: same bits.
 * Persistent waves, rays from a queue (wave-aggregated draws), as in k_trace. */
struct WalkIO {
        ull seed;
        long first;      /* the global index of ray 0 */
        int first_step;  /* the generation of the first step */
        int n_steps;     /* generations to take */
};

#ifndef WALK_WAVES_ATTR
#define WALK_WAVES_ATTR
#endif
template <int MODE, bool FAST>
__global__ void __launch_bounds__(256) WALK_WAVES_ATTR k_walk(tamd_view v, long n, double * __restrict__ pos,
    double * __restrict__ alt, double * __restrict__ elev, int * __restrict__ index,
    double * __restrict__ length, int * __restrict__ steps, WalkIO io, ull * __restrict__ stats,
    ull * __restrict__ queue)
{
        RayQueue q;
        OneCtx ctx;
        d_load_ctx<MODE, FAST>(v, ctx);
        CellCache cell = { ~0u, 0u, 0u, -1, nullptr };
        CellCache * cache = (FAST && (MODE != TAMD_MODE_GENERIC)) ? &cell : nullptr;

        long ray = -1;
        bool dead = false;
        int state = ST_STEP, count = 0;
        double bx = 0, by = 0, bz = 0, dx = 0, dy = 0, dz = 0, len = 0;
        double ds = 0;
        double s_alt = 0, s_e0 = 0, s_e1 = 0; /* the sample the ray stands on */
        Bisection b = { 0., 0., 0., 0., 0., -1, -1, 0 };
        int m = -1, k = -1;
        ull my_rays = 0, my_steps = 0, my_samples = 0, my_plain = 0;

        for (;;) {
                queue_refill(q, queue, kChunk, n, ray, dead, [&] {
                        m = index[2 * ray], k = index[2 * ray + 1];
                        if ((m < 0) || (io.n_steps <= 0)) {
                                ray = -1; /* has left the data: no further step */
                        } else {
                                bx = pos[3 * ray], by = pos[3 * ray + 1], bz = pos[3 * ray + 2];
                                s_alt = alt[ray], s_e0 = elev[2 * ray], s_e1 = elev[2 * ray + 1];
                                /* the sum goes on where it stands: the same roundings
                                 * in one call as in several */
                                len = length[ray], count = 0, state = ST_STEP;
                                ds = d_step_length(v, s_alt, s_e0, s_e1, m);
                                d_isotropic((ull)(io.first + ray), (ull)io.first_step, io.seed, dx, dy, dz);
                        }
                });
                if (__ballot(ray >= 0) == 0) {
                        if (q.exhausted) break;
                        continue; /* (every ray drawn had left the data: draw again) */
                }
                if (ray >= 0) {
                        /* ---- one sample at q = B + d * t ---- */
                        const bool stepping = (state == ST_STEP);
                        const double t = stepping ? ds : 0.5 * (b.ds0 + b.ds1);
                        const double qx = bx + dx * t, qy = by + dy * t, qz = bz + dz * t;
                        Sample s;
                        d_sample<MODE, FAST>(v, ctx, qx, qy, qz, s, cache);
                        my_samples++;
                        /* ---- bookkeeping: the step machine of turtle_amd_device.h ---- */
                        const StepOutcome o = step_or_bisect(b, state, bx, by, bz, m, ds, t, qx, qy, qz, s);
                        my_steps += stepping ? 1 : 0;
                        my_plain += o.accept ? 1 : 0;
                        bool ended = o.accept;
                        if (o.accept) {
                                len += ds, k = s.k;
                                s_alt = s.alt, s_e0 = s.e0, s_e1 = s.e1;
                        }
                        if (o.located) { /* [ref stepper.c:861-863] */
                                bx = bx + dx * b.ds1, by = by + dy * b.ds1, bz = bz + dz * b.ds1;
                                len += ds + b.ds1;
                                m = b.bm, k = b.bk;
                                s_alt = b.b_alt, s_e0 = b.b_e0, s_e1 = b.b_e1;
                                state = ST_STEP;
                                ended = true;
                        }
                        if (ended) { /* a generation is over */
                                count++;
                                if ((m < 0) || (count >= io.n_steps)) {
                                        pos[3 * ray] = bx, pos[3 * ray + 1] = by, pos[3 * ray + 2] = bz;
                                        alt[ray] = s_alt;
                                        elev[2 * ray] = (m >= 0) ? s_e0 : 0., elev[2 * ray + 1] = (m >= 0) ? s_e1 : 0.;
                                        index[2 * ray] = m, index[2 * ray + 1] = k;
                                        length[ray] = len, steps[ray] += count;
                                        my_rays++;
                                        ray = -1;
                                } else {
                                        ds = d_step_length(v, s_alt, s_e0, s_e1, m);
                                        d_isotropic((ull)(io.first + ray), (ull)(io.first_step + count), io.seed,
                                            dx, dy, dz);
                                }
                        }
                }
        }
        block_tally(stats, my_rays, my_steps, my_samples, my_plain);
}

/* Batch map projections.  By its subject a kernel of points.hip; it is here for d_project, which
 * is not inlined: a unit's one copy of it is compiled for the widest block among the kernels that
 * call it there, and only this kernel, of 1 024 threads a block at the most, gives the copy that the
 * trace and step kernels call the registers it has always had. */
__global__ void k_project(tamd_proj pr, int inverse, long n, const double * __restrict__ a,
    const double * __restrict__ b, double * __restrict__ c, double * __restrict__ d)
{
        for (long r = blockIdx.x * (long)blockDim.x + threadIdx.x; r < n;
             r += (long)gridDim.x * blockDim.x) {
                double u, w;
                if (inverse)
                        d_unproject(pr, a[r], b[r], u, w);
                else
                        d_project(pr, a[r], b[r], u, w);
                c[r] = u, d[r] = w;
        }
}

__global__ void k_philox(long n, ull seed, ull stream, long first, unsigned * __restrict__ out)
{
        for (long r = blockIdx.x * (long)blockDim.x + threadIdx.x; r < n;
             r += (long)gridDim.x * blockDim.x) {
                const ull id = (ull)(first + r);
                unsigned c[4] = { (unsigned)id, (unsigned)(id >> 32), (unsigned)stream,
                        (unsigned)(stream >> 32) };
                philox4x32_10(c, (unsigned)seed, (unsigned)(seed >> 32));
                for (int i = 0; i < 4; i++) out[4 * r + i] = c[i];
        }
}

__global__ void k_isotropic(long n, ull seed, ull stream, long first, double * __restrict__ dir)
{
        for (long r = blockIdx.x * (long)blockDim.x + threadIdx.x; r < n;
             r += (long)gridDim.x * blockDim.x) {
                double x, y, z;
                d_isotropic((ull)(first + r), stream, seed, x, y, z);
                dir[3 * r] = x, dir[3 * r + 1] = y, dir[3 * r + 2] = z;
        }
}

/* hits[m + 1] and a linear path-length histogram, exact integer counts.
 * Per-block LDS counters (32-bit) flushed with one 64-bit atomic per non-zero bin -- from at most a
 * block a CU (tamd_k_tally), since what such a launch costs is the adds that meet on one word in
 * HBM: a bin that every block holds sees a few hundred of them, not thousands.
 * The hits of a few media (kTallyBallotMedia: every real geometry) never meet in LDS either, where a
 * wave's 64 adds to one or two words would queue: a ballot per medium, and lane j of a wave keeps
 * the wave's count of medium j - 1 in a register until the end.  The histogram is in LDS, in
 * `copies` copies that the block's waves share out among themselves (as many as fit: the launcher). */
constexpr int kTallyThreads = 1024;
constexpr int kTallyBallotMedia = 7;

__global__ void __launch_bounds__(kTallyThreads) k_tally(long n, const int * __restrict__ index,
    const double * __restrict__ length, int n_media, ull * __restrict__ hits,
    int n_bins, double scale, ull * __restrict__ histogram, int copies)
{
        extern __shared__ unsigned int lds[];
        unsigned int * h_hits = lds;                 /* n_media + 1 */
        unsigned int * h_bins = lds + (n_media + 1); /* copies x (n_bins + 1) */
        const int total = n_media + 1 + copies * (n_bins + 1);
        for (int i = threadIdx.x; i < total; i += blockDim.x) lds[i] = 0;
        __syncthreads();
        const int lane = threadIdx.x & 63;
        unsigned int * my_bins = h_bins + (size_t)((threadIdx.x >> 6) % copies) * (n_bins + 1);
        const bool by_ballot = (n_media <= kTallyBallotMedia);
        unsigned int my_hits = 0; /* lane j: this wave's rays in medium j - 1 */
        /* (a wave at a time: its lanes stay together for the ballots) */
        for (long first = blockIdx.x * (long)blockDim.x + (threadIdx.x - lane); first < n;
             first += (long)gridDim.x * blockDim.x) {
                const long r = first + lane;
                const bool live = (r < n);
                int m = -2; /* (counted nowhere) */
                if (live) {
                        m = index[2 * r];
                        const double t = length[r] * scale;
                        int b = n_bins; /* overflow, also NaN and negatives */
                        if ((t >= 0.) && (t < (double)n_bins)) b = (int)t;
                        atomicAdd(&my_bins[b], 1u);
                }
                if (by_ballot) {
                        for (int j = 0; j <= n_media; j++) {
                                const unsigned int c = (unsigned int)__popcll(__ballot(m + 1 == j));
                                if (lane == j) my_hits += c;
                        }
                } else if ((m >= -1) && (m < n_media))
                        atomicAdd(&h_hits[m + 1], 1u);
        }
        if (by_ballot && (lane <= n_media) && (my_hits != 0)) atomicAdd(&h_hits[lane], my_hits);
        __syncthreads();
        for (int i = threadIdx.x; i < n_media + 1 + n_bins + 1; i += blockDim.x) {
                if (i <= n_media) {
                        if (h_hits[i] != 0) atomicAdd(&hits[i], (ull)h_hits[i]);
                        continue;
                }
                const int b = i - (n_media + 1);
                unsigned int c = 0;
                for (int k = 0; k < copies; k++) c += h_bins[(size_t)k * (n_bins + 1) + b];
                if (c != 0) atomicAdd(&histogram[b], (ull)c);
        }
}

/* ---- the ordered hand-over ---------------------------------------------------
 * The front [0, F) of a trace's hand-over list in the order of its one-byte keys (where phase A
 * parks: the shallowest rays first), the back [n - K, n) as it is: a counting sort in two flat
 * kernels, between the two passes (hand_over_sort).  F and K are read from the passes' counters on
 * the device; the places between the two ends are holes, known by their position, and nothing
 * reads them or their keys.  Both kernels give block b the same contiguous chunk of the front.
 * k_order_count adds up how many of each key there are (an LDS histogram a block, then one add per
 * non-zero bin to the 256 `counts`); k_order_place scans those for where each key's ids begin,
 * counts its chunk again, reserves its share of each bin with one returning add on the bin's cursor
 * and places its ids there.  Rays with EQUAL keys come out in whatever order the adds fell: the
 * list itself is filled by atomics, in no fixed order, and no result depends on the order the
 * lined pass draws its rays in (test_sorted_hand_over_changes_no_bit).  Nothing waits, spins or
 * polls.  counts and cursors: zeroed by the caller (tamd_k_trace's one fill). */
constexpr int kOrderThreads = 1024;
constexpr int kOrderBlocks = 256;
constexpr int kOrderBins = TAMD_ORDER_BINS;

struct OrderSpan {
        long n_front, n_back; /* F, K: within the list whatever the counters say */
        long lo, hi;          /* this block's chunk of the front */
};
__device__ __forceinline__ OrderSpan order_span(long n, const ull * __restrict__ n_front,
    const ull * __restrict__ n_back)
{
        OrderSpan s;
        s.n_front = min((long)min(*n_front, (ull)n), n);
        s.n_back = (n_back != nullptr) ? (long)min(*n_back, (ull)(n - s.n_front)) : 0;
        /* (a multiple of 16 places: a chunk's keys begin on a word) */
        const long chunk = ((s.n_front + gridDim.x - 1) / gridDim.x + 15) & ~15L;
        s.lo = min(s.n_front, blockIdx.x * chunk);
        s.hi = min(s.n_front, s.lo + chunk);
        return s;
}
/* f(place, key) for every place of [lo, hi), four keys a load (lo is a multiple of 4, as the keys'
 * address) */
template <class F>
__device__ __forceinline__ void order_each(const unsigned char * __restrict__ keys, long lo, long hi, F && f)
{
        for (long i = lo + 4L * threadIdx.x; i < hi; i += 4L * blockDim.x) {
                if (i + 4 <= hi) {
                        const unsigned int four = *(const unsigned int *)(keys + i);
                        for (int k = 0; k < 4; k++) f(i + k, (int)((four >> (8 * k)) & 255u));
                } else
                        for (long j = i; j < hi; j++) f(j, (int)keys[j]);
        }
}

__global__ void __launch_bounds__(kOrderThreads) k_order_count(long n, const unsigned char * __restrict__ keys,
    const ull * __restrict__ n_front, const ull * __restrict__ n_back, unsigned int * __restrict__ counts)
{
        __shared__ unsigned int mine[kOrderBins];
        const OrderSpan s = order_span(n, n_front, n_back);
        if (s.lo >= s.hi) return; /* (block-uniform) */
        if (threadIdx.x < kOrderBins) mine[threadIdx.x] = 0;
        __syncthreads();
        order_each(keys, s.lo, s.hi, [&](long, int key) { atomicAdd(&mine[key], 1u); });
        __syncthreads();
        if ((threadIdx.x < kOrderBins) && (mine[threadIdx.x] != 0)) atomicAdd(&counts[threadIdx.x], mine[threadIdx.x]);
}

__global__ void __launch_bounds__(kOrderThreads) k_order_place(long n, const unsigned char * __restrict__ keys,
    const int * __restrict__ ids, const ull * __restrict__ n_front, const ull * __restrict__ n_back,
    const unsigned int * __restrict__ counts, unsigned int * __restrict__ cursors, int * __restrict__ out)
{
        __shared__ unsigned int mine[kOrderBins]; /* this chunk's ids of each key; then where the next goes */
        __shared__ unsigned int wave_sum[kOrderBins / 64];
        const OrderSpan s = order_span(n, n_front, n_back);
        /* the back, as it is */
        for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < s.n_back; i += (long)gridDim.x * blockDim.x)
                out[n - s.n_back + i] = ids[n - s.n_back + i];
        if (s.lo >= s.hi) return; /* (block-uniform) */
        const int t = threadIdx.x, lane = t & 63;
        if (t < kOrderBins) mine[t] = 0;
        __syncthreads();
        order_each(keys, s.lo, s.hi, [&](long, int key) { atomicAdd(&mine[key], 1u); });
        /* where each key's ids begin: the exclusive scan of the counts, a wave over 64 bins */
        const unsigned int count = (t < kOrderBins) ? counts[t] : 0;
        unsigned int upto = count;
        for (int d = 1; d < 64; d <<= 1) {
                const unsigned int below = __shfl_up(upto, d, 64);
                if (lane >= d) upto += below;
        }
        if ((t < kOrderBins) && (lane == 63)) wave_sum[t >> 6] = upto;
        __syncthreads();
        if (t < kOrderBins) {
                unsigned int begin = upto - count;
                for (int w = 0; w < (t >> 6); w++) begin += wave_sum[w];
                const unsigned int held = mine[t];
                const unsigned int taken = (held != 0) ? atomicAdd(&cursors[t], held) : 0;
                mine[t] = begin + taken;
        }
        __syncthreads();
        order_each(keys, s.lo, s.hi, [&](long place, int key) {
                const unsigned int to = atomicAdd(&mine[key], 1u);
                if ((long)to < s.n_front) out[to] = ids[place];
        });
}

} /* namespace */

/* ======================================================================== */
/*                             the launch layer                             */
/* ======================================================================== */

#ifdef TRACE_POOL_STATS
extern "C" int tamd_dev_pool_stats(unsigned long long * out, int reset)
{
        HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_pool_stats), sizeof(g_pool_stats)));
        if (reset) {
                static unsigned long long zero[32];
                HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_pool_stats), zero, sizeof(zero)));
        }
        return 0;
}
#endif

/* n single steps: the step kernel, then -- with a direction and scratch for
 * the list -- the bisection of the rays that crossed a boundary.  stats /
 * queue: as for a trace (queue[2 * stride] counts the listed rays), or NULL. */
static int run_step(struct tamd_view view, long n, double * pos, const double * dir,
    double * lat, double * lon, double * alt, double * elev, double * step, int * index,
    int flags, CrossList cross, Paging pg, ull * stats, StepWalk walk)
{
        const bool strict = strict_math(view);
        return with_mode(view.mode, [&](auto mode) {
                constexpr int MODE = decltype(mode)::value;
                /* (the fast step of one map / one stack is a kernel of its own: see k_step_fast) */
                const auto kernel = strict          ? k_step<MODE, false> :
                    (MODE == TAMD_MODE_GENERIC) ? k_step<MODE, true> :
                                                  k_step_fast<MODE>;
                if (launch_blocks("k_step", kernel, grid_for(n, 256), 0, view, n, pos, dir, lat, lon, alt, elev,
                        step, index, flags, cross, pg, stats, walk))
                        return 1;
                if (cross.ray == nullptr) return 0;
                /* the listed rays are a few percent of n, and their number is on the
                 * device: a grid for a tenth of n, striding over whatever there is */
                return with_math(strict, [&](auto fast) {
                        return launch_blocks("k_bisect", k_bisect<MODE, decltype(fast)::value>,
                            grid_for(n / 10 + 1, 256), 0, view, pos, dir, lat, lon, alt, elev, step, index, flags,
                            cross, pg, stats, walk);
                });
        });
}

extern "C" int tamd_k_step(struct tamd_view view, long n, double * pos,
    const double * dir, double * lat, double * lon, double * alt, double * elev,
    double * step, int * index, int flags, struct tamd_paging pg)
{
        if (tamd_dev_init()) return 1;
        if (n <= 0) return 0;
        const CrossList none = { nullptr, nullptr, nullptr, nullptr };
        const StepWalk no_walk = { 0, 0, 0, 0, nullptr, nullptr };
        return run_step(view, n, pos, dir, lat, lon, alt, elev, step, index, flags, none, pg,
            nullptr, no_walk);
}

template <int MODE, bool FAST, bool MODEL, bool PAGED, bool CROSS, bool POOL = false>
static int launch_trace_(struct tamd_view view, long n, bool n_on_device, double * pos,
    const double * dir, int max_steps, int * index, double * length, int * n_steps,
    int flags, PhaseIO ph, ull * stats, ull * queue)
{
        /* phase B (n on the device): the rays phase A handed over -- the long ones (a few
         * percent of n) and whatever was in flight when its queue ran dry
         * (up to one ray per lane): as many blocks as fit, or as there can
         * be work for, which is a block a CU at the least */
        const long fill = (n_on_device && (n < 256L * g_cus)) ? 256L * g_cus : n;
        const auto kernel = k_trace<MODE, FAST, MODEL, PAGED, CROSS, POOL>;
        return launch_blocks("k_trace", kernel, persistent_blocks(kernel, fill), 0, view, n, pos, dir, max_steps,
            index, length, n_steps, flags, ph, stats, queue);
}

/* the instance for this call: PAGED where tiles may have to come in, CROSS where
 * there is a list for the crossings (always, for a lined pass) */
template <int MODE, bool FAST, bool MODEL>
static int launch_trace(struct tamd_view view, long n, bool n_on_device, double * pos,
    const double * dir, int max_steps, int * index, double * length, int * n_steps,
    int flags, PhaseIO ph, ull * stats, ull * queue)
{
#define TRACE_ARGS view, n, n_on_device, pos, dir, max_steps, index, length, n_steps, flags, ph, stats, queue
        constexpr bool CAN_PAGE = (MODE != TAMD_MODE_ONE_MAP);
        const bool paged = CAN_PAGE && (ph.pg.faulted != nullptr);
        const bool cross = (ph.cross.ray != nullptr);
        if (MODEL && !cross) {
                snprintf(g_error, sizeof(g_error), "k_trace: a lined pass needs the crossing list");
                return 1;
        }
        if (paged) {
                if (cross) return launch_trace_<MODE, FAST, MODEL, CAN_PAGE, true>(TRACE_ARGS);
                if constexpr (!MODEL) return launch_trace_<MODE, FAST, MODEL, CAN_PAGE, false>(TRACE_ARGS);
        }
        /* the lined pass of one map / one stack with its rays pooled per block (RayPool): an
         * instance of its own, so that the one without is what it was */
        if constexpr (FAST && MODEL && (MODE != TAMD_MODE_GENERIC))
                if (cross && (ph.pool > 0)) return launch_trace_<MODE, FAST, MODEL, false, true, true>(TRACE_ARGS);
        if (cross) return launch_trace_<MODE, FAST, MODEL, false, true>(TRACE_ARGS);
        if constexpr (!MODEL) return launch_trace_<MODE, FAST, MODEL, false, false>(TRACE_ARGS);
        return 1;
#undef TRACE_ARGS
}

/* the arrays the passes of a trace work in: the caller's, or the library's own (order_rays) */
struct TraceRays {
        double * pos;
        const double * dir;
        int * index;
        double * length;
        int * n_steps;
};

/* the crossings the passes listed (their number is on the device: a grid for
 * all of n, striding over whatever there is) */
template <int MODE, bool FAST>
static int launch_cross(struct tamd_view view, long n, const TraceRays & rays, CrossList cross, Paging pg,
    ull * stats, RayOut out = { nullptr, nullptr, nullptr, nullptr, nullptr }, CrossTail front = { nullptr })
{
        constexpr bool CAN_PAGE = (MODE != TAMD_MODE_ONE_MAP);
        const bool paged = CAN_PAGE && (pg.faulted != nullptr);
        const auto kernel = paged ? k_cross<MODE, FAST, CAN_PAGE> : k_cross<MODE, FAST, false>;
        return launch_blocks("k_cross", kernel, persistent_blocks(kernel, n), 0, view, rays.pos, rays.dir, rays.index,
            rays.length, rays.n_steps, cross, pg, stats, out, front, n);
}

/* ---- the launch policy ---------------------------------------------------
 *
 * What a trace's launches are sized and ordered by: each figure with what was measured for it. */

/* A run-time knob: an environment variable holding a number, read once per process;
 * `fallback` where it is unset or empty. */
struct Knob {
        const char * name;
        long fallback;
        bool read = false;
        long value = 0;
        long get()
        {
                if (!read) {
                        const char * env = getenv(name);
                        value = ((env != nullptr) && (*env != 0)) ? atol(env) : fallback;
                        read = true;
                }
                return value;
        }
};

/* Step counts at which a ray moves on to the next phase of a fast trace (0: no
 * further phase), and the rays a wave of phase A may still hold when it hands
 * over after the queue ran dry.  TURTLE_AMD_* override them for experiments. */
/* The lean steps of the lined pass (one map, a regular stack) cost a tenth of a
 * closed form in instructions: with the line from step 32 on instead of 512, C2
 * (1 M rays) goes from 7.2 to 6.0 ms, one map at 10 M rays from 36.1 to 35.4, C3
 * (a stack, 10 M rays) from 42.4 to 39.8 ms -- the last only with the stack's lined
 * kernel at three waves a SIMD (trace_waves(); at two, 47.5).  Layered geometries
 * have no lean loop. */
static int park_threshold(int mode)
{
        static Knob knob = { "TURTLE_AMD_PARK", -1 };
        const int value = (int)knob.get();
        if (value >= 0) return value;
        return (mode == TAMD_MODE_GENERIC) ? 512 : 32;
}
/* Few in a small batch, where the launch waits for single rays in all-but-empty
 * waves (C2, 1 M rays: 8 lanes 6.85 ms, 32 lanes 7.08, 64 lanes 7.4); more in a large
 * one, where phase B is a matter of throughput (C2 at 4 M rays: 20.5 -> 19.6 ms with 32;
 * C3, 10 M: 42.6 -> 41.8).  The loop gives the same bits whenever it engages. */
static int creep_lanes(long n)
{
        static Knob knob = { "TURTLE_AMD_CREEP_LANES", -1 };
        const int value = (int)knob.get();
        if (value >= 0) return value;
        return (n >= 2000000) ? 4 * kCreepLanes : kCreepLanes;
}
static int dense_go(void)
{
        static Knob knob = { "TURTLE_AMD_DENSE_GO", 24 };
        return (int)knob.get();
}
/* What phase A takes for a long ray when it sorts its hand-over (see there; 0: unsorted) */
static int sort_long_if(void)
{
        static Knob knob = { "TURTLE_AMD_SORT_LONG", 120 };
        return (int)knob.get();
}
/* Do the lined pass's waves exchange rays through LDS (RayPool)?  The same bits either way
 * (test_ray_pool_changes_no_bit); what it is worth, measured (round 4, one MI355X, each alone):
 * one map, 12.5 M rays (C4) 27.0 -> 26.0-26.4 ms; one map, 1 M rays (C2) 3.37 -> 3.55-3.72 ms
 * (a batch that small is as long as its longest rays' own chains, and a ray moves slower in a
 * wave that is kept full); a stack, 10 M rays (C3) 25.4 -> 31.7-33.9 ms (the stack's pooled
 * kernel spills 312 bytes a lane at three waves a SIMD); one map at 3 / 4 / 6 M rays: 8.29 ->
 * 8.42, 10.84 -> 11.15, 13.95 -> 13.74 ms.  So: one map, from 6 M rays on.
 * TURTLE_AMD_POOL=0 / 1: never / wherever the kernel exists. */
static int pool_on(int mode, long n)
{
        static Knob knob = { "TURTLE_AMD_POOL", -1 };
        const int value = (int)knob.get();
        if (value >= 0) return value;
        return (mode == TAMD_MODE_ONE_MAP) && (n >= 6000000);
}
/* Is the hand-over ordered between the passes (run_trace)?  A batch of a few million rays is as
 * long as its longest rays' own chains, and drawing those first is worth more than the sort costs
 * (TURTLE_AMD_SORT_KEY: 0 never, 1 always, else up to that many rays). */
static int sort_hand_over(long n)
{
        static Knob knob = { "TURTLE_AMD_SORT_KEY", -1 };
        const long value = knob.get();
        if (value == 0) return 0;
        if (value == 1) return 1;
        return n <= ((value > 1) ? value : 4000000L);
}
/* ... and by which sort: the counting sort of the library's own (k_order_count, k_order_place: two
 * kernels, no fill of the keys, nothing of its own to zero) or hipCUB's radix sort (three kernels on
 * one 8-bit pass, fills of its own, and the keys pre-filled so that the holes sort between the two
 * ends).  The same rays reach the lined pass in the same order of keys either way; ties may differ,
 * and no result depends on them (tests/test_gpu_sort_own.py).  Measured, one MI355X, the time from
 * phase A's end to the lined pass's start, hipCUB's -> the library's own: one map at 1 / 2 / 4 M rays
 * 50.2 -> 22.5, 56.9 -> 28.2, 62.9 -> 38.1 us; a 4 x 4 stack at 1 M rays 53.7 -> 24.1.  So: the
 * library's own for every batch the hand-over is ordered for.
 * TURTLE_AMD_SORT_OWN=0 / 1: hipCUB's / the library's own (unset: the rule). */
static int sort_own(void)
{
        static Knob knob = { "TURTLE_AMD_SORT_OWN", 1 };
        return knob.get() != 0;
}
/* Does a trace take its rays in the order of where they start (k_ray_cells)?  TURTLE_AMD_SPATIAL:
 * 0 never, 1 always, else from that many rays on. */
static int spatial_order(int mode, long n)
{
        static Knob knob = { "TURTLE_AMD_SPATIAL", -1 };
        const long value = knob.get();
        if ((mode == TAMD_MODE_GENERIC) || (value == 0)) return 0;
        if (value == 1) return 1;
        /* (measured, one pass alone, off -> on: one map at 1 / 2 / 4 / 12.5 M rays 3.13 -> 3.20, 5.91 ->
         * 5.95, 11.17 -> 10.92, 26.7 -> 26.3 ms; a 4 x 4 stack at 1 / 10 M rays 4.10 -> 4.10, 25.5 -> 22.8) */
        return n >= ((value > 1) ? value : 3000000L);
}
/* Do the lined pass's own waves locate the crossings that were listed before its queue ran dry
 * (CrossTail; trace_body, "the crossings under the tail")?  The same bits either way
 * (tests/test_gpu_cross_tail.py).  Measured, one MI355X, off -> on, a pass in ms.  One batch at a
 * time: one map at 1 / 2 / 4 / 6 M rays 3.23-3.28 -> 3.11-3.19, 5.90-5.92 -> 5.75-5.79, 11.09-11.18 ->
 * 10.89-11.41, 13.69-13.78 -> 13.39-13.67; a 4 x 4 stack at 1 / 3 M rays 4.20-4.33 -> 4.21-4.22, 10.98-11.14
 * -> 10.85; but C3 (10 M, a stack) 22.6 -> 25.7 and C4 (12.5 M, one map, pooled kernel with the
 * code in) 25.9 -> 26.4: k_cross all but vanishes (2.7 -> 0.04 ms, 2.9 -> 0.05) and the lined pass
 * grows by more (14.9 -> 21.7, 16.5 -> 20.2 ms) -- the long rays' chains slow down beside locating
 * waves on their SIMD, a priority level below them or not, for as long as the list lasts, and a
 * large batch's list lasts for milliseconds.  Three batches in flight: the tail is not idle then
 * (the next batch's bulk fills it) and the locating only competes: 1 / 2 / 4 M rays 2.19-2.21 ->
 * 2.26-2.27, 3.95 -> 4.38-4.41, 8.03-8.10 -> 9.41-9.69.  So: one batch at a time, up to 3 M rays.
 * TURTLE_AMD_CROSS_TAIL=0 / 1: never (one list, all of it left to k_cross) / wherever the kernel
 * has the code. */
static int cross_tail_on(long n)
{
        static Knob knob = { "TURTLE_AMD_CROSS_TAIL", -1 };
        const long value = knob.get();
        if (value >= 0) return value != 0;
        return (g_ctx.in_flight <= 1) && (n <= 3000000L);
}
/* phase A hands over when its queue is dry and a wave is down to this many rays (PhaseIO.drain_lanes;
 * 0: never, as in the passes that have nobody to hand over to): 64, so any wave does */
constexpr int kDrainLanes = 64;
/* Does the flat kernel (k_first) take the closed-form pass of a fast trace over one map or one
 * stack?  Where that pass is `park` uniform steps and a hand-over: the first round (a later round
 * of a paged trace takes rays at any step count), nothing paged (a ray may have to leave for a
 * tile at any sample), a hand-over within the kernel's bounded loop, and -- the caller's part -- lists
 * to hand over on and a step cap beyond the hand-over.  Everything else is k_trace's, as before.
 * The same bits either way (tests/test_gpu_first_pass.py).
 * TURTLE_AMD_FIRST_PASS=0 / 1: never / wherever the rule allows (unset: the rule). */
static bool first_pass_flat(int park, bool again, const Paging & pg)
{
        static Knob knob = { "TURTLE_AMD_FIRST_PASS", -1 };
        if (knob.get() == 0) return false;
        return !again && (pg.faulted == nullptr) && (park > 0) && (park <= 64);
}
/* The waves a SIMD holds of it: three, while the rays come as the caller has them -- the gathers
 * of a wave then go all over the terrain, and more waves only take each other's lines out of the
 * caches (measured, one map, kernel time in us at 5 -- what the registers allow -- / 4 / 3 / 2 waves:
 * 1 M rays 475 / 447 / 420 / 488; 0.5 M 244 / 237 / 227; 1.5 M 696 / 648 / 623; 2 M 919 / 847 / 822;
 * 0.25 M 126 / 127 / 131; a 4 x 4 stack, 1 M rays, at 4 -- what fits there -- / 3 / 2: 795 / 700 / 656, the
 * persistent kernel 792); as many as fit once the rays are in the order of where they start
 * (spatial_order(); 3 M rays 1104 / 1117 / 1190; 12.5 M 4634 / 4735 / 5004; a stack, 10 M: 4329 at
 * 4, 4514 at 3, 5298 at 2).  TURTLE_AMD_FIRST_WAVES=3 / 8: three / as many as fit, always. */
static int first_pass_waves(bool ordered)
{
        static Knob knob = { "TURTLE_AMD_FIRST_WAVES", -1 };
        if (knob.get() > 0) return (knob.get() <= 3) ? 3 : 8;
        return ordered ? 8 : 3;
}
/* Its grid: a block for every 256 rays (C2: 474 us; as the other flat kernels' grid -- grid_for: eight
 * blocks a CU at the most, each taking chunks of 256 rays in turn, TURTLE_AMD_FIRST_GRID=0 -- 485 us; as
 * 2 / 3 / 4 / 5 / 6 blocks a CU taking chunks in turn 519 / 446 / 482 / 494 / 515: what counts there is
 * the waves a SIMD holds, see above). */
template <int MODE>
static int launch_first(struct tamd_view view, long n, double * pos, const double * dir, int max_steps,
    int * index, double * length, int * n_steps, int flags, const FirstPass & fp, const RayOut & out, ull * stats)
{
        static Knob grid = { "TURTLE_AMD_FIRST_GRID", 1 };
        if (tamd_dev_init()) return 1;
        const unsigned blocks = (grid.get() == 0) ? (unsigned)grid_for(n, 256) : (unsigned)((n + 255) / 256);
        return with_constant<3, 8>(first_pass_waves(out.order_of != nullptr), [&](auto waves) {
                return launch_blocks("k_first", k_first<MODE, decltype(waves)::value>, blocks, 0, view, n, pos, dir,
                    max_steps, index, length, n_steps, flags, fp, out, stats);
        });
}

/* ---- a trace's passes ------------------------------------------------------
 *
 * Where their lists and arrays are: trace_room.h; their counters: internal.h (enum
 * tamd_trace_counter). */

static ull * counter_of(ull * queue, enum tamd_trace_counter c) { return queue + (int)c * kQ; }
/* (the lined pass is given B's queue and finds the tail's words from there: CrossTail) */
static_assert(((int)TAMD_TRACE_TAIL_N_DRY - (int)TAMD_TRACE_QUEUE_B) * kQ == kQTail,
    "CrossTail.n_dry is kQTail words behind the lined pass's queue");
static_assert(((int)TAMD_TRACE_TAIL_L1_NEXT == (int)TAMD_TRACE_TAIL_N_DRY + 1) &&
        ((int)TAMD_TRACE_TAIL_L2_COUNT == (int)TAMD_TRACE_TAIL_N_DRY + 2),
    "CrossTail.l1_next and .l2_count follow n_dry, kQ words apart");

/* A radix sort (hipCUB) of n (key, ray id) pairs in a trace's scratch: the ids in the hand-over
 * list's place and the keys beside them, each with its second buffer.  fits() asks what the sort
 * needs and says whether that is within its room; run() sorts, and Current() of both is the result. */
template <class KEY>
struct RoomSort {
        static_assert(sizeof(KEY) <= sizeof(int), "a key buffer holds an int a ray (trace_room.h)");
        hipcub::DoubleBuffer<KEY> keys;
        hipcub::DoubleBuffer<int> ids;
        void * temp;
        size_t temp_bytes;
        int n, bits;
        RoomSort(char * room, const tamd_trace_room & at, long n_, int bits_)
            : keys(TAMD_ROOM_AT(KEY, room, at.keys), TAMD_ROOM_AT(KEY, room, at.keys_alt)),
              ids(TAMD_ROOM_AT(int, room, at.parked), TAMD_ROOM_AT(int, room, at.ids_alt)),
              temp(room + at.sort_temp), temp_bytes(0), n((int)n_), bits(bits_)
        {
        }
        bool fits()
        {
                return (hipcub::DeviceRadixSort::SortPairs(nullptr, temp_bytes, keys, ids, n, 0, bits, g_stream) ==
                           hipSuccess) &&
                    (temp_bytes <= TAMD_TRACE_SORT_TEMP);
        }
        int run()
        {
                if (hipcub::DeviceRadixSort::SortPairs(temp, temp_bytes, keys, ids, n, 0, bits, g_stream) != hipSuccess)
                        return fail("hipcub::DeviceRadixSort", hipGetLastError());
                return 0;
        }
};

/* The rays in the order of where they start (k_ray_cells): keys and numbers into the sort's
 * room, one pass of the radix sort.  The passes then WORK in that order -- a ray's state
 * between the passes (position, medium, path length, step count, its direction) lives at its
 * place in the ordered list, in arrays of the library's own -- while the caller's arrays are
 * touched twice a ray: phase A reads a new ray from its place there, and whichever kernel
 * ENDS a ray (k_cross for nearly all) writes its results to that place (RayOut); no pass of
 * its own copies anything.  (Tried first: the passes working in the caller's arrays through
 * the ordered list -- every hand-over then goes to a place of its own instead of next to
 * its wave's: half the gain on C3, a loss on C4; and copies made by kernels of their own:
 * 0.9 + 1.4 ms for C4's 12.5 M rays, more than the order gains there.)  Not over paged tiles
 * (the pager's lists name rays by their place in the CALLER's arrays, round after round).
 * Leaves everything as it is where the sort does not fit its room. */
template <int MODE>
static int order_rays(struct tamd_view view, long n, char * room, const tamd_trace_room & at, TraceRays & rays,
    PhaseIO & a, PhaseIO & b, RayOut & out)
{
        RoomSort<SPATIAL_KEY_T> sort(room, at, n, SPATIAL_BITS);
        if (!sort.fits()) return 0;
        hipLaunchKernelGGL(k_ray_cells<MODE>, dim3(grid_for(n, 256)), dim3(256), 0, g_stream, view, n, rays.pos,
            sort.keys.Current(), sort.ids.Current());
        LAUNCH_CHECK("k_ray_cells");
        if (sort.run()) return 1;
        /* the list must outlive the passes, which use its place and the sort's room again */
        int * const kept = TAMD_ROOM_AT(int, room, at.order);
        HIP_TRY(hipMemcpyAsync(kept, sort.ids.Current(), (size_t)n * sizeof(int), hipMemcpyDeviceToDevice, g_stream));
        out.order_of = kept, out.pos = rays.pos, out.index = rays.index, out.length = rays.length;
        out.n_steps = rays.n_steps;
        a.out = out, b.out = out;
        a.pos_in = rays.pos, a.dir_in = rays.dir, a.index_in = rays.index;
        a.dir_copy = TAMD_ROOM_AT(double, room, at.dir_s);
        rays.pos = TAMD_ROOM_AT(double, room, at.pos_s), rays.dir = a.dir_copy;
        rays.index = TAMD_ROOM_AT(int, room, at.index_s), rays.length = TAMD_ROOM_AT(double, room, at.length_s);
        rays.n_steps = TAMD_ROOM_AT(int, room, at.n_steps_s);
        return 0;
}

/* The hand-over of a first round (a later round of a paged trace takes rays at any step count:
 * one end, unsorted).  The list is filled from both ends (sort_long_if(); PhaseIO).  And its front
 * may be ORDERED between the two passes, by one-byte keys beside the list (0 .. 253; the back's are
 * 255): by the library's counting sort of the front (k_order_count; sort_own()), which leaves the
 * back where the lined pass looks for it -- or by a radix sort of the whole list's n places, where
 * the places nobody filled carry a key (254) between the front's and the back's, so the front comes
 * out first, in order, and the back stays at the far end.  For batches small enough to be as long
 * as their longest rays (sort_hand_over()).  Planned before phase A, which writes the keys ... */
static int hand_over_plan(RoomSort<unsigned char> & sort, long n, bool again, ull * queue, double * ds_mark,
    PhaseIO & a, PhaseIO & b, bool & sorting)
{
        const int long_if = sort_long_if();
        sorting = false;
        if (again || (long_if <= 0)) return 0;
        a.n_parked_back = counter_of(queue, TAMD_TRACE_N_PARKED_BACK);
        a.ds_mark = ds_mark, a.mark_at = a.park_after / 2, a.long_if = (float)long_if;
        b.n_dev_back = a.n_parked_back;
        sorting = sort_hand_over(n) && (sort_own() || sort.fits());
        if (!sorting) return 0;
        a.sort_key = sort.keys.Current();
        if (!sort_own()) HIP_TRY(hipMemsetAsync(a.sort_key, 0xFE, (size_t)n, g_stream));
        return 0;
}
/* The two kernels of the counting sort: ids and keys as phase A left them, n_front and n_back its
 * counters, `words` the 2 x 256 zeroed words of the ordering (internal.h).  At most a block a CU's
 * worth (256), each with 4096 places or more of the front -- if the front were the whole list. */
static int launch_order(long n, const int * ids, const unsigned char * keys, const ull * n_front, const ull * n_back,
    unsigned int * words, int * out)
{
        const long wanted = (n + 4 * kOrderThreads - 1) / (4 * kOrderThreads);
        const unsigned blocks = (unsigned)((wanted < 1) ? 1 : (wanted > kOrderBlocks) ? kOrderBlocks : wanted);
        hipLaunchKernelGGL(k_order_count, dim3(blocks), dim3(kOrderThreads), 0, g_stream, n, keys, n_front, n_back,
            words);
        LAUNCH_CHECK("k_order_count");
        hipLaunchKernelGGL(k_order_place, dim3(blocks), dim3(kOrderThreads), 0, g_stream, n, keys, ids, n_front,
            n_back, words, words + kOrderBins, out);
        LAUNCH_CHECK("k_order_place");
        return 0;
}
/* ... and run behind it: the lined pass reads the ordered list */
static int hand_over_sort(RoomSort<unsigned char> & sort, long n, const PhaseIO & a, ull * queue, PhaseIO & b)
{
        if (sort_own()) {
                if (launch_order(n, sort.ids.Current(), sort.keys.Current(), a.n_parked, a.n_parked_back,
                        (unsigned int *)(queue + TAMD_TRACE_COUNTERS), sort.ids.Alternate()))
                        return 1;
                b.ids = sort.ids.Alternate();
                return 0;
        }
        if (sort.run()) return 1;
        b.ids = sort.ids.Current();
        return 0;
}

/* the pass that takes the rays as the call has them, in the arrays of the moment */
template <int MODE, int FAST>
static int launch_plain(struct tamd_view view, long n, bool again, const TraceRays & rays, int max_steps, int flags,
    const PhaseIO & ph, ull * stats, ull * queue)
{
        return launch_trace<MODE, FAST != 0, false>(view, n, again, rays.pos, rays.dir, max_steps, rays.index,
            rays.length, rays.n_steps, flags, ph, stats, counter_of(queue, TAMD_TRACE_QUEUE_A));
}

/* Phase A: the flat kernel where its rule holds (first_pass_flat: the closed-form pass of a fast,
 * listed, uncapped first round), else the persistent one */
template <int MODE>
static int launch_phase_a(struct tamd_view view, long n, bool again, const TraceRays & rays, int max_steps, int flags,
    const PhaseIO & a, const RayOut & out, ull * stats, ull * queue)
{
        if constexpr (MODE != TAMD_MODE_GENERIC) {
                if (first_pass_flat(a.park_after, again, a.pg)) {
                        const FirstPass fp = { a.park_after, a.mark_at, a.long_if, a.parked, a.n_parked,
                                a.n_parked_back, a.sort_key, a.cross, a.pos_in, a.dir_in, a.index_in, a.dir_copy };
                        return launch_first<MODE>(view, n, rays.pos, rays.dir, max_steps, rays.index, rays.length,
                            rays.n_steps, flags, fp, out, stats);
                }
        }
        return launch_plain<MODE, Fast::value>(view, n, again, rays, max_steps, flags, a, stats, queue);
}

/* Phase B: the rays on the hand-over list, each on its line; with `tail`, its idle waves locate
 * the crossings of L1 (CrossTail) */
template <int MODE>
static int launch_lined(struct tamd_view view, long n, const TraceRays & rays, int max_steps, int flags,
    const PhaseIO & b, const CrossTail & tail, ull * stats, ull * queue)
{
        const int tail_flag = (tail.words != nullptr) ? TRACE_CROSS_TAIL : 0;
        return launch_trace<MODE, true, true>(view, n, true, rays.pos, rays.dir, max_steps, rays.index, rays.length,
            rays.n_steps, flags | TRACE_CARRY_MEDIUM | tail_flag, b, stats, counter_of(queue, TAMD_TRACE_QUEUE_B));
}

/* One round of a trace: all the rays (pg.ids == NULL), or the ones the last
 * round listed because they needed a tile (they carry on from the arrays).
 *
 * The passes step; a ray whose step crossed a boundary goes on a list (CROSS, see
 * trace_body) and k_cross locates the crossings at the end, packed.
 * Fast arithmetic steps in two passes: A takes every ray by the closed form up to
 * park_threshold() steps (32, or 512: see there) and hands over what is left; B
 * takes those to their crossing on their lines.  A ray changes pass at a fixed
 * step count, or (below it, when A's queue ran dry) where its arithmetic does not
 * depend on the pass: see LINED.  (A third pass for the rays beyond a second
 * threshold, a few to a wave on an otherwise empty chip, was wired in until round
 * 3 and always off: on C2 every threshold from 256 to 2 048 made the trace slower,
 * 6.9-7.8 ms against 6.0 ms.)
 * Without scratch for the lists (`room` NULL: a batch beyond 2^31 rays, media that do not
 * pack) there is one pass, which bisects in place. */
template <int MODE>
static int run_trace(struct tamd_view view, long n, TraceRays rays, int max_steps, int flags, char * room,
    Paging pg, ull * stats, ull * queue)
{
        const bool again = (pg.ids != nullptr);
        if (again) flags |= TRACE_CARRY_MEDIUM;
        const bool strict = strict_math(view);
        const bool listed = (room != nullptr) && (rays.length != nullptr) && (rays.n_steps != nullptr);
        tamd_trace_room at;
        tamd_trace_room_layout(&at, n);
        CrossList cross = { nullptr, nullptr, nullptr, nullptr };
        if (listed) {
                cross.ray = TAMD_ROOM_AT(int, room, at.cross_ray), cross.ds = TAMD_ROOM_AT(double, room, at.cross_ds);
                cross.count = counter_of(queue, TAMD_TRACE_N_CROSS);
                cross.other = TAMD_ROOM_AT(int, room, at.cross_other);
        }
        PhaseIO shared = {}; /* (by every pass of the round) */
        shared.pg = pg, shared.chunk = kChunk, shared.creep_lanes = creep_lanes(n), shared.dense_go = dense_go();
        shared.cross = cross;
        /* the only pass, where there is one: the rays as the call has them, to their end */
        PhaseIO one = shared;
        one.ids = pg.ids, one.n_dev = pg.n_in, one.accumulate = again ? 2 : 0;
        if (!listed)
                return with_math(strict, [&](auto fast) {
                        return launch_plain<MODE, decltype(fast)::value>(view, n, again, rays, max_steps, flags, one,
                            stats, queue);
                });
        if (strict) {
                if (launch_plain<MODE, Strict::value>(view, n, again, rays, max_steps, flags, one, stats, queue)) return 1;
                return launch_cross<MODE, false>(view, n, rays, cross, pg, stats);
        }
        const int park = park_threshold(MODE);
        if ((park <= 0) || (max_steps <= park)) {
                if (launch_plain<MODE, Fast::value>(view, n, again, rays, max_steps, flags, one, stats, queue)) return 1;
                return launch_cross<MODE, true>(view, n, rays, cross, pg, stats);
        }
        /* A: as `one`, up to `park` steps, then onto the hand-over list; B: from that list, lined */
        PhaseIO a = one, b = shared;
        a.parked = TAMD_ROOM_AT(int, room, at.parked), a.n_parked = counter_of(queue, TAMD_TRACE_N_PARKED);
        a.park_after = park, a.drain_lanes = kDrainLanes;
        b.ids = a.parked, b.n_dev = a.n_parked, b.accumulate = 1, b.line_after = park;
        b.pool = pool_on(MODE, n);
        /* (the lined pass's instances that have the code: fast, one map or one stack, nothing paged) */
        CrossTail tail = { nullptr };
        if ((MODE != TAMD_MODE_GENERIC) && (pg.faulted == nullptr) && cross_tail_on(n))
                tail.words = counter_of(queue, TAMD_TRACE_TAIL_N_DRY);
        RayOut out = { nullptr, nullptr, nullptr, nullptr, nullptr };
        if constexpr (MODE != TAMD_MODE_GENERIC) {
                if (!again && (pg.faulted == nullptr) && spatial_order(MODE, n))
                        if (order_rays<MODE>(view, n, room, at, rays, a, b, out)) return 1;
        }
        RoomSort<unsigned char> hand_over(room, at, n, 8);
        bool sorting = false;
        if (hand_over_plan(hand_over, n, again, queue, TAMD_ROOM_AT(double, room, at.ds_mark), a, b, sorting)) return 1;
        if (launch_phase_a<MODE>(view, n, again, rays, max_steps, flags, a, out, stats, queue)) return 1;
        if (sorting && hand_over_sort(hand_over, n, a, queue, b)) return 1;
        if (launch_lined<MODE>(view, n, rays, max_steps, flags, b, tail, stats, queue)) return 1;
        return launch_cross<MODE, true>(view, n, rays, cross, pg, stats, out, tail);
}

/* room: the stepper's scratch laid out for n rays (trace_room.h), or NULL.  pg: the round of a
 * paged geometry (paging.c), all NULL otherwise; the counters in `stats` add up over the rounds
 * of a call. */
extern "C" int tamd_k_trace(struct tamd_view view, long n, double * pos,
    const double * dir, int max_steps, int * index, double * length, int * n_steps,
    int flags, void * room, struct tamd_paging pg, unsigned long long * stats,
    unsigned long long * queue)
{
        if (tamd_dev_init()) return 1;
        if ((pos == nullptr) || (dir == nullptr) || (index == nullptr) || (stats == nullptr) ||
            (queue == nullptr) ||
            ((pg.faulted != nullptr) &&
                ((pg.tentative == nullptr) || (length == nullptr) || (n_steps == nullptr) ||
                    (pg.n_faulted == nullptr) || (pg.wanted == nullptr) || (pg.wanted_first == nullptr)))) {
                /* (a kernel that writes through a null pointer can take the node down) */
                snprintf(g_error, sizeof(g_error), "tamd_k_trace: a required array is missing");
                return 1;
        }
        if (zero_words(stats, (pg.ids == nullptr) ? 4 : 0, queue, TAMD_TRACE_QUEUE_WORDS)) return 1;
        if (n <= 0) return 0;
        const int carry = (flags & TURTLE_AMD_TRACE_RESUME) ? TRACE_CARRY_MEDIUM : 0;
        const TraceRays rays = { pos, dir, index, length, n_steps };
        return with_mode(view.mode, [&](auto mode) {
                return run_trace<decltype(mode)::value>(view, n, rays, max_steps, carry, (char *)room, pg, stats, queue);
        });
}

/* n single steps with a direction, in two passes (see k_step); cross_ray /
 * cross_ds: scratch for n entries, or NULL to bisect in place */
extern "C" int tamd_k_step_dir(struct tamd_view view, long n, double * pos,
    const double * dir, double * lat, double * lon, double * alt, double * elev,
    double * step, int * index, int flags, int * cross_ray, double * cross_ds,
    struct tamd_paging pg, unsigned long long * stats, unsigned long long * queue)
{
        if (tamd_dev_init()) return 1;
        if (zero_words(stats, (pg.ids == nullptr) ? 4 : 0, queue, 3)) return 1;
        if (n <= 0) return 0;
        const CrossList cross = { cross_ray, (cross_ray != nullptr) ? cross_ds : nullptr, queue + 2, nullptr };
        const StepWalk no_walk = { 0, 0, 0, 0, nullptr, nullptr };
        return run_step(view, n, pos, dir, lat, lon, alt, elev, step, index, flags, cross, pg,
            stats, no_walk);
}

/* One generation of a scattering walk: as tamd_k_step_dir with
 * TURTLE_AMD_STEP_RESUME, the directions drawn in the kernels from Philox(first +
 * ray, stream; seed) and the step added to length[] / steps[] */
extern "C" int tamd_k_step_walk(struct tamd_view view, long n, double * pos, double * alt,
    double * elev, int * index, unsigned long long seed, unsigned long long stream, long first,
    double * length, int * steps, int * cross_ray, double * cross_ds, struct tamd_paging pg,
    unsigned long long * stats, unsigned long long * queue)
{
        if (tamd_dev_init()) return 1;
        /* (stats add up over the generations of a walk: the caller zeroes them) */
        HIP_TRY(hipMemsetAsync(queue, 0, 3 * sizeof(ull), g_stream));
        if (n <= 0) return 0;
        const CrossList cross = { cross_ray, cross_ds, queue + 2, nullptr };
        const StepWalk walk = { 1, seed, stream, first, length, steps };
        return run_step(view, n, pos, nullptr, nullptr, nullptr, alt, elev, nullptr, index,
            TURTLE_AMD_STEP_RESUME, cross, pg, stats, walk);
}

/* A whole walk in one launch (k_walk): every tile resident, nothing listed.
 * stats are NOT zeroed (the caller does); queue[0] is. */
extern "C" int tamd_k_walk(struct tamd_view view, long n, double * pos, double * alt, double * elev,
    int * index, unsigned long long seed, long first, int first_step, int n_steps, double * length,
    int * steps, unsigned long long * stats, unsigned long long * queue)
{
        if (tamd_dev_init()) return 1;
        HIP_TRY(hipMemsetAsync(queue, 0, sizeof(ull), g_stream));
        if (n <= 0) return 0;
        const WalkIO io = { seed, first, first_step, n_steps };
        const bool strict = strict_math(view);
        return with_mode(view.mode, [&](auto mode) {
                return with_math(strict, [&](auto fast) {
                        const auto kernel = k_walk<decltype(mode)::value, decltype(fast)::value>;
                        return launch_blocks("k_walk", kernel, persistent_blocks(kernel, n), 0, view, n, pos, alt,
                            elev, index, length, steps, io, stats, queue);
                });
        });
}

/* One generation of a paged traverse: as tamd_k_step_dir with TURTLE_AMD_STEP_RESUME, the
 * finished rays (index[r][0] = -1) left out; stats add up over the generations */
extern "C" int tamd_k_step_live(struct tamd_view view, long n, double * pos, const double * dir,
    double * alt, double * elev, double * step, int * index, int * cross_ray, double * cross_ds,
    struct tamd_paging pg, unsigned long long * stats, unsigned long long * queue)
{
        if (tamd_dev_init()) return 1;
        HIP_TRY(hipMemsetAsync(queue, 0, 3 * sizeof(ull), g_stream));
        if (n <= 0) return 0;
        const CrossList cross = { cross_ray, (cross_ray != nullptr) ? cross_ds : nullptr, queue + 2, nullptr };
        const StepWalk no_walk = { 0, 0, 0, 0, nullptr, nullptr };
        return run_step(view, n, pos, dir, nullptr, nullptr, alt, elev, step, index,
            TURTLE_AMD_STEP_RESUME | TAMD_STEP_LIVE, cross, pg, stats, no_walk);
}

extern "C" int tamd_k_project(struct tamd_proj proj, int inverse, long n, const double * a,
    const double * b, double * c, double * d)
{
        return launch_items("k_project", k_project, n, 0, proj, inverse, n, a, b, c, d);
}

extern "C" int tamd_k_philox(long n, unsigned long long seed, unsigned long long stream,
    long first, unsigned * out)
{
        return launch_items("k_philox", k_philox, n, 0, n, seed, stream, first, out);
}

extern "C" int tamd_k_isotropic(long n, unsigned long long seed, unsigned long long stream,
    long first, double * dir)
{
        return launch_items("k_isotropic", k_isotropic, n, 0, n, seed, stream, first, dir);
}

extern "C" int tamd_k_tally(long n, const int * index, const double * length,
    int n_media, unsigned long long * hits, int n_bins, double length_max,
    unsigned long long * histogram)
{
        if (tamd_dev_init()) return 1;
        if (n <= 0) return 0;
        const size_t lds = (size_t)(n_media + 1 + n_bins + 1) * sizeof(unsigned int);
        if (lds > 64 * 1024) {
                snprintf(g_error, sizeof(g_error), "too many tally bins (%d)", n_bins);
                return 1;
        }
        const double scale = (double)n_bins / length_max;
        /* a block a CU at the most, a ray a thread at the least; as many copies of the histogram as
         * the block has waves, or as fit beside the hits in the 64 KB a launch may ask for.  (C2's 1 M
         * rays, 2 media, 1 024 bins: 10.0 us; on eight 256-thread blocks a CU, the hits by LDS adds:
         * 47.7 us) */
        static Knob block = { "TURTLE_AMD_TALLY_THREADS", kTallyThreads }; /* (experiments: 256, 512) */
        const int threads = ((block.get() == 256) || (block.get() == 512)) ? (int)block.get() : kTallyThreads;
        const long cus = (g_cus > 0) ? g_cus : 256;
        long blocks = (n + threads - 1) / threads;
        if (blocks > cus) blocks = cus;
        const size_t one = (size_t)(n_bins + 1) * sizeof(unsigned int);
        size_t copies = (64 * 1024 - (size_t)(n_media + 1) * sizeof(unsigned int)) / one;
        if (copies > (size_t)threads / 64) copies = (size_t)threads / 64;
        hipLaunchKernelGGL(k_tally, dim3((unsigned)blocks), dim3(threads),
            (size_t)(n_media + 1) * sizeof(unsigned int) + copies * one, g_stream, n, index, length, n_media, hits,
            n_bins, scale, histogram, (int)copies);
        LAUNCH_CHECK("k_tally");
        return 0;
}

/* the ordering of a hand-over list on its own (run_trace has it between its passes): see
 * k_order_count; words: 2 x 256 x 32 bits, zeroed by the caller */
extern "C" int tamd_k_hand_over_order(long n, const int * ids, const unsigned char * keys,
    const unsigned long long * n_front, const unsigned long long * n_back, unsigned int * words, int * out)
{
        if (tamd_dev_init()) return 1;
        if (n <= 0) return 0;
        if ((ids == nullptr) || (keys == nullptr) || (n_front == nullptr) || (words == nullptr) || (out == nullptr)) {
                snprintf(g_error, sizeof(g_error), "tamd_k_hand_over_order: a required array is missing");
                return 1;
        }
        return launch_order(n, ids, keys, n_front, n_back, words, out);
}
