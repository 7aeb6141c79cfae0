/*
 * internal.h -- declarations shared by the host C objects and the HIP device
 * layer of libturtle_amd.  Not installed.
 *
 * Split of responsibilities:
 *   host (C99: error.c map.c hgt.c stack.c client.c stepper.c ecef.c batch.c)
 *        owns the opaque handles of the public API, file ingest, the error
 *        convention, and flattening a stepper into the POD tables below;
 *   device (runtime.hip: HBM and the stream; device.hip, points.hip, maps.hip,
 *        sight.hip, rays.hip: the kernels, a family each, and their launches).  All arithmetic of the path happens there.
 */
#ifndef TURTLE_AMD_INTERNAL_H
#define TURTLE_AMD_INTERNAL_H

#include <stddef.h>
#include <stdint.h>

#include "turtle_amd.h"
#include "turtle_amd_device.h" /* the POD tables read by the kernels */

#ifdef __cplusplus
extern "C" {
#endif


/* ------------------------------------------------------------------------ */
/* Device layer (runtime.hip, the units of kernels).  Each returns 0 or a    */
/* non-zero value after recording a message readable with tamd_dev_error(). */
/* ------------------------------------------------------------------------ */

/* The device, the stream, the arithmetic mode, the scratch arena and the blocks
 * below belong to the calling THREAD (runtime.hip; device_ctx.h: struct Ctx). */
const char * tamd_dev_error(void);
int tamd_dev_init(void);   /* idempotent; selects the thread's device, makes its stream */
void tamd_dev_release(void); /* frees what the calling thread holds on its device */
int tamd_dev_sync_device(int device); /* every stream of that device */
void tamd_dev_free_on(int device, void * ptr);
/* a grow-only block of the calling thread (0: pager, 1: a stack's own tables) */
int tamd_dev_block(int which, void ** ptr, size_t bytes, int * grown);
#define TAMD_MAX_DEVICES 16
int tamd_dev_count(void);
int tamd_dev_select(int device);
int tamd_dev_current(void);
int tamd_dev_cus(void);
int tamd_dev_stream_set(void * stream);
int tamd_dev_sync(void);
void tamd_dev_math_set(int strict); /* 1: reference-order arithmetic in k_trace */
int tamd_dev_math_get(void);
void tamd_dev_in_flight_set(int batches); /* the batches the thread keeps in flight (a hint: device_launch.h, trace_blocks_per_cu) */
int tamd_dev_in_flight_get(void);

int tamd_dev_malloc(void ** ptr, size_t bytes);
void tamd_dev_free(void * ptr);
int tamd_dev_h2d(void * dst, const void * src, size_t bytes); /* stream-ordered, then synced */
int tamd_dev_d2h(void * dst, const void * src, size_t bytes);
int tamd_dev_zero(void * dst, size_t bytes);                   /* stream-ordered */
/* a pinned host buffer of the calling thread (grow-only), and copies between it and
 * HBM that are queued on the thread's stream and not waited for */
int tamd_dev_pinned(void ** ptr, size_t bytes);
int tamd_dev_copy_async(void * dst, const void * src, size_t bytes, int to_device);
/* page-locked host memory that outlives the call (tile staging) */
int tamd_dev_host_alloc(void ** ptr, size_t bytes);
void tamd_dev_host_free(void * ptr);

/* Grow-only scratch arena for HOST-space calls: reset at the start of each
 * API call, handed out in 256-byte aligned pieces. */
void tamd_scratch_reset(void);
int tamd_scratch_get(void ** ptr, size_t bytes);

/* One round of a batch call over a geometry with paged tiles: which items to
 * run (ids / n_in, NULL for all of 0 .. n-1) and where to list the ones that
 * met a tile that is not resident (faulted / n_faulted) and, over the tile
 * table, how much each tile is wanted.  All NULL: nothing is paged. */
/* The demand counters of the tiles are a line apart: a batch whose rays start over tiles
 * that are not resident adds to a handful of them millions of times in one pass, and in
 * one line those additions queue in ONE channel of the L2 -- behind them, the loads of
 * every other wave that go through that channel. */
#define TAMD_DEMAND_STRIDE 32
struct tamd_paging {
        const int * ids;
        const unsigned long long * n_in;
        int * faulted;
        unsigned long long * n_faulted;
        unsigned * wanted;       /* per entry of the tile table: how many listed items want it
                                  * (entry t at wanted[t * TAMD_DEMAND_STRIDE]: a cache line each) */
        unsigned * wanted_first; /* bitmap: wanted by the first item of the list (served without fail) */
        double * tentative;      /* traces: per ray, the step a waiting ray was about to take */
        int first_id;            /* the item whose wants go to wanted_first (-1: the first listed) */
};

/* Kernel launchers.  All pointers are DEVICE pointers; NULL output pointers
 * are allowed where the public API allows them. */
int tamd_k_ecef_from_geodetic(long n, const double * lat, const double * lon,
    const double * elev, double * ecef);
int tamd_k_ecef_to_geodetic(long n, const double * ecef, double * lat,
    double * lon, double * alt);
int tamd_k_ecef_from_horizontal(long n, const double * lat, const double * lon,
    const double * az, const double * el, double * dir);
int tamd_k_ecef_to_horizontal(long n, const double * lat, const double * lon,
    const double * dir, double * az, double * el);
/* elevation of n points on metas[0] of the view (a MAP or a STACK entry) */
int tamd_k_elevation(struct tamd_view view, long n, const double * a,
    const double * b, double * z, int * inside, struct tamd_paging pg);
/* gradient of n points on metas[0]: MAP (x, y) -> (gx, gy); STACK (lat, lon)
 * -> (glat, glon); ga/gb are in-out */
int tamd_k_gradient(struct tamd_view view, long n, const double * a,
    const double * b, double * ga, double * gb, int * inside, struct tamd_paging pg);
int tamd_k_position(struct tamd_view view, long n, const double * lat,
    const double * lon, const double * height, int layer, double * pos,
    int * data_index, struct tamd_paging pg);
/* the unit normal of the top surface of layer[r] at pos[r] (turtle_stepper_normal_n): rows of
 * `normal` with no data there, or no such layer, are left untouched, their data_index -1 */
int tamd_k_normal(struct tamd_view view, long n, const double * pos, const int * layer,
    double * normal, int * data_index, struct tamd_paging pg);
/* the skyline (turtle_stepper_horizon_n): item r * n_azimuths + a is line a of observer r; over
 * RESIDENT geometry only (a tile that is not in memory answers nothing); items without a sample
 * that has data get sample 0 and keep their elevation and range (NULL: not wanted) */
int tamd_k_horizon(struct tamd_view view, int n_items, int n_azimuths, int n_distances,
    const double * pos, const double * azimuth, const double * distance, int layer, double * elevation,
    int * sample, double * range);
/* the viewshed (turtle_stepper_viewshed_n) over the same lines: every element of visible
 * [n_items][n_distances] is written (1, 0, or -1 for a skipped sample), and of sine, horizon
 * (same shape) and n_visible [n_items] where they are wanted (NULL: not) */
int tamd_k_viewshed(struct tamd_view view, int n_items, int n_azimuths, int n_distances,
    const double * pos, const double * azimuth, const double * distance, int layer, double target_height,
    signed char * visible, double * sine, double * horizon, int * n_visible);
/* the clearance of chords (turtle_stepper_clearance_n): item r * n_targets + t is the line from
 * observer r to target t, or item r the line to target r where `paired`; over RESIDENT geometry
 * only; items without a sample that has data get sample 0 and keep their clearance; n_data
 * [n_items] where it is wanted (NULL: not) */
int tamd_k_clearance(struct tamd_view view, int n_items, int n_targets, int paired, int n_fractions,
    const double * observer, const double * target, const double * fraction, int layer, double * clearance,
    int * sample, int * n_data);
int tamd_k_step(struct tamd_view view, long n, double * pos,
    const double * dir, double * lat, double * lon, double * alt,
    double * elev, double * step, int * index, int flags, struct tamd_paging pg);
/* The counters of a trace's passes, in the `queue` of tamd_k_trace: counter c is the word
 * queue[c * TAMD_TRACE_COUNTER_STRIDE] -- a cache line or two apart, every wave of a pass adds to
 * them.  The lined pass's kernel is given B's queue and finds the tail's three behind it
 * (device.hip, CrossTail): their order and distance from TAMD_TRACE_QUEUE_B are part of it. */
enum tamd_trace_counter {
        TAMD_TRACE_QUEUE_A = 0,     /* the work queue of the first pass (phase A; or the only pass) */
        TAMD_TRACE_QUEUE_B,         /* ... of the lined pass */
        TAMD_TRACE_N_PARKED,        /* the length of the hand-over list (from its front) */
        TAMD_TRACE_N_CROSS,         /* the length of the crossings' list (L1, from its front) */
        TAMD_TRACE_N_PARKED_BACK,   /* the length of the hand-over list's far end */
        TAMD_TRACE_TAIL_N_DRY,      /* CrossTail: the lined pass's waves that know their queue dry */
        TAMD_TRACE_TAIL_L1_NEXT,    /* ... the tickets drawn on the crossings' list */
        TAMD_TRACE_TAIL_L2_COUNT,   /* ... the length of that list's far end (L2) */
        TAMD_TRACE_N_COUNTERS
};
#define TAMD_TRACE_COUNTER_STRIDE 16
#define TAMD_TRACE_COUNTERS (TAMD_TRACE_N_COUNTERS * TAMD_TRACE_COUNTER_STRIDE)
/* Behind the counters, in the same `queue`: the words of the ordered hand-over (k_order_count,
 * k_order_place) -- 256 bin counts, then 256 bin cursors, 32 bits each -- so that one fill zeroes
 * them with the counters. */
#define TAMD_ORDER_BINS 256
#define TAMD_TRACE_ORDER_WORDS (2 * TAMD_ORDER_BINS * 4 / 8) /* in uint64 words */
#define TAMD_TRACE_QUEUE_WORDS (TAMD_TRACE_COUNTERS + TAMD_TRACE_ORDER_WORDS)
/* A stepper's words on the device (host.h: d_stats): the 4 stats of its last batch call, the
 * `queue` of the launchers (a trace's counters and ordering words; the others use its first three
 * words), and the step kernels' own stats of a paged traverse, which keeps its sums in the first 4
 * meanwhile.  stats and queue are contiguous: a launcher that zeroes both does it in one fill. */
#define TAMD_STATS_QUEUE 4
#define TAMD_STATS_ORDER (TAMD_STATS_QUEUE + TAMD_TRACE_COUNTERS)
#define TAMD_STATS_STEPS (TAMD_STATS_QUEUE + TAMD_TRACE_QUEUE_WORDS)
#define TAMD_STATS_WORDS (TAMD_STATS_STEPS + 4)
#if defined(__cplusplus)
static_assert(TAMD_STATS_ORDER + TAMD_TRACE_ORDER_WORDS == TAMD_STATS_STEPS,
    "stats, the trace's counters and the ordering's words are one contiguous run of d_stats");
#else
_Static_assert(TAMD_STATS_ORDER + TAMD_TRACE_ORDER_WORDS == TAMD_STATS_STEPS,
    "stats, the trace's counters and the ordering's words are one contiguous run of d_stats");
#endif
/* stats: 4 x uint64 on the device (rays, steps, samples, capped); queue: TAMD_TRACE_QUEUE_WORDS x
 * uint64 (enum tamd_trace_counter, then the ordering's words); both zeroed by the launcher, in one
 * fill where queue == stats + TAMD_STATS_QUEUE.
 * room: the stepper's scratch block, laid out for THIS n by tamd_trace_room_layout() (trace_room.h: the
 * lists of rays handed from pass to pass, the sorts' room, the ordered copies), or NULL for a
 * single-pass launch that bisects in place; with it, length and n_steps must not be NULL.  (The
 * caller gives NULL too where the lists cannot be used: media that do not pack into 16 bits.)
 * pg.tentative is the caller's to set, from the same layout. */
int tamd_k_trace(struct tamd_view view, long n, double * pos,
    const double * dir, int max_steps, int * index, double * length,
    int * n_steps, int flags, void * room, struct tamd_paging pg,
    unsigned long long * stats, unsigned long long * queue);
/* The ordering of a trace's hand-over list, as tamd_k_trace runs it between its passes: of `ids`
 * (n places) and the one-byte `keys` beside them, the front's *n_front ids into out[0, *n_front) in
 * non-decreasing order of their keys (equal keys in any order) and the back's *n_back ids (NULL:
 * none) into out[n - *n_back, n) as they are; the places between are not written.  words: 2 x
 * TAMD_ORDER_BINS 32-bit words, zeroed by the caller. */
int tamd_k_hand_over_order(long n, const int * ids, const unsigned char * keys,
    const unsigned long long * n_front, const unsigned long long * n_back, unsigned int * words, int * out);
/* a flag of the step kernels beside enum turtle_amd_step_flags: `alt` holds the tentative length
 * of the next step instead of the altitude, `elev` is not used (turtle_stepper_walk_n) */
#define TAMD_STEP_COMPACT 0x200
/* n single steps with a direction: the step kernel lists the rays that crossed
 * a boundary (cross_ray / cross_ds: scratch for n entries each, or NULL to
 * bisect in place) and a second kernel bisects them, packed; `flags` are enum
 * turtle_amd_step_flags */
int tamd_k_step_dir(struct tamd_view view, long n, double * pos,
    const double * dir, double * lat, double * lon, double * alt,
    double * elev, double * step, int * index, int flags, int * cross_ray,
    double * cross_ds, struct tamd_paging pg, unsigned long long * stats,
    unsigned long long * queue);
/* one generation of turtle_stepper_scatter_n: single steps resumed from the
 * sample in alt / elev / index, directions drawn in the kernels from Philox(first
 * + ray, stream; seed), the step added to length[] and steps[]; cross_ray /
 * cross_ds as for tamd_k_step_dir (not NULL); stats are NOT zeroed */
int tamd_k_step_walk(struct tamd_view view, long n, double * pos, double * alt,
    double * elev, int * index, unsigned long long seed, unsigned long long stream, long first,
    double * length, int * steps, int * cross_ray, double * cross_ds, struct tamd_paging pg,
    unsigned long long * stats, unsigned long long * queue);
/* the same walk, all its generations in one launch, the rays' state in registers
 * (every tile resident); stats are NOT zeroed */
int tamd_k_walk(struct tamd_view view, long n, double * pos, double * alt, double * elev,
    int * index, unsigned long long seed, long first, int first_step, int n_steps, double * length,
    int * steps, unsigned long long * stats, unsigned long long * queue);
/* a flag of the step kernels: a ray whose index[r][0] is -1 takes no step and is left as it is (the
 * rays a paged turtle_stepper_traverse_n has finished) */
#define TAMD_STEP_LIVE 0x400
/* where turtle_stepper_crossings_n records crossing c of ray r: element c * n + r of each array
 * (zeroed by the caller), for c < capacity */
struct tamd_crossings {
        double * point;    /* [capacity][n][3] or NULL */
        double * distance; /* [capacity][n] or NULL */
        int * media;       /* [capacity][n][2] or NULL */
        int capacity;
};
/* turtle_stepper_traverse_n, every tile resident: each ray sampled at its origin, then stepped
 * along dir until it leaves the data, reaches `ceiling` or has taken max_steps steps, its path
 * length summed per medium into length[m * n + r] (zeroed by the caller; or NULL); n_steps and
 * n_cross may be NULL.  rec: where to record the crossings (turtle_stepper_crossings_n), or NULL.
 * stats (rays, steps, samples, rays stopped by max_steps) and queue[0] are zeroed by the
 * launcher. */
int tamd_k_traverse(struct tamd_view view, long n, double * pos, const double * dir,
    double ceiling, int max_steps, int * index, double * length, int * n_steps, int * n_cross,
    const struct tamd_crossings * rec, unsigned long long * stats, unsigned long long * queue);
/* turtle_stepper_advance_n, every tile resident: traverse's loop with a depth budget and an
 * optional distance limit a ray (include/turtle_amd.h states it).  distance_max, depth, distance
 * and n_steps may be NULL.  scale_height [media]: turtle_stepper_advance_exp_n's law (the LAW
 * instances of the kernel), or NULL: every medium uniform (the instances without it).  grid (host
 * memory, its density a device pointer): turtle_stepper_advance_grid_n's box of voxels (the GRID
 * instances; not together with scale_height), or NULL.  stats (rays, steps, samples, rays stopped
 * by max_steps) and queue[0] are zeroed by the launcher. */
int tamd_k_advance(struct tamd_view view, long n, double * pos, const double * dir,
    const double * density, const double * scale_height, const struct turtle_amd_grid_view * grid,
    const double * budget, const double * distance_max, double ceiling, int max_steps, int * index, double * depth,
    double * distance, int * n_steps, int * status, unsigned long long * stats,
    unsigned long long * queue);
/* the generation-by-generation form over paged stacks: one step of every ray whose index[r][0]
 * >= 0, resumed from alt / elev / index (tamd_k_step_dir with TURTLE_AMD_STEP_RESUME |
 * TAMD_STEP_LIVE; stats NOT zeroed); then tamd_k_traverse_gen adds what it took to the sums.
 * first != 0: no step was taken yet, the outputs are set from the origin's sample. counters:
 * rays finished, steps, rays stopped by max_steps, rays still live (the caller zeroes [3]). */
int tamd_k_step_live(struct tamd_view view, long n, double * pos, const double * dir,
    double * alt, double * elev, double * step, int * index, int * cross_ray, double * cross_ds,
    struct tamd_paging pg, unsigned long long * stats, unsigned long long * queue);
int tamd_k_traverse_gen(long n, int first, const double * alt, const double * step, int * live_index,
    int * medium, int * index, double * length, int * n_steps, int * n_cross, double ceiling,
    int max_steps, unsigned long long * counters);
/* the crossings of a paged turtle_stepper_crossings_n, launched after each generation's steps and
 * before its tamd_k_traverse_gen: each live ray's step added to its running total (zeroed by the
 * caller), and a ray whose medium changed recorded into slot n_cross[r] */
int tamd_k_crossings_gen(long n, const double * pos, const double * step, const int * live_index,
    const int * medium, const int * n_cross, double * total, struct tamd_crossings rec);
int tamd_k_philox(long n, unsigned long long seed, unsigned long long stream,
    long first, unsigned * out);
int tamd_k_isotropic(long n, unsigned long long seed, unsigned long long stream,
    long first, double * dir);
/* forward (inverse == 0: lat, lon -> x, y) or inverse projection of n points */
int tamd_k_project(struct tamd_proj proj, int inverse, long n, const double * a,
    const double * b, double * c, double * d);
int tamd_k_tally(long n, const int * index, const double * length,
    int n_media, unsigned long long * hits, int n_bins, double length_max,
    unsigned long long * histogram);
/* turtle_map_resample: every block of the target grids[0] (a device table; its nodes are the
 * map's current HBM copy) from metas[0] of the view, a STACK (from_map == 0), or from the map
 * grids[1].  out: a whole new copy of the target in the HBM layout (n_blocks x 64 nodes); z0, dz,
 * is_signed: the target's encoding as turtle_map_fill applies it; flags: enum
 * turtle_amd_resample_flags | TAMD_RESAMPLE_IDENTITY (the source map has the target's
 * projection: it is looked up at the node's own x, y).  counters: 4 x uint64, zeroed by the
 * caller and added to round after round -- nodes outside the data, nodes outside the span and
 * not clamped, nodes clamped.  Over a paged stack the items of `pg` are blocks. */
#define TAMD_RESAMPLE_IDENTITY 0x100
int tamd_k_resample(struct tamd_view view, const struct tamd_grid * grids, int from_map,
    double z0, double dz, int is_signed, int flags, long n_blocks, uint16_t * out,
    struct tamd_paging pg, unsigned long long * counters);
/* the map's host rows (south to north) from an HBM copy */
int tamd_k_unblock(const uint16_t * blocked, int nx, int ny, int nbx, uint16_t * rows);
/* turtle_map_fill_n: the window's elevations (ny rows of nx, `ld` doubles apart) encoded as
 * turtle_map_fill encodes them into ny x nx codes; nothing of the map is written.  counters: 4 x
 * uint64 zeroed by the caller -- elements that fail the call (off the span and not clamped, or
 * NaN), elements clamped, the failed ones with dz <= 0 and z != z0 (not NaN).  flags: enum turtle_amd_fill_flags. */
int tamd_k_fill_encode(const double * elevation, long ld, int nx, int ny, double z0, double dz,
    int is_signed, int flags, uint16_t * codes, unsigned long long * counters);
/* ... and those codes into the window (ix0, iy0, nx, ny) of an HBM copy, in place, a wave a
 * touched block.  blank: the copy holds nothing yet and the window is the whole map. */
int tamd_k_fill_store(uint16_t * nodes, int nbx, int ix0, int iy0, int nx, int ny, int blank,
    const uint16_t * codes);
/* turtle_map_node_n: the window of an HBM copy decoded into ny rows of nx doubles, `ld` apart */
int tamd_k_nodes(const uint16_t * nodes, int nbx, int ix0, int iy0, int nx, int ny, double z0,
    double dz, int is_signed, double * elevation, long ld);

#ifdef __cplusplus
}
#endif
#endif
