/*
 * trace_room.h -- where every byte of a stepper's scratch block lives.
 *
 * One block per stepper (host.h: d_room), laid out for the n rays of the CALL:
 * a block allocated for a larger batch serves a smaller one, because every
 * region's size, and so the total, never decreases as n grows.  Every region
 * begins on a 256-byte boundary of the block.  stepper.c allocates the block
 * and takes the regions of its own from here; run_trace (device.hip) takes the
 * rest.  A new region is one line of the list below.
 *
 * C99 and C++, no HIP.
 */
#ifndef TURTLE_AMD_TRACE_ROOM_H
#define TURTLE_AMD_TRACE_ROOM_H

#include <stddef.h>

/* the temporary storage the two radix sorts of a trace may ask for (they are not run if they
 * ask for more) */
#define TAMD_TRACE_SORT_TEMP ((size_t)32 << 20)

/* X(name, bytes for n rays) -- who writes it; who reads it.  A sort key is at most an int. */
#define TAMD_TRACE_ROOM_REGIONS(X, n) \
        /* the lists, an int a ray */ \
        X(parked, (n) * sizeof(int))      /* the hand-over list, from both ends: phase A; the lined pass. \
                                           * First id buffer of the two sorts */ \
        X(cross_ray, (n) * sizeof(int))   /* the rays whose step crossed a boundary (L1 from the front, L2 \
                                           * from the far end): the passes, the step kernels; k_cross */ \
        X(cross_other, (n) * sizeof(int)) /* ... the medium and data index they found, packed */ \
        X(own_n_steps, (n) * sizeof(int)) /* n_steps of a trace whose caller asks for none (stepper.c) */ \
        X(ids_alt, (n) * sizeof(int))     /* second id buffer of the sorts */ \
        X(keys, (n) * sizeof(int))        /* the sorts' keys: k_ray_cells, phase A; the sorts */ \
        X(keys_alt, (n) * sizeof(int))    /* second key buffer of the sorts */ \
        X(sort_temp, TAMD_TRACE_SORT_TEMP) /* the sorts' temporary storage (hipCUB's own) */ \
        /* the rays in the order the trace takes them (run_trace, the spatial order): the passes */ \
        X(pos_s, (n) * 3 * sizeof(double)) \
        X(dir_s, (n) * 3 * sizeof(double)) \
        X(length_s, (n) * sizeof(double)) \
        X(index_s, (n) * 2 * sizeof(int)) \
        X(n_steps_s, (n) * sizeof(int)) \
        X(order, (n) * sizeof(int))       /* ... and each one's place in the caller's arrays (RayOut) */ \
        /* a double a ray */ \
        X(tentative, (n) * sizeof(double))  /* the step a ray that waits for a tile was about to take: \
                                             * the passes; the next round's (tamd_paging) */ \
        X(cross_ds, (n) * sizeof(double))   /* the crossing steps' lengths, beside cross_ray */ \
        X(own_length, (n) * sizeof(double)) /* length of a trace whose caller asks for none (stepper.c) */ \
        X(ds_mark, (n) * sizeof(double))    /* a ray's step length at step mark_at, which the two-ended \
                                             * hand-over goes by: phase A */

/* byte offsets of the regions from the block's base, and the block's size */
struct tamd_trace_room {
#define TAMD_ROOM_FIELD(name, size) size_t name;
        TAMD_TRACE_ROOM_REGIONS(TAMD_ROOM_FIELD, 0)
#undef TAMD_ROOM_FIELD
        size_t bytes;
};

/* the layout for a batch of n >= 0 rays; returns room->bytes (stepper.c allocates none for 2^31 - 1
 * rays or more: the ids are ints) */
static inline size_t tamd_trace_room_layout(struct tamd_trace_room * room, long n)
{
        const size_t rays = (size_t)n;
        size_t at = 0;
#define TAMD_ROOM_PLACE(name, size) room->name = at, at += (((size_t)(size)) + 255) / 256 * 256;
        TAMD_TRACE_ROOM_REGIONS(TAMD_ROOM_PLACE, rays)
#undef TAMD_ROOM_PLACE
        room->bytes = at;
        return at;
}

/* a region of the block at `base` */
#define TAMD_ROOM_AT(type, base, offset) ((type *)((char *)(base) + (offset)))

#endif
