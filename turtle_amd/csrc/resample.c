/*
 * resample.c -- turtle_map_resample: every node of a map filled from a stack or from
 * another map in one call, the loop of the reference's examples/example-projection.c
 * (turtle_map_node, turtle_projection_unproject, turtle_stack_elevation, turtle_map_fill).
 *
 * The kernel (k_resample, maps.hip) writes a whole new HBM copy of the map.  This file
 * checks the arguments, runs the rounds of a paged stack (paging.c; the items are the
 * map's 8 x 8 blocks), and then commits the copy -- it becomes this device's copy, the
 * host rows are read back from it, the other devices' copies go stale -- or drops it,
 * when a node failed the span check: the map is then exactly as it was.
 */
#include "host.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* "the same projection": the same type and parameters, or both geographic */
static int same_projection(const struct turtle_projection * a, const struct turtle_projection * b)
{
        if ((a->type < 0) || (b->type < 0)) return (a->type < 0) && (b->type < 0);
        if (a->type != b->type) return 0;
        if (a->type == TAMD_PROJ_LAMBERT) return a->lambert_tag == b->lambert_tag;
        return (a->longitude_0 == b->longitude_0) && (a->hemisphere == b->hemisphere);
}

struct resample_call {
        struct turtle_map * map;
        struct turtle_stack * stack;
        struct turtle_map * source;
        int flags;
        long n_blocks;
        struct tamd_grid * d_grids;         /* [0] the map, [1] the source map */
        unsigned long long * d_counters;    /* 4 */
        uint16_t * out;                     /* the new HBM copy */
};

/* the device table of the target (and source) grid, then one launch; inside the use span */
static int resample_launch(struct resample_call * c, struct tamd_view view, struct tamd_paging pg)
{
        struct tamd_grid grids[2];
        memset(grids, 0, sizeof(grids));
        if (tamd_map_sync(c->map, &grids[0])) return 1;
        if ((c->source != NULL) && tamd_map_sync(c->source, &grids[1])) return 1;
        if (tamd_dev_h2d(c->d_grids, grids, sizeof(grids))) return 1;
        const struct turtle_map * m = c->map;
        return tamd_k_resample(view, c->d_grids, c->source != NULL, m->z0, m->dz, m->is_signed,
            c->flags, c->n_blocks, c->out, pg, c->d_counters);
}

/* The kernel over the whole map: one launch from a map, rounds over a stack.  Returns 0,
 * -1 (device) or a positive enum turtle_return with `message` set. */
static int resample_rounds(struct resample_call * c, char * message, size_t size)
{
        struct tamd_view view;
        const struct tamd_paging none = { NULL, NULL, NULL, NULL, NULL, NULL, NULL, -1 };
        if (c->source != NULL) {
                memset(&view, 0, sizeof(view));
                tamd_geometry_use_begin();
                const int rc = resample_launch(c, view, none) ? -1 : 0;
                tamd_geometry_use_end();
                return rc;
        }
        struct turtle_stack * s = c->stack;
        struct tamd_pager pager;
        memset(&pager, 0, sizeof(pager));
        if (tamd_stack_is_paged(s) &&
            tamd_pager_begin(&pager, c->n_blocks, s->latitude_n * s->longitude_n))
                return -1;
        int rc = 0;
        for (;;) {
                struct tamd_paging pg;
                tamd_geometry_use_begin();
                if ((rc = tamd_stack_view(s, &view, message, size)) == 0) {
                        if (tamd_pager_round(&pager, &pg) || resample_launch(c, view, pg)) rc = -1;
                }
                tamd_geometry_use_end();
                if (rc != 0) break;
                unsigned long long faulted = 0;
                if (tamd_pager_collect(&pager, &faulted)) {
                        rc = -1;
                        break;
                }
                if (faulted == 0) break;
                const int got = tamd_stack_page_in(s, pager.wanted, pager.pinned, 0,
                    faulted <= TAMD_PAGING_FEW, message, size);
                if (got < 0) {
                        rc = -got;
                        break;
                }
                if (pager.rounds > TAMD_PAGING_ROUNDS) { /* cannot be: a round serves a block */
                        snprintf(message, size, "stack of %d tiles is too small for this query (%s)",
                            tamd_stack_budget(s), s->root);
                        rc = TURTLE_RETURN_MEMORY_ERROR;
                        break;
                }
        }
        tamd_pager_end(&pager);
        tamd_stack_trim(s);
        return rc;
}

/* The new copy becomes the map's: the host rows first (read back into a buffer of their
 * own), then both swapped in at once, under the geometry held exclusively */
static int resample_commit(struct resample_call * c)
{
        struct turtle_map * m = c->map;
        const size_t n = (size_t)m->nx * m->ny;
        const int device = tamd_dev_current();
        uint16_t * rows = NULL;
        uint16_t * host = malloc(n * sizeof(*host));
        if ((host == NULL) || tamd_dev_malloc((void **)&rows, n * sizeof(*rows)) ||
            tamd_k_unblock(c->out, m->nx, m->ny, (int)((m->nx + TAMD_BLOCK - 1) / TAMD_BLOCK), rows) ||
            tamd_dev_d2h(host, rows, n * sizeof(*rows))) {
                tamd_dev_free(rows);
                free(host);
                return 1;
        }
        tamd_dev_free(rows);
        tamd_geometry_write_begin();
        void * old = m->d_nodes[device];
        uint16_t * old_rows = m->nodes;
        m->d_nodes[device] = c->out;
        m->nodes = host;
        m->d_fresh = 1u << device; /* the other devices' copies are stale */
        /* (launches queued before, on any stream of the device, may still read the old copy) */
        if ((old != NULL) && (tamd_dev_sync_device(device) == 0)) tamd_dev_free(old);
        tamd_geometry_changed();
        tamd_geometry_write_end();
        free(old_rows);
        c->out = NULL;
        return 0;
}

enum turtle_return turtle_map_resample(struct turtle_map * map, struct turtle_stack * stack,
    const struct turtle_map * source, int flags, long * outside, long * clamped)
{
        TAMD_ERROR_INIT(&turtle_map_resample);
        TAMD_VIEW_GUARD();
        if ((map == NULL) || ((stack == NULL) && (source == NULL)))
                return TAMD_RAISE(TURTLE_RETURN_BAD_ADDRESS, "invalid null argument");
        if ((stack != NULL) && (source != NULL))
                return TAMD_RAISE(TURTLE_RETURN_DOMAIN_ERROR, "a stack or a source map, not both");
        if (source == map)
                return TAMD_RAISE(TURTLE_RETURN_DOMAIN_ERROR, "a map cannot be resampled from itself");
        if (map->stack != NULL)
                return TAMD_RAISE(TURTLE_RETURN_DOMAIN_ERROR, "a tile of a stack cannot be resampled");
        if (flags & ~TURTLE_AMD_RESAMPLE_CLAMP)
                return TAMD_RAISE(TURTLE_RETURN_DOMAIN_ERROR, "invalid flags (%d)", flags);

        struct resample_call c;
        memset(&c, 0, sizeof(c));
        c.map = map, c.stack = stack, c.source = (struct turtle_map *)source;
        c.flags = flags;
        if ((source != NULL) && same_projection(&map->projection, &source->projection))
                c.flags |= TAMD_RESAMPLE_IDENTITY;
        const long nbx = (map->nx + TAMD_BLOCK - 1) / TAMD_BLOCK;
        const long nby = (map->ny + TAMD_BLOCK - 1) / TAMD_BLOCK;
        c.n_blocks = nbx * nby;

        char message[4200];
        unsigned long long counts[4] = { 0, 0, 0, 0 };
        void * tables;
        int rc = -1;
        if (tamd_dev_init() == 0) {
                tamd_scratch_reset();
                if ((tamd_scratch_get(&tables, 2 * sizeof(struct tamd_grid) + 4 * sizeof(counts[0])) == 0) &&
                    (tamd_dev_malloc((void **)&c.out, (size_t)c.n_blocks * 64 * sizeof(uint16_t)) == 0)) {
                        c.d_grids = tables;
                        c.d_counters = (unsigned long long *)(c.d_grids + 2);
                        if ((tamd_dev_zero(c.d_counters, sizeof(counts)) == 0) &&
                            ((rc = resample_rounds(&c, message, sizeof(message))) == 0))
                                rc = tamd_dev_d2h(counts, c.d_counters, sizeof(counts)) ? -1 : 0;
                }
        }
        if ((rc == 0) && (counts[1] > 0) && !(flags & TURTLE_AMD_RESAMPLE_CLAMP)) {
                /* [ref map.c:192-200]: nothing changes */
                rc = TURTLE_RETURN_DOMAIN_ERROR;
                snprintf(message, sizeof(message), "%s",
                    (map->dz <= 0.) ? "inconsistent elevation value" : "elevation is outside of map span");
        }
        if ((rc == 0) && resample_commit(&c)) rc = -1;
        tamd_dev_free(c.out);
        if (rc < 0) return TAMD_RAISE_DEVICE();
        if (rc > 0) return TAMD_RAISE((enum turtle_return)rc, "%s", message);
        if (outside != NULL) *outside = (long)counts[0];
        if (clamped != NULL) *clamped = (long)counts[2];
        return TURTLE_RETURN_SUCCESS;
}
