/*
 * fill.c -- turtle_map_fill_n and turtle_map_node_n: a window of a map's nodes written from,
 * or read into, rows of doubles in one call -- the loops of turtle_map_fill and
 * turtle_map_node over the window.
 *
 * A fill runs in two kernels (maps.hip).  k_fill_encode turns the elevations into codes in
 * a buffer of the call's own and counts the elements that turtle_map_fill would refuse; this
 * file reads the counters and then either raises, with the map exactly as it was, or commits:
 * k_fill_store puts the codes into the map's HBM copy in place, block by touched block, and
 * the same codes come back into the host rows.  Work and traffic follow the window, not the
 * map.  A read is one kernel, k_nodes, over the HBM copy.
 */
#include "host.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

struct fill_call {
        struct turtle_map * map;
        int ix0, iy0, nx, ny;
        int whole;                          /* the window is the whole map */
        uint16_t * d_codes;                 /* [ny][nx], in the arena */
        uint16_t * codes;                   /* their host copy */
};

/* The map's copy on this device, current -- or, when every node is about to be overwritten,
 * merely there (*blank) */
static int fill_sync(struct fill_call * c, struct tamd_grid * grid, int * blank)
{
        *blank = 0;
        return c->whole ? tamd_map_sync_blank(c->map, grid, blank) : tamd_map_sync(c->map, grid);
}

/* The codes become the map's: into this device's copy in place, then into the host rows,
 * under the geometry held exclusively.  Whatever fails after the store was queued leaves the
 * host rows as they were and the copy marked stale: the map is then as it was. */
static int fill_commit(struct fill_call * c)
{
        struct turtle_map * m = c->map;
        const size_t n = (size_t)c->nx * c->ny;
        const int device = tamd_dev_current();
        struct tamd_grid grid;
        int blank, rc = 1;
        tamd_geometry_write_begin();
        /* (a turtle_map_fill of another thread since the first sync: the copy is brought up to date
         * again; launches queued before, on any stream of the device, may still read it) */
        if ((fill_sync(c, &grid, &blank) == 0) && (tamd_dev_sync_device(device) == 0)) {
                if ((tamd_k_fill_store((uint16_t *)grid.nodes, grid.nbx, c->ix0, c->iy0, c->nx, c->ny, blank,
                         c->d_codes) == 0) &&
                    (tamd_dev_sync() == 0) && (tamd_dev_d2h(c->codes, c->d_codes, n * sizeof(*c->codes)) == 0)) {
                        int j;
                        for (j = 0; j < c->ny; j++)
                                memcpy(m->nodes + (size_t)(c->iy0 + j) * m->nx + c->ix0, c->codes + (size_t)j * c->nx,
                                    (size_t)c->nx * sizeof(*c->codes));
                        m->d_fresh = 1u << device; /* the other devices' copies are stale */
                        rc = 0;
                } else {
                        m->d_fresh &= ~(1u << device);
                }
                tamd_geometry_changed();
        }
        tamd_geometry_write_end();
        return rc;
}

static int window_outside(const struct turtle_map * map, int ix0, int iy0, int nx, int ny)
{
        return (ix0 < 0) || (iy0 < 0) || ((long)ix0 + nx > map->nx) || ((long)iy0 + ny > map->ny);
}

static size_t window_span(int nx, int ny, long ld) { return ((size_t)(ny - 1) * (size_t)ld + (size_t)nx) * sizeof(double); }

enum turtle_return turtle_map_fill_n(struct turtle_map * map, int ix0, int iy0, int nx, int ny,
    const double * elevation, long ld, int flags, long * clamped, int space)
{
        TAMD_ERROR_INIT(&turtle_map_fill_n);
        TAMD_VIEW_GUARD();
        if ((map == NULL) || (elevation == NULL))
                return TAMD_RAISE(TURTLE_RETURN_BAD_ADDRESS, "invalid null argument");
        if (flags & ~TURTLE_AMD_FILL_CLAMP)
                return TAMD_RAISE(TURTLE_RETURN_DOMAIN_ERROR, "invalid flags (%d)", flags);
        if ((space != TURTLE_AMD_HOST) && (space != TURTLE_AMD_DEVICE))
                return TAMD_RAISE(TURTLE_RETURN_DOMAIN_ERROR, "invalid space (%d)", space);
        if (map->stack != NULL)
                return TAMD_RAISE(TURTLE_RETURN_DOMAIN_ERROR, "a tile of a stack cannot be resampled");
        if ((nx <= 0) || (ny <= 0)) return TURTLE_RETURN_SUCCESS;
        if (window_outside(map, ix0, iy0, nx, ny))
                return TAMD_RAISE(TURTLE_RETURN_DOMAIN_ERROR, "point is outside of map");
        if (ld < nx)
                return TAMD_RAISE(TURTLE_RETURN_DOMAIN_ERROR, "invalid leading dimension (%ld < %d)", ld, nx);

        struct fill_call c;
        memset(&c, 0, sizeof(c));
        c.map = map, c.ix0 = ix0, c.iy0 = iy0, c.nx = nx, c.ny = ny;
        c.whole = (nx == map->nx) && (ny == map->ny);
        const size_t n = (size_t)nx * ny;

        /* the arena: the caller's rows (HOST space), then 4 counters and the codes */
        struct tamd_stage st = { 0 };
        struct tamd_grid grid;
        unsigned long long counts[4] = { 0, 0, 0, 0 };
        void *dz, *work;
        int blank;
        tamd_stage_add(&st, elevation, window_span(nx, ny, ld), TAMD_IN, &dz);
        tamd_stage_add(&st, NULL, 256 + n * sizeof(*c.codes), TAMD_SCRATCH, &work);
        int rc = -1;
        if ((fill_sync(&c, &grid, &blank) == 0) && (tamd_stage_open(&st, space) == 0)) {
                unsigned long long * d_counters = work;
                c.d_codes = (uint16_t *)((char *)work + 256);
                if ((tamd_dev_zero(d_counters, sizeof(counts)) == 0) &&
                    (tamd_k_fill_encode(dz, ld, nx, ny, map->z0, map->dz, map->is_signed, flags, c.d_codes,
                         d_counters) == 0) &&
                    (tamd_dev_d2h(counts, d_counters, sizeof(counts)) == 0))
                        rc = 0;
        }
        if ((rc == 0) && (counts[0] > 0)) {
                /* [ref map.c:192-200]: nothing changes.  (A NaN is "outside of map span" whatever dz.) */
                return TAMD_RAISE(TURTLE_RETURN_DOMAIN_ERROR, "%s",
                    (counts[2] > 0) ? "inconsistent elevation value" : "elevation is outside of map span");
        }
        if (rc == 0) {
                c.codes = malloc(n * sizeof(*c.codes));
                if (c.codes == NULL) return TAMD_RAISE(TURTLE_RETURN_MEMORY_ERROR, "could not allocate memory");
                if (fill_commit(&c) || tamd_stage_close(&st)) rc = -1;
                free(c.codes);
        }
        if (rc < 0) return TAMD_RAISE_DEVICE();
        if (clamped != NULL) *clamped = (long)counts[1];
        return TURTLE_RETURN_SUCCESS;
}

/* the launch of a read, the geometry held in use from the sync until it is queued */
static int node_n(struct turtle_map * map, int ix0, int iy0, int nx, int ny, double * elevation, long ld,
    int space)
{
        struct tamd_stage st = { 0 };
        struct tamd_grid grid;
        void * dz;
        /* (HOST space, rows with padding: the padding goes in and comes back as it was) */
        tamd_stage_add(&st, elevation, window_span(nx, ny, ld), (ld == nx) ? TAMD_OUT : TAMD_INOUT, &dz);
        tamd_geometry_use_begin();
        const int rc = tamd_map_sync(map, &grid) || tamd_stage_open(&st, space) ||
            tamd_k_nodes((const uint16_t *)grid.nodes, grid.nbx, ix0, iy0, nx, ny, map->z0, map->dz,
                map->is_signed, dz, ld);
        tamd_geometry_use_end();
        return rc || tamd_stage_close(&st);
}

enum turtle_return turtle_map_node_n(const struct turtle_map * map, int ix0, int iy0, int nx, int ny,
    double * elevation, long ld, int space)
{
        TAMD_ERROR_INIT(&turtle_map_node_n);
        if ((map == NULL) || (elevation == NULL))
                return TAMD_RAISE(TURTLE_RETURN_BAD_ADDRESS, "invalid null argument");
        if ((space != TURTLE_AMD_HOST) && (space != TURTLE_AMD_DEVICE))
                return TAMD_RAISE(TURTLE_RETURN_DOMAIN_ERROR, "invalid space (%d)", space);
        if ((nx <= 0) || (ny <= 0)) return TURTLE_RETURN_SUCCESS;
        if (window_outside(map, ix0, iy0, nx, ny))
                return TAMD_RAISE(TURTLE_RETURN_DOMAIN_ERROR, "point is outside of map");
        if (ld < nx)
                return TAMD_RAISE(TURTLE_RETURN_DOMAIN_ERROR, "invalid leading dimension (%ld < %d)", ld, nx);
        if (node_n((struct turtle_map *)map, ix0, iy0, nx, ny, elevation, ld, space)) return TAMD_RAISE_DEVICE();
        return TURTLE_RETURN_SUCCESS;
}
