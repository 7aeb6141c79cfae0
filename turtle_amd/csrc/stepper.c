/*
 * stepper.c -- the layered-topography stepper handle [ref src/turtle/
 * stepper.c:379-931, stepper.h:45-110].
 *
 * The reference keeps linked lists of layers -> (data, offset) metas -> data
 * sources and walks them per sample on the CPU.  Here the same description is
 * kept in small host arrays and FLATTENED into POD tables in HBM
 * (internal.h); every sample, step and trace is then computed by the kernels
 * of device.hip, rays.hip and sight.hip.  Scalar entry points are the batch ones with n = 1.
 */
#include "host.h"
#include "trace_room.h"

#include <time.h>

#include <float.h>
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* what the stepper holds in HBM, on the device it was last used on */
#define VIEW_OUT_TEXT "a device view of the stepper is out (turtle_amd_stepper_view_release comes first)"
#define VIEW_OUT_GUARD(stepper)                                                \
        do {                                                                   \
                if ((stepper)->view_out) return TAMD_RAISE(TURTLE_RETURN_DOMAIN_ERROR, VIEW_OUT_TEXT); \
        } while (0)

static void stepper_release_device(struct turtle_stepper * s)
{
        int drained = 1;
        if ((s->d_tables != NULL) || (s->d_stats != NULL) || (s->d_room != NULL))
                drained = (tamd_dev_sync_device(s->device) == 0);
        if (drained) { /* else: leaked, rather than freed under a launch that may still read it */
                tamd_dev_free_on(s->device, s->d_tables);
                tamd_dev_free_on(s->device, s->d_stats);
                tamd_dev_free_on(s->device, s->d_room);
        }
        s->d_tables = NULL, s->d_stats = NULL, s->d_room = NULL;
        s->d_tables_size = 0, s->room_capacity = 0, s->epoch = 0;
}

/* The stepper's HBM (tables, counters, scratch) is on the device of the thread
 * that uses it: what it held elsewhere goes when that thread has moved on.
 * Before anything of it is allocated or used. */
static int stepper_bind_device(struct turtle_stepper * s)
{
        if (tamd_dev_init()) return 1;
        if (s->device != tamd_dev_current()) {
                if (s->device >= 0) stepper_release_device(s);
                s->device = tamd_dev_current();
        }
        return 0;
}

/* ---- construction [ref stepper.c:547-600] -------------------------------- */

enum turtle_return turtle_stepper_create(struct turtle_stepper ** stepper)
{
        TAMD_ERROR_INIT(&turtle_stepper_create);
        struct turtle_stepper * s = calloc(1, sizeof(*s));
        if (s == NULL)
                return TAMD_RAISE(TURTLE_RETURN_MEMORY_ERROR, "could not allocate memory");
        s->device = -1;
        s->local_range = 1.; /* defaults [ref stepper.c:558-560] */
        s->slope_factor = 0.4;
        s->resolution_factor = 1E-02;
        *stepper = s;
        return TURTLE_RETURN_SUCCESS;
}

enum turtle_return turtle_stepper_destroy(struct turtle_stepper ** stepper)
{
        if ((stepper == NULL) || (*stepper == NULL)) return TURTLE_RETURN_SUCCESS;
        struct turtle_stepper * s = *stepper;
        if (s->view_out) {
                TAMD_ERROR_INIT(&turtle_stepper_destroy);
                return TAMD_RAISE(TURTLE_RETURN_DOMAIN_ERROR, VIEW_OUT_TEXT);
        }
        int i;
        for (i = 0; i < s->n_data; i++) /* owned clients [ref stepper.c:578-586] */
                if (s->data[i].client != NULL) turtle_client_destroy(&s->data[i].client);
        for (i = 0; i < s->n_layers; i++) free(s->layers[i].meta);
        stepper_release_device(s);
        free(s->data);
        free(s->layers);
        free(s);
        *stepper = NULL;
        return TURTLE_RETURN_SUCCESS;
}

/* [ref stepper.c:364-388]: an empty top layer is reused */
static int push_layer(struct turtle_stepper * s)
{
        if ((s->n_layers > 0) && (s->layers[s->n_layers - 1].size == 0)) return 0;
        if (s->n_layers == s->cap_layers) {
                const int cap = s->cap_layers ? 2 * s->cap_layers : 4;
                struct tamd_layer * l = realloc(s->layers, cap * sizeof(*l));
                if (l == NULL) return 1;
                s->layers = l, s->cap_layers = cap;
        }
        memset(&s->layers[s->n_layers++], 0, sizeof(*s->layers));
        tamd_geometry_changed();
        return 0;
}

enum turtle_return turtle_stepper_add_layer(struct turtle_stepper * stepper)
{
        TAMD_ERROR_INIT(&turtle_stepper_add_layer);
        VIEW_OUT_GUARD(stepper);
        if (push_layer(stepper))
                return TAMD_RAISE(TURTLE_RETURN_MEMORY_ERROR, "could not allocate memory");
        return TURTLE_RETURN_SUCCESS;
}

static int push_data(struct turtle_stepper * s, const struct tamd_data * d)
{
        if (s->n_data == s->cap_data) {
                const int cap = s->cap_data ? 2 * s->cap_data : 4;
                struct tamd_data * p = realloc(s->data, cap * sizeof(*p));
                if (p == NULL) return -1;
                s->data = p, s->cap_data = cap;
        }
        s->data[s->n_data] = *d;
        return s->n_data++;
}

/* [ref stepper.c:390-409]: the first data creates layer 0; metas append to
 * the top layer */
static int push_meta(struct turtle_stepper * s, int data, double offset)
{
        if ((s->n_layers == 0) && push_layer(s)) return 1;
        struct tamd_layer * l = &s->layers[s->n_layers - 1];
        if (l->size == l->capacity) {
                const int cap = l->capacity ? 2 * l->capacity : 4;
                struct tamd_layer_meta * m = realloc(l->meta, cap * sizeof(*m));
                if (m == NULL) return 1;
                l->meta = m, l->capacity = cap;
        }
        l->meta[l->size].data = data;
        l->meta[l->size].offset = offset;
        l->size++;
        s->last.valid = 0; /* (the host's cached sample: scalar.c) */
        tamd_geometry_changed();
        return 0;
}

/* [ref stepper.c:411-470]: one data per distinct stack; a locked stack gets a
 * client owned by the stepper */
enum turtle_return turtle_stepper_add_stack(
    struct turtle_stepper * stepper, struct turtle_stack * stack, double offset)
{
        TAMD_ERROR_INIT(&turtle_stepper_add_stack);
        VIEW_OUT_GUARD(stepper);
        int i, data = -1;
        for (i = 0; i < stepper->n_data; i++)
                if ((stepper->data[i].kind == TAMD_STACK) && (stepper->data[i].stack == stack))
                        data = i;
        if (data < 0) {
                struct tamd_data d = { TAMD_STACK, NULL, stack, NULL };
                if (stack->lock != NULL) {
                        const enum turtle_return rc = turtle_client_create(&d.client, stack);
                        if (rc != TURTLE_RETURN_SUCCESS) return rc;
                }
                data = push_data(stepper, &d);
                if (data < 0) {
                        turtle_client_destroy(&d.client);
                        return TAMD_RAISE(
                            TURTLE_RETURN_MEMORY_ERROR, "could not allocate memory");
                }
        }
        if (push_meta(stepper, data, offset))
                return TAMD_RAISE(TURTLE_RETURN_MEMORY_ERROR, "could not allocate memory");
        return TURTLE_RETURN_SUCCESS;
}

/* [ref stepper.c:472-509] */
enum turtle_return turtle_stepper_add_map(
    struct turtle_stepper * stepper, struct turtle_map * map, double offset)
{
        TAMD_ERROR_INIT(&turtle_stepper_add_map);
        VIEW_OUT_GUARD(stepper);
        int i, data = -1;
        for (i = 0; i < stepper->n_data; i++)
                if ((stepper->data[i].kind == TAMD_MAP) && (stepper->data[i].map == map))
                        data = i;
        if (data < 0) {
                const struct tamd_data d = { TAMD_MAP, map, NULL, NULL };
                data = push_data(stepper, &d);
        }
        if ((data < 0) || push_meta(stepper, data, offset))
                return TAMD_RAISE(TURTLE_RETURN_MEMORY_ERROR, "could not allocate memory");
        return TURTLE_RETURN_SUCCESS;
}

/* [ref stepper.c:511-545] */
enum turtle_return turtle_stepper_add_flat(struct turtle_stepper * stepper, double offset)
{
        TAMD_ERROR_INIT(&turtle_stepper_add_flat);
        VIEW_OUT_GUARD(stepper);
        int i, data = -1;
        for (i = 0; i < stepper->n_data; i++)
                if (stepper->data[i].kind == TAMD_FLAT) data = i;
        if (data < 0) {
                const struct tamd_data d = { TAMD_FLAT, NULL, NULL, NULL };
                data = push_data(stepper, &d);
        }
        if ((data < 0) || push_meta(stepper, data, offset))
                return TAMD_RAISE(TURTLE_RETURN_MEMORY_ERROR, "could not allocate memory");
        return TURTLE_RETURN_SUCCESS;
}

/* A second stepper over the same geometry: the layers and their data in the order they
 * were added, the geoid and the settings (turtle_amd.h: one stepper is one stream of
 * calls; a batch more in flight takes a stepper more).  Built with the public calls, so
 * that it is exactly what the caller's own sequence of them would have made. */
enum turtle_return turtle_amd_stepper_clone(
    const struct turtle_stepper * stepper, struct turtle_stepper ** clone)
{
        TAMD_ERROR_INIT(&turtle_amd_stepper_clone);
        if ((stepper == NULL) || (clone == NULL))
                return TAMD_RAISE(TURTLE_RETURN_BAD_ADDRESS, "a stepper and where to put its clone");
        *clone = NULL;
        struct turtle_stepper * c = NULL;
        enum turtle_return rc = turtle_stepper_create(&c);
        int i, j;
        for (i = 0; (rc == TURTLE_RETURN_SUCCESS) && (i < stepper->n_layers); i++) {
                /* (an empty layer is one more add_layer: push_layer reuses an empty top layer) */
                rc = turtle_stepper_add_layer(c);
                for (j = 0; (rc == TURTLE_RETURN_SUCCESS) && (j < stepper->layers[i].size); j++) {
                        const struct tamd_layer_meta * m = &stepper->layers[i].meta[j];
                        const struct tamd_data * d = &stepper->data[m->data];
                        if (d->kind == TAMD_MAP)
                                rc = turtle_stepper_add_map(c, d->map, m->offset);
                        else if (d->kind == TAMD_STACK)
                                rc = turtle_stepper_add_stack(c, d->stack, m->offset);
                        else
                                rc = turtle_stepper_add_flat(c, m->offset);
                }
        }
        if (rc != TURTLE_RETURN_SUCCESS) {
                turtle_stepper_destroy(&c);
                return rc;
        }
        c->geoid = stepper->geoid;
        c->local_range = stepper->local_range;
        c->slope_factor = stepper->slope_factor;
        c->resolution_factor = stepper->resolution_factor;
        *clone = c;
        return TURTLE_RETURN_SUCCESS;
}

/* ---- setters/getters [ref stepper.c:617-672] ----------------------------- */

void turtle_stepper_geoid_set(struct turtle_stepper * stepper, struct turtle_map * geoid)
{
        stepper->geoid = geoid;
        stepper->last.valid = 0;
        tamd_geometry_changed();
}

struct turtle_map * turtle_stepper_geoid_get(const struct turtle_stepper * stepper)
{
        return stepper->geoid;
}

double turtle_stepper_range_get(const struct turtle_stepper * stepper)
{
        return stepper->local_range;
}

void turtle_stepper_range_set(struct turtle_stepper * stepper, double range)
{
        stepper->local_range = range; /* recorded only: see turtle_amd.h */
}

/* nothing is cached between calls, so there is no history to reset */
/* [ref stepper.c:662-672]: forgets the cached sample (the scalar calls on the host keep one) */
void turtle_stepper_reset(struct turtle_stepper * stepper) { stepper->last.valid = 0; }

double turtle_stepper_slope_get(const struct turtle_stepper * stepper)
{
        return stepper->slope_factor;
}

void turtle_stepper_slope_set(struct turtle_stepper * stepper, double slope)
{
        stepper->slope_factor = slope;
}

double turtle_stepper_resolution_get(const struct turtle_stepper * stepper)
{
        return stepper->resolution_factor;
}

void turtle_stepper_resolution_set(struct turtle_stepper * stepper, double resolution)
{
        stepper->resolution_factor = resolution;
}

/* ---- flattening ---------------------------------------------------------- */

struct grid_list {
        struct turtle_map ** map;
        int n, cap;
};

static int grid_index(struct grid_list * g, struct turtle_map * m)
{
        int i;
        for (i = 0; i < g->n; i++)
                if (g->map[i] == m) return i;
        if (g->n == g->cap) {
                const int cap = g->cap ? 2 * g->cap : 16;
                struct turtle_map ** p = realloc(g->map, cap * sizeof(*p));
                if (p == NULL) return -1;
                g->map = p, g->cap = cap;
        }
        g->map[g->n] = m;
        return g->n++;
}

static int stepper_flatten_locked(struct turtle_stepper * s, char * message, size_t size);

/* Returns 0, -1 for a device error (tamd_dev_error has the text), or a
 * positive enum turtle_return with `message` filled in. */
int tamd_stepper_flatten(struct turtle_stepper * s, char * message, size_t size)
{
        if (stepper_bind_device(s)) return -1;
        if (s->d_stats == NULL) {
                const size_t words = TAMD_STATS_WORDS;
                if (tamd_dev_malloc((void **)&s->d_stats, words * sizeof(*s->d_stats))) return -1;
                if (tamd_dev_zero(s->d_stats, words * sizeof(*s->d_stats))) return -1;
        }
        s->view.slope = s->slope_factor;
        s->view.resolution = s->resolution_factor;
        /* a view of it is out: the tables it names stay (nothing they point at can go meanwhile:
         * the view holds the geometry in use) */
        if (s->view_out && (s->d_tables != NULL)) return 0;
        if ((s->epoch == tamd_geometry_epoch_get()) && (s->d_tables != NULL)) return 0;
        /* the lists of tiles are read, and maps uploaded, under the lock */
        tamd_geometry_lock();
        const int rc_ = stepper_flatten_locked(s, message, size);
        tamd_geometry_unlock();
        return rc_;
}

static int stepper_flatten_locked(struct turtle_stepper * s, char * message, size_t size)
{
        const unsigned long epoch_now = tamd_geometry_epoch_get();

        /* the tiles that are in memory go into the tables; the others read
         * TAMD_TILE_PAGED there and come in when a batch wants them (paging.c) */
        int i, j, n_stacks = 0, n_tiles = 0, n_metas = 0;
        for (i = 0; i < s->n_data; i++) {
                if (s->data[i].kind != TAMD_STACK) continue;
                n_stacks++;
                n_tiles += s->data[i].stack->latitude_n * s->data[i].stack->longitude_n;
        }
        s->n_table = n_tiles;
        for (i = 0; i < s->n_layers; i++) n_metas += s->layers[i].size;

        /* unique grids: maps, tiles, geoid */
        struct grid_list gl = { NULL, 0, 0 };
        int rc = 0;
        int * data_src = calloc(s->n_data + 1, sizeof(*data_src));
        int * tiles = calloc(n_tiles + 1, sizeof(*tiles));
        struct tamd_stack * stacks = calloc(n_stacks + 1, sizeof(*stacks));
        if ((data_src == NULL) || (tiles == NULL) || (stacks == NULL)) rc = 1;
        int stack_count = 0, tile_count = 0;
        for (i = 0; (rc == 0) && (i < s->n_data); i++) {
                struct tamd_data * d = &s->data[i];
                if (d->kind == TAMD_MAP) {
                        data_src[i] = grid_index(&gl, d->map);
                        if (data_src[i] < 0) rc = 1;
                } else if (d->kind == TAMD_STACK) {
                        struct turtle_stack * st = d->stack;
                        struct tamd_stack * t = &stacks[stack_count];
                        t->lat0 = st->latitude_0, t->lon0 = st->longitude_0;
                        t->dlat = st->latitude_delta, t->dlon = st->longitude_delta;
                        t->inv_dlat = 1. / t->dlat, t->inv_dlon = 1. / t->dlon;
                        t->nlat = st->latitude_n, t->nlon = st->longitude_n;
                        t->tile_first = tile_count;
                        const int slots = st->latitude_n * st->longitude_n;
                        for (j = 0; (rc == 0) && (j < slots); j++) {
                                int g = (st->path[j] != NULL) ? TAMD_TILE_PAGED : TAMD_TILE_NONE;
                                if (st->tile[j] != NULL) {
                                        g = grid_index(&gl, st->tile[j]);
                                        if (g < 0) rc = 1;
                                }
                                tiles[tile_count++] = g;
                        }
                        data_src[i] = stack_count++;
                }
        }
        int geoid = -1;
        if ((rc == 0) && (s->geoid != NULL)) {
                geoid = grid_index(&gl, s->geoid);
                if (geoid < 0) rc = 1;
        }
        if (rc != 0) {
                free(gl.map), free(data_src), free(tiles), free(stacks);
                snprintf(message, size, "could not allocate memory");
                return TURTLE_RETURN_MEMORY_ERROR;
        }

        /* one blob: grids | stacks | metas | layer_first | tiles | slot_nodes */
        const size_t o_grids = 0;
        const size_t o_stacks = o_grids + (size_t)(gl.n + 1) * sizeof(struct tamd_grid);
        const size_t o_metas = o_stacks + (size_t)(n_stacks + 1) * sizeof(struct tamd_stack);
        const size_t o_first = o_metas + (size_t)(n_metas + 1) * sizeof(struct tamd_meta);
        const size_t o_tiles = o_first + (size_t)(s->n_layers + 2) * sizeof(int);
        const size_t o_nodes =
            (o_tiles + (size_t)(n_tiles + 1) * sizeof(int) + 15) & ~(size_t)15;
        const size_t bytes = o_nodes + (size_t)(n_tiles + 1) * sizeof(void *);
        char * host = calloc(1, bytes);
        if (host == NULL) {
                free(gl.map), free(data_src), free(tiles), free(stacks);
                snprintf(message, size, "could not allocate memory");
                return TURTLE_RETURN_MEMORY_ERROR;
        }
        struct tamd_grid * h_grids = (struct tamd_grid *)(host + o_grids);
        struct tamd_meta * h_metas = (struct tamd_meta *)(host + o_metas);
        int * h_first = (int *)(host + o_first);
        int dev_fail = 0;
        for (i = 0; i < gl.n; i++)
                if (tamd_map_sync(gl.map[i], &h_grids[i])) dev_fail = 1;
        /* regular stacks: shared tile shape + one node pointer per slot */
        const uint16_t ** h_nodes = (const uint16_t **)(host + o_nodes);
        int fast_ok = 1;
        for (i = 0; i < gl.n; i++)
                if ((h_grids[i].nx < 2) || (h_grids[i].ny < 2)) fast_ok = 0;
        for (i = 0; i < n_stacks; i++) {
                struct tamd_stack * t = &stacks[i];
                const int slots = t->nlat * t->nlon;
                const struct tamd_grid * proto = NULL;
                /* slot and cell share a 32-bit id in the lanes' caches (slot << 24 |
                 * cell, ~0u: empty): at most 254 slots of at most 2^24 cells */
                int regular = (slots > 0) && (slots <= 254);
                t->nodes_first = t->tile_first;
                for (j = 0; j < slots; j++) {
                        const int g = tiles[t->tile_first + j];
                        h_nodes[t->nodes_first + j] = (g >= 0) ? h_grids[g].nodes : NULL;
                        if (g < 0) continue;
                        const struct tamd_grid * q = &h_grids[g];
                        if (proto == NULL) proto = q;
                        if (((size_t)q->nx * (size_t)q->ny > ((size_t)1 << 24)) || (q->nx != proto->nx) || (q->ny != proto->ny) ||
                            (q->dx != proto->dx) || (q->dy != proto->dy) ||
                            (q->z0 != proto->z0) || (q->dz != proto->dz) ||
                            (q->is_signed != proto->is_signed) ||
                            (q->x0 != t->lon0 + (j % t->nlon) * t->dlon) ||
                            (q->y0 != t->lat0 + (j / t->nlon) * t->dlat) ||
                            /* ... and spans its lattice cell, no more */
                            (fabs((q->nx - 1) * q->dx - t->dlon) > 1E-10 * fabs(t->dlon)) ||
                            (fabs((q->ny - 1) * q->dy - t->dlat) > 1E-10 * fabs(t->dlat)))
                                regular = 0;
                }
                t->regular = regular && (proto != NULL);
                if (t->regular) t->proto = *proto;
        }
        memcpy(host + o_stacks, stacks, (size_t)n_stacks * sizeof(*stacks));
        memcpy(host + o_tiles, tiles, (size_t)n_tiles * sizeof(*tiles));
        int m = 0;
        for (i = 0; i < s->n_layers; i++) {
                h_first[i] = m;
                /* last added first [ref stepper.c:722-724] */
                for (j = s->layers[i].size - 1; j >= 0; j--, m++) {
                        const struct tamd_layer_meta * lm = &s->layers[i].meta[j];
                        h_metas[m].kind = s->data[lm->data].kind;
                        h_metas[m].src = data_src[lm->data];
                        h_metas[m].offset = lm->offset;
                }
        }
        h_first[s->n_layers] = m;

        if (!dev_fail && (bytes > s->d_tables_size)) {
                tamd_dev_sync();
                tamd_dev_free(s->d_tables);
                s->d_tables = NULL, s->d_tables_size = 0;
                if (tamd_dev_malloc(&s->d_tables, bytes))
                        dev_fail = 1;
                else
                        s->d_tables_size = bytes;
        }
        if (!dev_fail && tamd_dev_h2d(s->d_tables, host, bytes)) dev_fail = 1;

        if (!dev_fail) {
                char * d = s->d_tables;
                s->view.grids = (const struct tamd_grid *)(d + o_grids);
                s->view.stacks = (const struct tamd_stack *)(d + o_stacks);
                s->view.metas = (const struct tamd_meta *)(d + o_metas);
                s->view.layer_first = (const int *)(d + o_first);
                s->view.tiles = (const int *)(d + o_tiles);
                s->view.slot_nodes = (const uint16_t * const *)(d + o_nodes);
                s->view.fast_ok = fast_ok;
                s->view.n_layers = s->n_layers;
                s->view.geoid = geoid;
                s->view.mode = TAMD_MODE_GENERIC;
                if ((s->n_layers == 1) && (n_metas == 1) && (geoid < 0)) {
                        if ((h_metas[0].kind == TAMD_MAP) &&
                            (h_grids[h_metas[0].src].proj.type < 0))
                                s->view.mode = TAMD_MODE_ONE_MAP;
                        if (h_metas[0].kind == TAMD_STACK) s->view.mode = TAMD_MODE_ONE_STACK;
                }
                s->epoch = epoch_now;
        }
        free(host), free(gl.map), free(data_src), free(tiles), free(stacks);
        return dev_fail ? -1 : 0;
}

/* What stepper_rounds, stepper_resident or tamd_stepper_flatten returned (not 0), raised: a
 * device failure (< 0, or TURTLE_RETURN_LIBRARY_ERROR) with the device's text, any other code
 * with the text they left in stepper->message */
#define RAISE_ROUNDS(stepper, rc)                                              \
        ((((rc) < 0) || ((rc) == TURTLE_RETURN_LIBRARY_ERROR)) ?               \
                TAMD_RAISE_DEVICE() :                                          \
                TAMD_RAISE((enum turtle_return)(rc), "%s", (stepper)->message))
#define FLATTEN(stepper) tamd_stepper_flatten((stepper), (stepper)->message, sizeof((stepper)->message))

/* ---- batch calls over paged stacks (paging.c) --------------------------- */

static int stepper_is_paged(const struct turtle_stepper * s)
{
        int i;
        for (i = 0; i < s->n_data; i++)
                if ((s->data[i].kind == TAMD_STACK) && tamd_stack_is_paged(s->data[i].stack)) return 1;
        return 0;
}

/* the tiles a round wanted, stack by stack (the tile table lists the stacks in
 * the order of s->data): 0 if none could come in, -1 with `code` set on error */
static int stepper_page_in(struct turtle_stepper * s, const unsigned * wanted,
    const unsigned * wanted_first, int few, int * code, char * message, size_t size)
{
        int i, first = 0, loaded = 0;
        for (i = 0; i < s->n_data; i++) {
                if (s->data[i].kind != TAMD_STACK) continue;
                struct turtle_stack * st = s->data[i].stack;
                const int got = tamd_stack_page_in(st, wanted, wanted_first, first, few, message, size);
                if (got < 0) {
                        *code = -got;
                        return -1;
                }
                loaded += got;
                first += st->latitude_n * st->longitude_n;
        }
        return loaded;
}

/* Runs `launch` (the kernels of one round) until nothing is listed any more.
 * Returns an enum turtle_return; TURTLE_RETURN_LIBRARY_ERROR: device failure; any
 * other failure has its text in stepper->message (RAISE_ROUNDS raises either) */
typedef int stepper_round_t(struct turtle_stepper * stepper, struct tamd_paging pg, int round,
    void * args);

static int stepper_rounds(struct turtle_stepper * stepper, long n, stepper_round_t * launch, void * args)
{
        char * const message = stepper->message;
        const size_t size = sizeof(stepper->message);
        struct tamd_pager pager;
        memset(&pager, 0, sizeof(pager));
        message[0] = 0;
        int paged = 0; /* did this call bring tiles in? */
        int rc = tamd_stepper_flatten(stepper, message, size);
        if (rc != 0) return (rc < 0) ? TURTLE_RETURN_LIBRARY_ERROR : rc;
        if (stepper_is_paged(stepper) && tamd_pager_begin(&pager, n, stepper->n_table))
                return TURTLE_RETURN_LIBRARY_ERROR;
        static int trace_rounds = -1; /* TURTLE_AMD_PAGING_TRACE=1: the time of each round, to stderr */
        if (trace_rounds < 0) trace_rounds = (getenv("TURTLE_AMD_PAGING_TRACE") != NULL);
        for (;;) {
                struct tamd_paging pg;
                struct timespec t0, t1, t2, t3;
                if (trace_rounds) clock_gettime(CLOCK_MONOTONIC, &t0);
                /* tables and launches of a round: nothing they point at may go meanwhile */
                tamd_geometry_use_begin();
                rc = tamd_stepper_flatten(stepper, message, size);
                if (rc != 0)
                        rc = (rc < 0) ? TURTLE_RETURN_LIBRARY_ERROR : rc;
                else if (tamd_pager_round(&pager, &pg) || launch(stepper, pg, pager.rounds, args))
                        rc = TURTLE_RETURN_LIBRARY_ERROR;
                tamd_geometry_use_end();
                if (rc != 0) break;
                if (trace_rounds) clock_gettime(CLOCK_MONOTONIC, &t1);
                unsigned long long faulted = 0;
                if (tamd_pager_collect(&pager, &faulted)) {
                        rc = TURTLE_RETURN_LIBRARY_ERROR;
                        break;
                }
                if (trace_rounds) clock_gettime(CLOCK_MONOTONIC, &t2);
                if (faulted == 0) {
                        if (trace_rounds)
                                fprintf(stderr, "[paging] round %d: tables+launch %.2f ms, kernels %.2f ms, done\n", pager.rounds,
                                    1e3 * (t1.tv_sec - t0.tv_sec) + 1e-6 * (t1.tv_nsec - t0.tv_nsec),
                                    1e3 * (t2.tv_sec - t1.tv_sec) + 1e-6 * (t2.tv_nsec - t1.tv_nsec));
                        break;
                }
                int code = 0;
                paged = 1;
                const int got = stepper_page_in(stepper, pager.wanted, pager.pinned,
                    faulted <= TAMD_PAGING_FEW, &code, message, size);
                if (trace_rounds) {
                        clock_gettime(CLOCK_MONOTONIC, &t3);
                        fprintf(stderr, "[paging] round %d: tables+launch %.2f ms, kernels %.2f ms, %llu items wait, %d tiles in %.2f ms (%lu from their buffers so far)\n",
                            pager.rounds, 1e3 * (t1.tv_sec - t0.tv_sec) + 1e-6 * (t1.tv_nsec - t0.tv_nsec),
                            1e3 * (t2.tv_sec - t1.tv_sec) + 1e-6 * (t2.tv_nsec - t1.tv_nsec), faulted, got,
                            1e3 * (t3.tv_sec - t2.tv_sec) + 1e-6 * (t3.tv_nsec - t2.tv_nsec), tamd_stack_buffer_hits);
                }
                if (got < 0) {
                        rc = code;
                        break;
                }
                if (pager.rounds > TAMD_PAGING_ROUNDS) { /* cannot be: a round serves an item */
                        snprintf(message, size,
                            "the stacks of the stepper are too small (stack_size) for this batch");
                        rc = TURTLE_RETURN_MEMORY_ERROR;
                        break;
                }
        }
        tamd_pager_end(&pager);
        stepper->last_rounds = (pager.rounds > 0) ? pager.rounds : 1;
        if (paged) {
                /* whatever the call came to: the tiles this thread had brought in for a
                 * round that will not run are anybody's again, and the stacks go back to
                 * their sizes (a pin never outlives the call that set it) */
                int i;
                for (i = 0; i < stepper->n_data; i++)
                        if (stepper->data[i].kind == TAMD_STACK) tamd_stack_trim(stepper->data[i].stack);
        }
        return rc;
}

/* Every tile resident: the whole call in ONE launch (no paging: pg.first_id -1), over tables
 * made current with the geometry held in use until the launch is queued.  Returns as
 * stepper_rounds.  (What turtle_amd_stepper_rounds reports is the caller's to set: scatter_n
 * leaves it as its last rounds did.) */
static int stepper_resident(struct turtle_stepper * stepper, stepper_round_t * launch, void * args)
{
        const struct tamd_paging none = { NULL, NULL, NULL, NULL, NULL, NULL, NULL, -1 };
        tamd_geometry_use_begin();
        int rc = FLATTEN(stepper);
        if ((rc < 0) || ((rc == 0) && launch(stepper, none, 0, args))) rc = TURTLE_RETURN_LIBRARY_ERROR;
        tamd_geometry_use_end();
        return rc;
}

/* Every tile of every stack in memory (turtle_stack_load): what a device view needs before its
 * span begins, and the calls over lines of sight before they launch (a wave cannot wait for a tile
 * in the middle of its reduction or its scan).  `who` `does`: the message's clause, "<who> <does>
 * resident tiles only". */
static enum turtle_return stepper_load_all(struct turtle_stepper * stepper, struct tamd_error * error,
    const char * who, const char * does)
{
        int i;
        for (i = 0; i < stepper->n_data; i++) {
                if (stepper->data[i].kind != TAMD_STACK) continue;
                struct turtle_stack * stack = stepper->data[i].stack;
                if (tamd_stack_budget(stack) < stack->n_files)
                        return tamd_raise_(error, TURTLE_RETURN_DOMAIN_ERROR, __FILE__, __LINE__,
                            "a stack of %d tiles cannot keep them all in memory (stack_size %d): "
                            "%s %s resident tiles only", stack->n_files, stack->max_size, who, does);
                if (stack->n_loaded >= stack->n_files) continue;
                if (tamd_geometry_view_held()) /* (loading takes what a view of this thread holds) */
                        return tamd_raise_(error, TURTLE_RETURN_DOMAIN_ERROR, __FILE__, __LINE__,
                            TAMD_VIEW_HELD_TEXT);
                const enum turtle_return rc = turtle_stack_load(stack);
                if (rc != TURTLE_RETURN_SUCCESS) return rc;
        }
        return TURTLE_RETURN_SUCCESS;
}

/* ---- a device view: the geometry lent to the caller's own kernel ------------- */

void turtle_amd_view_layout(int * version, size_t * size)
{
        if (version != NULL) *version = TURTLE_AMD_VIEW_VERSION;
        if (size != NULL) *size = sizeof(struct turtle_amd_view);
}

enum turtle_return turtle_amd_stepper_view_acquire(struct turtle_stepper * stepper, void * view, size_t size)
{
        TAMD_ERROR_INIT(&turtle_amd_stepper_view_acquire);
        if ((stepper == NULL) || (view == NULL))
                return TAMD_RAISE(TURTLE_RETURN_BAD_ADDRESS, "invalid null argument");
        if (size != sizeof(struct turtle_amd_view))
                return TAMD_RAISE(TURTLE_RETURN_DOMAIN_ERROR,
                    "the view is %zu bytes, this library's is %zu (version %d): build the caller with this "
                    "library's turtle_amd_device.h", size, sizeof(struct turtle_amd_view), TURTLE_AMD_VIEW_VERSION);
        if (stepper->view_out) return TAMD_RAISE(TURTLE_RETURN_DOMAIN_ERROR, "the stepper's view is out already");
        if (tamd_dev_init()) return TAMD_RAISE_DEVICE();
        const enum turtle_return loaded = stepper_load_all(stepper, &error_, "a device view", "names");
        if (loaded != TURTLE_RETURN_SUCCESS) return loaded;
        tamd_geometry_use_begin();
        int rc = FLATTEN(stepper);
        int paged = 0;
        if (rc == 0) paged = stepper_is_paged(stepper); /* (a tile another thread took meanwhile) */
        if ((rc != 0) || paged) {
                tamd_geometry_use_end();
                if (rc != 0) return RAISE_ROUNDS(stepper, rc);
                return TAMD_RAISE(TURTLE_RETURN_DOMAIN_ERROR, "a tile left its stack while the view was made: try again");
        }
        struct turtle_amd_view out;
        memset(&out, 0, sizeof(out));
        out.geometry = stepper->view;
        out.version = TURTLE_AMD_VIEW_VERSION;
        out.size = (int)sizeof(out);
        memcpy(view, &out, sizeof(out));
        stepper->view_out = 1;
        tamd_geometry_view_hold(+1);
        return TURTLE_RETURN_SUCCESS;
}

enum turtle_return turtle_amd_stepper_view_release(struct turtle_stepper * stepper)
{
        TAMD_ERROR_INIT(&turtle_amd_stepper_view_release);
        if (stepper == NULL) return TAMD_RAISE(TURTLE_RETURN_BAD_ADDRESS, "invalid null argument");
        if (!stepper->view_out || (tamd_geometry_view_held() == 0))
                return TAMD_RAISE(TURTLE_RETURN_DOMAIN_ERROR,
                    "no device view of the stepper is held by the calling thread");
        stepper->view_out = 0;
        tamd_geometry_view_hold(-1);
        tamd_geometry_use_end();
        return TURTLE_RETURN_SUCCESS;
}

/* ---- batch entry points --------------------------------------------------- */

struct position_args {
        long n;
        void *lat, *lon, *height;
        int layer;
        void *pos, *index;
};

static int position_round(struct turtle_stepper * stepper, struct tamd_paging pg, int round, void * p)
{
        struct position_args * a = p;
        (void)round;
        return tamd_k_position(stepper->view, a->n, a->lat, a->lon, a->height, a->layer, a->pos,
            a->index, pg);
}

enum turtle_return turtle_stepper_position_n(struct turtle_stepper * stepper, long n,
    const double * latitude, const double * longitude, const double * height,
    int layer_index, double * position, int * data_index, int space)
{
        TAMD_ERROR_INIT(&turtle_stepper_position_n);
        if ((layer_index < 0) || (layer_index >= stepper->n_layers))
                return TAMD_RAISE(TURTLE_RETURN_DOMAIN_ERROR, "no valid data");
        if ((position == NULL) || (data_index == NULL))
                return TAMD_RAISE(TURTLE_RETURN_BAD_ADDRESS, "invalid null argument");
        struct tamd_stage st = { 0 };
        struct position_args args = { n, NULL, NULL, NULL, layer_index, NULL, NULL };
        const size_t nb = (size_t)n * sizeof(double);
        tamd_stage_add(&st, latitude, nb, TAMD_IN, &args.lat);
        tamd_stage_add(&st, longitude, nb, TAMD_IN, &args.lon);
        tamd_stage_add(&st, height, nb, TAMD_IN, &args.height);
        tamd_stage_add(&st, position, 3 * nb, TAMD_INOUT, &args.pos); /* untouched rows keep their value */
        tamd_stage_add(&st, data_index, n * sizeof(int), TAMD_OUT, &args.index);
        if (tamd_stage_open(&st, space)) return TAMD_RAISE_DEVICE();
        const int rc = stepper_rounds(stepper, n, &position_round, &args);
        if (rc != 0) return RAISE_ROUNDS(stepper, rc);
        if (tamd_stage_close(&st)) return TAMD_RAISE_DEVICE();
        return TURTLE_RETURN_SUCCESS;
}

struct normal_args {
        long n;
        void *pos, *layer, *normal, *index;
};

static int normal_round(struct turtle_stepper * stepper, struct tamd_paging pg, int round, void * p)
{
        struct normal_args * a = p;
        (void)round;
        return tamd_k_normal(stepper->view, a->n, a->pos, a->layer, a->normal, a->index, pg);
}

enum turtle_return turtle_stepper_normal_n(struct turtle_stepper * stepper, long n,
    const double * position, const int * layer, double * normal, int * data_index, int space)
{
        TAMD_ERROR_INIT(&turtle_stepper_normal_n);
        if ((stepper == NULL) || (position == NULL) || (layer == NULL) || (normal == NULL) ||
            (data_index == NULL))
                return TAMD_RAISE(TURTLE_RETURN_BAD_ADDRESS, "invalid null argument");
        if (n <= 0) return TURTLE_RETURN_SUCCESS;
        struct tamd_stage st = { 0 };
        struct normal_args args = { n, NULL, NULL, NULL, NULL };
        const size_t nb = (size_t)n * sizeof(double);
        tamd_stage_add(&st, position, 3 * nb, TAMD_IN, &args.pos);
        tamd_stage_add(&st, layer, n * sizeof(int), TAMD_IN, &args.layer);
        tamd_stage_add(&st, normal, 3 * nb, TAMD_INOUT, &args.normal); /* untouched rows keep their value */
        tamd_stage_add(&st, data_index, n * sizeof(int), TAMD_OUT, &args.index);
        if (tamd_stage_open(&st, space)) return TAMD_RAISE_DEVICE();
        const int rc = stepper_rounds(stepper, n, &normal_round, &args);
        if (rc != 0) return RAISE_ROUNDS(stepper, rc);
        if (tamd_stage_close(&st)) return TAMD_RAISE_DEVICE();
        return TURTLE_RETURN_SUCCESS;
}

/* What the calls over lines of sight (observers x azimuths x distances, one wave a line) share:
 * the lines, staged.  Each call's own arguments embed it first. */
struct sight_lines {
        struct tamd_stage stage;
        int n_items, n_azimuths, n_distances, layer; /* n_items 0: nothing to do */
        void *pos, *azimuth, *distance;
        int paged; /* out: a tile was not resident when the tables were made current */
};

#define error_ (*error) /* (the TAMD_RAISE macros name it: the messages carry the caller's name) */

/* After the caller's NULL checks: the other checks in their order, every tile in memory, the three
 * inputs staged.  The caller adds its outputs to l->stage, then sight_run. */
static enum turtle_return sight_begin(struct tamd_error * error, struct sight_lines * l,
    struct turtle_stepper * stepper, long n, const double * position, int n_azimuths, const double * azimuth,
    int n_distances, const double * distance, int layer_index, int space)
{
        if ((layer_index < 0) || (layer_index >= stepper->n_layers))
                return TAMD_RAISE(TURTLE_RETURN_DOMAIN_ERROR, "no valid data");
        if ((space != TURTLE_AMD_HOST) && (space != TURTLE_AMD_DEVICE))
                return TAMD_RAISE(TURTLE_RETURN_DOMAIN_ERROR, "invalid space (%d)", space);
        if ((n <= 0) || (n_azimuths <= 0) || (n_distances <= 0)) return TURTLE_RETURN_SUCCESS;
        if (n > (long)(INT_MAX / n_azimuths))
                return TAMD_RAISE(TURTLE_RETURN_DOMAIN_ERROR,
                    "too many lines of sight (%ld observers x %d azimuths): the items of a call are numbered by ints",
                    n, n_azimuths);
        const enum turtle_return loaded =
            stepper_load_all(stepper, error, turtle_error_function(error->function), "reads");
        if (loaded != TURTLE_RETURN_SUCCESS) return loaded;
        l->n_items = (int)(n * n_azimuths), l->n_azimuths = n_azimuths, l->n_distances = n_distances;
        l->layer = layer_index;
        tamd_stage_add(&l->stage, position, 3 * (size_t)n * sizeof(double), TAMD_IN, &l->pos);
        tamd_stage_add(&l->stage, azimuth, (size_t)n_azimuths * sizeof(double), TAMD_IN, &l->azimuth);
        tamd_stage_add(&l->stage, distance, (size_t)n_distances * sizeof(double), TAMD_IN, &l->distance);
        return TURTLE_RETURN_SUCCESS;
}

/* `launch`, the call's own kernel over `args` (which embed l), and the closing sequence */
static enum turtle_return sight_run(struct tamd_error * error, struct sight_lines * l,
    struct turtle_stepper * stepper, int space, stepper_round_t * launch, void * args)
{
        if (tamd_stage_open(&l->stage, space)) return TAMD_RAISE_DEVICE();
        const int rc = stepper_resident(stepper, launch, args);
        stepper->last_rounds = 1;
        if (rc != 0) return RAISE_ROUNDS(stepper, rc);
        if (l->paged)
                return TAMD_RAISE(TURTLE_RETURN_DOMAIN_ERROR, "a tile left its stack while the call was made: try again");
        if (tamd_stage_close(&l->stage)) return TAMD_RAISE_DEVICE();
        return TURTLE_RETURN_SUCCESS;
}

#undef error_

struct horizon_args {
        struct sight_lines lines;
        void *elevation, *sample, *range;
};

static int horizon_resident(struct turtle_stepper * stepper, struct tamd_paging pg, int round, void * p)
{
        struct horizon_args * a = p;
        struct sight_lines * l = &a->lines;
        (void)pg, (void)round;
        if ((l->paged = stepper_is_paged(stepper))) return 0; /* (a tile another thread took meanwhile) */
        return tamd_k_horizon(stepper->view, l->n_items, l->n_azimuths, l->n_distances, l->pos, l->azimuth,
            l->distance, l->layer, a->elevation, a->sample, a->range);
}

enum turtle_return turtle_stepper_horizon_n(struct turtle_stepper * stepper, long n,
    const double * position, int n_azimuths, const double * azimuth, int n_distances,
    const double * distance, int layer_index, double * elevation, int * sample, double * range, int space)
{
        TAMD_ERROR_INIT(&turtle_stepper_horizon_n);
        if ((stepper == NULL) || (position == NULL) || (azimuth == NULL) || (distance == NULL) ||
            (elevation == NULL) || (sample == NULL))
                return TAMD_RAISE(TURTLE_RETURN_BAD_ADDRESS, "invalid null argument");
        struct horizon_args a = { 0 };
        const enum turtle_return rc = sight_begin(&error_, &a.lines, stepper, n, position, n_azimuths, azimuth,
            n_distances, distance, layer_index, space);
        if ((rc != TURTLE_RETURN_SUCCESS) || (a.lines.n_items == 0)) return rc;
        const size_t items = (size_t)a.lines.n_items;
        tamd_stage_add(&a.lines.stage, elevation, items * sizeof(double), TAMD_INOUT, &a.elevation); /* lines without */
        tamd_stage_add(&a.lines.stage, range, items * sizeof(double), TAMD_INOUT, &a.range); /* a sample keep theirs */
        tamd_stage_add(&a.lines.stage, sample, items * sizeof(int), TAMD_OUT, &a.sample);
        return sight_run(&error_, &a.lines, stepper, space, &horizon_resident, &a);
}

struct viewshed_args {
        struct sight_lines lines;
        double target_height;
        void *visible, *sine, *horizon, *n_visible;
};

static int viewshed_resident(struct turtle_stepper * stepper, struct tamd_paging pg, int round, void * p)
{
        struct viewshed_args * a = p;
        struct sight_lines * l = &a->lines;
        (void)pg, (void)round;
        if ((l->paged = stepper_is_paged(stepper))) return 0; /* (a tile another thread took meanwhile) */
        return tamd_k_viewshed(stepper->view, l->n_items, l->n_azimuths, l->n_distances, l->pos, l->azimuth,
            l->distance, l->layer, a->target_height, a->visible, a->sine, a->horizon, a->n_visible);
}

enum turtle_return turtle_stepper_viewshed_n(struct turtle_stepper * stepper, long n,
    const double * position, int n_azimuths, const double * azimuth, int n_distances,
    const double * distance, int layer_index, double target_height, signed char * visible, double * sine,
    double * horizon, int * n_visible, int space)
{
        TAMD_ERROR_INIT(&turtle_stepper_viewshed_n);
        if ((stepper == NULL) || (position == NULL) || (azimuth == NULL) || (distance == NULL) ||
            (visible == NULL))
                return TAMD_RAISE(TURTLE_RETURN_BAD_ADDRESS, "invalid null argument");
        struct viewshed_args a = { 0 };
        const enum turtle_return rc = sight_begin(&error_, &a.lines, stepper, n, position, n_azimuths, azimuth,
            n_distances, distance, layer_index, space);
        if ((rc != TURTLE_RETURN_SUCCESS) || (a.lines.n_items == 0)) return rc;
        const size_t items = (size_t)a.lines.n_items, elements = items * (size_t)n_distances;
        a.target_height = target_height;
        tamd_stage_add(&a.lines.stage, visible, elements * sizeof(signed char), TAMD_OUT, &a.visible); /* every */
        tamd_stage_add(&a.lines.stage, sine, elements * sizeof(double), TAMD_OUT, &a.sine); /* element of each is */
        tamd_stage_add(&a.lines.stage, horizon, elements * sizeof(double), TAMD_OUT, &a.horizon); /* written: nothing */
        tamd_stage_add(&a.lines.stage, n_visible, items * sizeof(int), TAMD_OUT, &a.n_visible); /* to copy in */
        return sight_run(&error_, &a.lines, stepper, space, &viewshed_resident, &a);
}

/* The chords of turtle_stepper_clearance_n are not sight_begin's fans (no azimuths, no distances):
 * the call has a begin of its own, with the same checks in the same order, and shares the stage,
 * the residency and sight_run.  Of `lines`: n_azimuths holds the targets of an observer (1 where
 * paired), n_distances the fractions; azimuth and distance stay NULL. */
struct clearance_args {
        struct sight_lines lines;
        int paired;
        void *target, *fraction, *clearance, *sample, *n_data;
};

static int clearance_resident(struct turtle_stepper * stepper, struct tamd_paging pg, int round, void * p)
{
        struct clearance_args * a = p;
        struct sight_lines * l = &a->lines;
        (void)pg, (void)round;
        if ((l->paged = stepper_is_paged(stepper))) return 0; /* (a tile another thread took meanwhile) */
        return tamd_k_clearance(stepper->view, l->n_items, l->n_azimuths, a->paired, l->n_distances, l->pos,
            a->target, a->fraction, l->layer, a->clearance, a->sample, a->n_data);
}

enum turtle_return turtle_stepper_clearance_n(struct turtle_stepper * stepper, long n,
    const double * observer, long m, const double * target, int n_fractions, const double * fraction,
    int layer_index, int flags, double * clearance, int * sample, int * n_data, int space)
{
        TAMD_ERROR_INIT(&turtle_stepper_clearance_n);
        if ((stepper == NULL) || (observer == NULL) || (target == NULL) || (fraction == NULL) ||
            (clearance == NULL) || (sample == NULL))
                return TAMD_RAISE(TURTLE_RETURN_BAD_ADDRESS, "invalid null argument");
        if ((layer_index < 0) || (layer_index >= stepper->n_layers))
                return TAMD_RAISE(TURTLE_RETURN_DOMAIN_ERROR, "no valid data");
        if ((space != TURTLE_AMD_HOST) && (space != TURTLE_AMD_DEVICE))
                return TAMD_RAISE(TURTLE_RETURN_DOMAIN_ERROR, "invalid space (%d)", space);
        if (flags & ~TURTLE_AMD_CLEARANCE_PAIRED)
                return TAMD_RAISE(TURTLE_RETURN_DOMAIN_ERROR, "invalid flags (%d)", flags);
        const int paired = (flags & TURTLE_AMD_CLEARANCE_PAIRED) != 0;
        if (paired && (m != n))
                return TAMD_RAISE(TURTLE_RETURN_DOMAIN_ERROR,
                    "paired lines need as many targets as observers (%ld observers, %ld targets)", n, m);
        if ((n <= 0) || (m <= 0) || (n_fractions <= 0)) return TURTLE_RETURN_SUCCESS;
        if (paired ? (n > (long)INT_MAX) : (n > (long)INT_MAX / m))
                return TAMD_RAISE(TURTLE_RETURN_DOMAIN_ERROR,
                    "too many lines (%ld observers, %ld targets): the items of a call are numbered by ints", n, m);
        const enum turtle_return loaded =
            stepper_load_all(stepper, &error_, turtle_error_function(error_.function), "reads");
        if (loaded != TURTLE_RETURN_SUCCESS) return loaded;
        struct clearance_args a = { 0 };
        struct sight_lines * l = &a.lines;
        a.paired = paired;
        l->n_items = paired ? (int)n : (int)(n * m), l->n_azimuths = paired ? 1 : (int)m;
        l->n_distances = n_fractions, l->layer = layer_index;
        const size_t items = (size_t)l->n_items;
        tamd_stage_add(&l->stage, observer, 3 * (size_t)n * sizeof(double), TAMD_IN, &l->pos);
        tamd_stage_add(&l->stage, target, 3 * (size_t)m * sizeof(double), TAMD_IN, &a.target);
        tamd_stage_add(&l->stage, fraction, (size_t)n_fractions * sizeof(double), TAMD_IN, &a.fraction);
        tamd_stage_add(&l->stage, clearance, items * sizeof(double), TAMD_INOUT, &a.clearance); /* lines without */
        tamd_stage_add(&l->stage, sample, items * sizeof(int), TAMD_OUT, &a.sample);          /* a sample keep theirs */
        tamd_stage_add(&l->stage, n_data, items * sizeof(int), TAMD_OUT, &a.n_data);
        return sight_run(&error_, l, stepper, space, &clearance_resident, &a);
}

/* Grow-only scratch of the batch calls: one block, whose regions trace_room.h names and lays
 * out for the n of each call (a block for more rays holds every smaller layout).  0 if it holds
 * n rays; 1 if n is beyond an int (the caller does without); room_capacity < 0 after a device
 * failure. */
static int tamd_stepper_scratch(struct turtle_stepper * stepper, long n)
{
        if (n >= 2147483647L) return 1;
        if (stepper_bind_device(stepper)) {
                stepper->room_capacity = -1;
                return 1;
        }
        if (n <= stepper->room_capacity) return 0;
        if (stepper->d_room != NULL) {
                tamd_dev_sync();
                tamd_dev_free(stepper->d_room);
                stepper->d_room = NULL;
        }
        struct tamd_trace_room room;
        stepper->room_capacity = 0;
        if (tamd_dev_malloc(&stepper->d_room, tamd_trace_room_layout(&room, n))) {
                stepper->room_capacity = -1;
                return 1;
        }
        stepper->room_capacity = n;
        return 0;
}

/* the crossing list of a batch of n single steps, in the scratch (n rays fit: the caller saw to it) */
static int * stepper_cross_list(const struct turtle_stepper * stepper, long n, double ** cross_ds)
{
        struct tamd_trace_room room;
        tamd_trace_room_layout(&room, n);
        *cross_ds = TAMD_ROOM_AT(double, stepper->d_room, room.cross_ds);
        return TAMD_ROOM_AT(int, stepper->d_room, room.cross_ray);
}

struct step_args {
        long n;
        void *pos, *dir, *lat, *lon, *alt, *elev, *step, *index;
        int flags, listed;
};

static int step_round(struct turtle_stepper * stepper, struct tamd_paging pg, int round, void * p)
{
        struct step_args * a = p;
        (void)round;
        if (a->dir == NULL)
                return tamd_k_step(stepper->view, a->n, a->pos, a->dir, a->lat, a->lon, a->alt,
                    a->elev, a->step, a->index, a->flags, pg);
        double * cross_ds = NULL;
        int * const cross_ray = a->listed ? stepper_cross_list(stepper, a->n, &cross_ds) : NULL;
        return tamd_k_step_dir(stepper->view, a->n, a->pos, a->dir, a->lat, a->lon, a->alt, a->elev,
            a->step, a->index, a->flags, cross_ray, cross_ds, pg, stepper->d_stats,
            stepper->d_stats + TAMD_STATS_QUEUE);
}

static enum turtle_return step_n(struct tamd_error * error, struct turtle_stepper * stepper,
    long n, double * position, const double * direction, double * latitude,
    double * longitude, double * altitude, double * elevation, double * step, int * index,
    int flags, int space)
{
        struct tamd_error error_ = *error;
        if ((position == NULL) || (index == NULL))
                return TAMD_RAISE(TURTLE_RETURN_BAD_ADDRESS, "invalid null argument");
        if ((flags & TURTLE_AMD_STEP_RESUME) && !(flags & TAMD_STEP_COMPACT) &&
            ((altitude == NULL) || (elevation == NULL)))
                return TAMD_RAISE(TURTLE_RETURN_BAD_ADDRESS,
                    "TURTLE_AMD_STEP_RESUME needs altitude, elevation and index");
        struct tamd_stage st = { 0 };
        struct step_args args = { n, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, flags, 0 };
        const size_t nb = (size_t)n * sizeof(double);
        /* a step moves the position; a sample leaves it.  The sample is the call's result, and
         * what a resumed call starts from as well */
        const int sample = (flags & TURTLE_AMD_STEP_RESUME) ? TAMD_INOUT : TAMD_OUT;
        tamd_stage_add(&st, position, 3 * nb, (direction != NULL) ? TAMD_INOUT : TAMD_IN, &args.pos);
        tamd_stage_add(&st, direction, 3 * nb, TAMD_IN, &args.dir);
        tamd_stage_add(&st, latitude, nb, sample, &args.lat);
        tamd_stage_add(&st, longitude, nb, sample, &args.lon);
        tamd_stage_add(&st, altitude, nb, sample, &args.alt);
        tamd_stage_add(&st, elevation, 2 * nb, sample, &args.elev);
        tamd_stage_add(&st, index, 2 * n * sizeof(int), sample, &args.index);
        tamd_stage_add(&st, step, nb, TAMD_OUT, &args.step);
        if (tamd_stage_open(&st, space)) return TAMD_RAISE_DEVICE();
        /* with a direction: two passes, the second for the rays that crossed a
         * boundary (a single step bisects in place: nothing to pack) */
        args.listed = (direction != NULL) && (n > 1) && (tamd_stepper_scratch(stepper, n) == 0);
        if ((direction != NULL) && (n > 1) && !args.listed && (stepper->room_capacity < 0))
                return TAMD_RAISE_DEVICE();
        const int rc = stepper_rounds(stepper, n, &step_round, &args);
        if (rc != 0) return RAISE_ROUNDS(stepper, rc);
        if (tamd_stage_close(&st)) return TAMD_RAISE_DEVICE();
        return TURTLE_RETURN_SUCCESS;
}

/* ---- scattering walk ------------------------------------------------------ */

struct walk_args {
        long n;
        void *pos, *alt, *elev, *index, *length, *steps;
        unsigned long long seed, stream;
        long first;
        int first_step, n_steps;
};

static int walk_round(struct turtle_stepper * stepper, struct tamd_paging pg, int round, void * p)
{
        struct walk_args * a = p;
        (void)round;
        double * cross_ds;
        int * const cross_ray = stepper_cross_list(stepper, a->n, &cross_ds);
        return tamd_k_step_walk(stepper->view, a->n, a->pos, a->alt, a->elev, a->index, a->seed,
            a->stream, a->first, a->length, a->steps, cross_ray, cross_ds, pg, stepper->d_stats,
            stepper->d_stats + TAMD_STATS_QUEUE);
}

static int walk_start_round(struct turtle_stepper * stepper, struct tamd_paging pg, int round, void * p)
{
        struct walk_args * a = p;
        (void)round;
        return tamd_k_step(stepper->view, a->n, a->pos, NULL, NULL, NULL, a->alt, a->elev, NULL,
            a->index, 0, pg);
}

static int walk_resident(struct turtle_stepper * stepper, struct tamd_paging pg, int round, void * p)
{
        struct walk_args * a = p;
        (void)pg, (void)round;
        return tamd_k_walk(stepper->view, a->n, a->pos, a->alt, a->elev, a->index, a->seed, a->first,
            a->first_step, a->n_steps, a->length, a->steps, stepper->d_stats,
            stepper->d_stats + TAMD_STATS_QUEUE);
}

enum turtle_return turtle_stepper_scatter_n(struct turtle_stepper * stepper, long n,
    double * position, unsigned long long seed, long first_ray, int first_step, int n_steps,
    double * altitude, double * elevation, int * index, double * length, int * steps, int flags,
    int space)
{
        TAMD_ERROR_INIT(&turtle_stepper_scatter_n);
        if ((position == NULL) || (altitude == NULL) || (elevation == NULL) || (index == NULL) ||
            (length == NULL) || (steps == NULL))
                return TAMD_RAISE(TURTLE_RETURN_BAD_ADDRESS, "invalid null argument");
        if ((n_steps < 0) || (first_step < 0))
                return TAMD_RAISE(TURTLE_RETURN_DOMAIN_ERROR, "invalid input parameter(s)");
        if (n <= 0) return TURTLE_RETURN_SUCCESS;
        if (tamd_stepper_scratch(stepper, n) != 0) {
                if (stepper->room_capacity < 0) return TAMD_RAISE_DEVICE();
                return TAMD_RAISE(TURTLE_RETURN_MEMORY_ERROR, "batch too large");
        }
        struct tamd_stage st = { 0 };
        struct walk_args a = { n, NULL, NULL, NULL, NULL, NULL, NULL, seed, 0, first_ray, first_step, n_steps };
        const size_t nb = (size_t)n * sizeof(double);
        const int start = (flags & TURTLE_AMD_SCATTER_START) != 0;
        const int state = start ? TAMD_OUT : TAMD_INOUT; /* made here, or carried from call to call */
        tamd_stage_add(&st, position, 3 * nb, TAMD_INOUT, &a.pos);
        tamd_stage_add(&st, altitude, nb, state, &a.alt);
        tamd_stage_add(&st, elevation, 2 * nb, state, &a.elev);
        tamd_stage_add(&st, index, 2 * n * sizeof(int), state, &a.index);
        tamd_stage_add(&st, length, nb, state, &a.length);
        tamd_stage_add(&st, steps, n * sizeof(int), state, &a.steps);
        if (tamd_stage_open(&st, space)) return TAMD_RAISE_DEVICE();
        int rc = 0, k;
        if (start) {
                rc = stepper_rounds(stepper, n, &walk_start_round, &a);
                if ((rc == 0) && (tamd_dev_zero(a.length, nb) || tamd_dev_zero(a.steps, n * sizeof(int))))
                        rc = TURTLE_RETURN_LIBRARY_ERROR;
        } else if (stepper->d_stats == NULL)
                rc = FLATTEN(stepper);
        /* the counters are those of THIS call (turtle_stepper_trace_stats), whatever the
         * stepper's last batch left there */
        if ((rc == 0) && tamd_dev_zero(stepper->d_stats, 4 * sizeof(*stepper->d_stats)))
                rc = TURTLE_RETURN_LIBRARY_ERROR;
        /* every tile resident: the whole walk in one launch, the rays' state in
         * registers (k_walk); else generation by generation, each in rounds over the
         * rays that wait for a tile (TURTLE_AMD_WALK=steps: that form always) */
        static int by_steps = -1;
        if (by_steps < 0) {
                const char * env = getenv("TURTLE_AMD_WALK");
                by_steps = ((env != NULL) && (strcmp(env, "steps") == 0)) ? 1 : 0;
        }
        if ((rc == 0) && !by_steps && !stepper_is_paged(stepper) && (n_steps > 0)) {
                rc = stepper_resident(stepper, &walk_resident, &a);
                n_steps = 0;
        }
        for (k = 0; (rc == 0) && (k < n_steps); k++) {
                a.stream = (unsigned long long)(first_step + k);
                rc = stepper_rounds(stepper, n, &walk_round, &a);
        }
        if (rc != 0) return RAISE_ROUNDS(stepper, rc);
        if (tamd_stage_close(&st)) return TAMD_RAISE_DEVICE();
        return TURTLE_RETURN_SUCCESS;
}

/* A walk, step by step, with the least state between the calls: `next` (the tentative length of
 * the next step) and `index` are all a step resumes from [ref stepper.c:708-710, :799-813]. */
enum turtle_return turtle_stepper_walk_n(struct turtle_stepper * stepper, long n, double * position,
    const double * direction, double * next, double * step, int * index, int space)
{
        TAMD_ERROR_INIT(&turtle_stepper_walk_n);
        if (next == NULL) return TAMD_RAISE(TURTLE_RETURN_BAD_ADDRESS, "invalid null argument");
        return step_n(&error_, stepper, n, position, direction, NULL, NULL, next, NULL, step, index,
            TAMD_STEP_COMPACT | ((direction != NULL) ? TURTLE_AMD_STEP_RESUME : 0), space);
}

enum turtle_return turtle_stepper_step_n(struct turtle_stepper * stepper, long n,
    double * position, const double * direction, double * latitude, double * longitude,
    double * altitude, double * elevation, double * step, int * index, int flags,
    int space)
{
        TAMD_ERROR_INIT(&turtle_stepper_step_n);
        return step_n(&error_, stepper, n, position, direction, latitude, longitude,
            altitude, elevation, step, index, flags, space);
}

struct trace_args {
        long n;
        void *pos, *dir, *index, *length, *n_steps;
        int max_steps, flags, scratch;
};

static int trace_round(struct turtle_stepper * stepper, struct tamd_paging pg, int round, void * p)
{
        struct trace_args * a = p;
        (void)round;
        struct tamd_trace_room room;
        tamd_trace_room_layout(&room, a->n);
        pg.tentative = a->scratch ? TAMD_ROOM_AT(double, stepper->d_room, room.tentative) : NULL;
        /* the lists of the passes; the packed media of the crossings hold 16 bits each */
        const int listed = a->scratch && (stepper->n_layers < 65000) && (stepper->n_data < 65000);
        return tamd_k_trace(stepper->view, a->n, a->pos, a->dir, a->max_steps, a->index, a->length,
            a->n_steps, a->flags, listed ? stepper->d_room : NULL, pg, stepper->d_stats,
            stepper->d_stats + TAMD_STATS_QUEUE);
}

enum turtle_return turtle_stepper_trace_n(struct turtle_stepper * stepper, long n,
    double * position, const double * direction, int max_steps, int * index,
    double * length, int * n_steps, int flags, int space)
{
        TAMD_ERROR_INIT(&turtle_stepper_trace_n);
        if ((position == NULL) || (direction == NULL) || (index == NULL))
                return TAMD_RAISE(TURTLE_RETURN_BAD_ADDRESS, "invalid null argument");
        struct trace_args args = { n, NULL, NULL, NULL, NULL, NULL, max_steps, flags, 0 };
        args.scratch = (tamd_stepper_scratch(stepper, n) == 0);
        if (!args.scratch && (stepper->room_capacity < 0)) return TAMD_RAISE_DEVICE();
        struct tamd_stage st = { 0 };
        const size_t nb = (size_t)n * sizeof(double);
        tamd_stage_add(&st, position, 3 * nb, TAMD_INOUT, &args.pos);
        tamd_stage_add(&st, direction, 3 * nb, TAMD_IN, &args.dir);
        tamd_stage_add(&st, index, 2 * n * sizeof(int),
            (flags & TURTLE_AMD_TRACE_RESUME) ? TAMD_INOUT : TAMD_OUT, &args.index);
        tamd_stage_add(&st, length, nb, TAMD_OUT, &args.length);
        tamd_stage_add(&st, n_steps, n * sizeof(int), TAMD_OUT, &args.n_steps);
        if (tamd_stage_open(&st, space)) return TAMD_RAISE_DEVICE();
        /* a ray that waits for a tile keeps its path length and step count in
         * these arrays, and so does a ray handed from pass to pass: they exist
         * even if the caller has none -- which outputs a caller asks for changes
         * neither the kernels that run nor a bit of the others */
        if (stepper_is_paged(stepper) && !args.scratch)
                return TAMD_RAISE(TURTLE_RETURN_MEMORY_ERROR,
                    "a batch this large cannot run over stacks with tiles left to page in");
        if (args.scratch && (n > 0)) { /* (in place of the NULL of an array that is not brought back) */
                struct tamd_trace_room room;
                tamd_trace_room_layout(&room, n);
                if (args.length == NULL) args.length = TAMD_ROOM_AT(double, stepper->d_room, room.own_length);
                if (args.n_steps == NULL) args.n_steps = TAMD_ROOM_AT(int, stepper->d_room, room.own_n_steps);
        }
        const int rc = stepper_rounds(stepper, n, &trace_round, &args);
        if (rc != 0) return RAISE_ROUNDS(stepper, rc);
        if (tamd_stage_close(&st)) return TAMD_RAISE_DEVICE();
        return TURTLE_RETURN_SUCCESS;
}

/* ---- lines of sight --------------------------------------------------------- */

int turtle_amd_stepper_media(const struct turtle_stepper * stepper) { return stepper->n_layers + 1; }

struct traverse_args {
        long n;
        void *pos, *dir, *alt, *elev, *step, *live;
};

static int traverse_start_round(struct turtle_stepper * stepper, struct tamd_paging pg, int round, void * p)
{
        struct traverse_args * a = p;
        (void)round;
        return tamd_k_step(stepper->view, a->n, a->pos, NULL, NULL, NULL, a->alt, a->elev, NULL,
            a->live, 0, pg);
}

static int traverse_round(struct turtle_stepper * stepper, struct tamd_paging pg, int round, void * p)
{
        struct traverse_args * a = p;
        (void)round;
        double * cross_ds;
        int * const cross_ray = stepper_cross_list(stepper, a->n, &cross_ds);
        return tamd_k_step_live(stepper->view, a->n, a->pos, a->dir, a->alt, a->elev, a->step, a->live,
            cross_ray, cross_ds, pg, stepper->d_stats + TAMD_STATS_STEPS, stepper->d_stats + TAMD_STATS_QUEUE);
}

static void * traverse_piece(char * block, size_t * used, size_t bytes)
{
        void * piece = block + *used;
        *used += ((bytes + 255) / 256) * 256;
        return piece;
}

/* Over paged stacks: generation by generation over the step kernels, each in rounds over the rays
 * that wait for a tile (as scatter_n), the sums kept by k_traverse_gen.  The same arithmetic on the
 * same values as k_traverse in STRICT: the same bits. */
static int traverse_paged(struct turtle_stepper * stepper, long n, double * pos, const double * dir,
    double ceiling, int max_steps, int * index, double * length, int * n_steps, int * n_cross,
    const struct tamd_crossings * rec)
{
        /* the sample state between generations, the counts the caller may not want and, recording
         * crossings, the running totals */
        const size_t nb = (size_t)n * sizeof(double), ni = (size_t)n * sizeof(int);
        const size_t bytes = (4 + (rec != NULL)) * nb + 5 * ni + 4 * sizeof(unsigned long long) + 8 * 256;
        char * block;
        if (tamd_dev_malloc((void **)&block, bytes)) return TURTLE_RETURN_LIBRARY_ERROR;
        size_t used = 0;
        struct traverse_args a = { n, pos, (void *)dir, NULL, NULL, NULL, NULL };
        a.alt = traverse_piece(block, &used, nb);
        a.elev = traverse_piece(block, &used, 2 * nb);
        a.step = traverse_piece(block, &used, nb);
        a.live = traverse_piece(block, &used, 2 * ni);
        int * medium = traverse_piece(block, &used, ni);
        int * own = traverse_piece(block, &used, 2 * ni);
        unsigned long long * counters = traverse_piece(block, &used, 4 * sizeof(unsigned long long));
        double * total = (rec != NULL) ? traverse_piece(block, &used, nb) : NULL;
        if (n_steps == NULL) n_steps = own;
        if (n_cross == NULL) n_cross = own + n;
        /* counters: [0, 4) k_traverse_gen's; the step kernels' stats are at d_stats + TAMD_STATS_STEPS */
        int rc = stepper_rounds(stepper, n, &traverse_start_round, &a);
        int rounds = stepper->last_rounds; /* (turtle_amd_stepper_rounds: the most a generation took) */
        if ((rc == 0) && (tamd_dev_zero(counters, 4 * sizeof(*counters)) ||
                             tamd_dev_zero(stepper->d_stats + TAMD_STATS_STEPS, 4 * sizeof(*stepper->d_stats)) ||
                             ((total != NULL) && tamd_dev_zero(total, nb)) ||
                             tamd_k_traverse_gen(n, 1, a.alt, NULL, a.live, medium, index, length,
                                 n_steps, n_cross, ceiling, max_steps, counters)))
                rc = TURTLE_RETURN_LIBRARY_ERROR;
        unsigned long long c[4] = { 0, 0, 0, 0 };
        while (rc == 0) { /* (a generation ends a ray or takes a step of it: max_steps bounds the loop) */
                if (tamd_dev_d2h(c, counters, sizeof(c))) {
                        rc = TURTLE_RETURN_LIBRARY_ERROR;
                        break;
                }
                if (c[3] == 0) break; /* no ray left live */
                if (tamd_dev_zero(counters + 3, sizeof(*counters))) {
                        rc = TURTLE_RETURN_LIBRARY_ERROR;
                        break;
                }
                rc = stepper_rounds(stepper, n, &traverse_round, &a);
                if (stepper->last_rounds > rounds) rounds = stepper->last_rounds;
                if ((rc == 0) && (total != NULL) &&
                    tamd_k_crossings_gen(n, a.pos, a.step, a.live, medium, n_cross, total, *rec))
                        rc = TURTLE_RETURN_LIBRARY_ERROR;
                if ((rc == 0) && tamd_k_traverse_gen(n, 0, a.alt, a.step, a.live, medium, index, length,
                                     n_steps, n_cross, ceiling, max_steps, counters))
                        rc = TURTLE_RETURN_LIBRARY_ERROR;
        }
        /* turtle_stepper_trace_stats: rays, steps, samples (the origins' and the step kernels'),
         * rays stopped by max_steps */
        unsigned long long taken[4];
        if ((rc == 0) && tamd_dev_d2h(taken, stepper->d_stats + TAMD_STATS_STEPS, sizeof(taken)))
                rc = TURTLE_RETURN_LIBRARY_ERROR;
        if (rc == 0) {
                const unsigned long long stats[4] = { c[0], c[1], (unsigned long long)n + taken[2], c[2] };
                if (tamd_dev_h2d(stepper->d_stats, stats, sizeof(stats))) rc = TURTLE_RETURN_LIBRARY_ERROR;
        }
        stepper->last_rounds = rounds;
        tamd_dev_sync();
        tamd_dev_free(block);
        return rc;
}

struct sight_args {
        long n;
        void *pos, *dir, *index, *length, *n_steps, *n_cross, *point, *distance, *media;
        double ceiling;
        int max_steps;
        const struct tamd_crossings * rec; /* the three arrays above, or NULL */
};

static int sight_resident(struct turtle_stepper * stepper, struct tamd_paging pg, int round, void * p)
{
        struct sight_args * a = p;
        (void)pg, (void)round;
        return tamd_k_traverse(stepper->view, a->n, a->pos, a->dir, a->ceiling, a->max_steps, a->index,
            a->length, a->n_steps, a->n_cross, a->rec, stepper->d_stats, stepper->d_stats + TAMD_STATS_QUEUE);
}

/* turtle_stepper_traverse_n and, rec != NULL (the caller's arrays), turtle_stepper_crossings_n */
static enum turtle_return traverse_n(struct tamd_error * error, struct turtle_stepper * stepper, long n,
    double * position, const double * direction, double altitude_max, int max_steps, int * index,
    double * length, int * n_steps, int * n_crossings, const struct tamd_crossings * rec, int space)
{
        struct tamd_error error_ = *error;
        if ((position == NULL) || (direction == NULL) || (index == NULL))
                return TAMD_RAISE(TURTLE_RETURN_BAD_ADDRESS, "invalid null argument");
        if (max_steps < 0) return TAMD_RAISE(TURTLE_RETURN_DOMAIN_ERROR, "invalid input parameter(s)");
        if (n <= 0) return TURTLE_RETURN_SUCCESS;
        int rc = FLATTEN(stepper);
        if (rc != 0) return RAISE_ROUNDS(stepper, rc);
        const int paged = stepper_is_paged(stepper);
        if (paged && (tamd_stepper_scratch(stepper, n) != 0)) {
                if (stepper->room_capacity < 0) return TAMD_RAISE_DEVICE();
                return TAMD_RAISE(TURTLE_RETURN_MEMORY_ERROR, "batch too large");
        }
        const long media = stepper->n_layers + 1;
        struct tamd_stage st = { 0 };
        struct sight_args a = { n, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, altitude_max,
                max_steps, NULL };
        const size_t nb = (size_t)n * sizeof(double), ni = (size_t)n * sizeof(int);
        const size_t slots = (rec != NULL) ? (size_t)rec->capacity : 0; /* (of n rays each) */
        tamd_stage_add(&st, position, 3 * nb, TAMD_INOUT, &a.pos);
        tamd_stage_add(&st, direction, 3 * nb, TAMD_IN, &a.dir);
        tamd_stage_add(&st, index, 2 * ni, TAMD_OUT, &a.index);
        tamd_stage_add(&st, length, media * nb, TAMD_OUT, &a.length);
        tamd_stage_add(&st, n_steps, ni, TAMD_OUT, &a.n_steps);
        tamd_stage_add(&st, n_crossings, ni, TAMD_OUT, &a.n_cross);
        if (rec != NULL) {
                tamd_stage_add(&st, rec->point, 3 * slots * nb, TAMD_OUT, &a.point);
                tamd_stage_add(&st, rec->distance, slots * nb, TAMD_OUT, &a.distance);
                tamd_stage_add(&st, rec->media, 2 * slots * ni, TAMD_OUT, &a.media);
        }
        if (tamd_stage_open(&st, space)) return TAMD_RAISE_DEVICE();
        const struct tamd_crossings drec = { a.point, a.distance, a.media, (int)slots };
        if (rec != NULL) a.rec = &drec;
        /* the sums are added to where they stand: they start from zero; and the slots past a ray's
         * crossings are zero (media {0, 0}) */
        if ((a.length != NULL) && tamd_dev_zero(a.length, media * nb)) return TAMD_RAISE_DEVICE();
        if ((slots > 0) && (((a.point != NULL) && tamd_dev_zero(a.point, 3 * slots * nb)) ||
                               ((a.distance != NULL) && tamd_dev_zero(a.distance, slots * nb)) ||
                               ((a.media != NULL) && tamd_dev_zero(a.media, 2 * slots * ni))))
                return TAMD_RAISE_DEVICE();
        if (!paged) { /* every tile resident: the whole traverse in one launch */
                rc = stepper_resident(stepper, &sight_resident, &a);
                stepper->last_rounds = 1;
        } else
                rc = traverse_paged(stepper, n, a.pos, a.dir, altitude_max, max_steps, a.index, a.length,
                    a.n_steps, a.n_cross, a.rec);
        if (rc != 0) return RAISE_ROUNDS(stepper, rc);
        if (tamd_stage_close(&st)) return TAMD_RAISE_DEVICE();
        return TURTLE_RETURN_SUCCESS;
}

enum turtle_return turtle_stepper_traverse_n(struct turtle_stepper * stepper, long n,
    double * position, const double * direction, double altitude_max, int max_steps, int * index,
    double * length, int * n_steps, int * n_crossings, int space)
{
        TAMD_ERROR_INIT(&turtle_stepper_traverse_n);
        return traverse_n(&error_, stepper, n, position, direction, altitude_max, max_steps, index,
            length, n_steps, n_crossings, NULL, space);
}

enum turtle_return turtle_stepper_crossings_n(struct turtle_stepper * stepper, long n,
    double * position, const double * direction, double altitude_max, int max_steps, int * index,
    double * length, int * n_steps, int * n_crossings, int capacity, double * point,
    double * distance, int * media, int space)
{
        TAMD_ERROR_INIT(&turtle_stepper_crossings_n);
        if (n_crossings == NULL) return TAMD_RAISE(TURTLE_RETURN_BAD_ADDRESS, "invalid null argument");
        if (capacity < 0) return TAMD_RAISE(TURTLE_RETURN_DOMAIN_ERROR, "invalid input parameter(s)");
        const struct tamd_crossings rec = { point, distance, media, capacity };
        return traverse_n(&error_, stepper, n, position, direction, altitude_max, max_steps, index,
            length, n_steps, n_crossings, &rec, space);
}

/* turtle_stepper_advance_n, turtle_stepper_advance_exp_n (scale_height, or NULL) and
 * turtle_stepper_advance_grid_n (grid, or NULL; its voxels staged like any array): resident tiles
 * only (a cut needs the position its step began at, which the generation kernels overwrite): one
 * launch through stepper_resident, and sight_run's closing sequence over a stage of its own. */
struct advance_args {
        struct tamd_stage stage;
        int paged; /* out: a tile was not resident when the tables were made current */
        long n;
        void *pos, *dir, *density, *scale_height, *voxels, *budget, *distance_max, *index, *depth, *distance, *n_steps, *status;
        const struct turtle_amd_grid * grid; /* or NULL */
        double ceiling;
        int max_steps;
};

static int advance_resident(struct turtle_stepper * stepper, struct tamd_paging pg, int round, void * p)
{
        struct advance_args * a = p;
        (void)pg, (void)round;
        if ((a->paged = stepper_is_paged(stepper))) return 0; /* (a tile another thread took meanwhile) */
        struct turtle_amd_grid_view view, *grid = NULL;
        if (a->grid != NULL) { /* the caller's box, its voxels where the stage put them */
                memcpy(view.origin, a->grid->origin, sizeof(view.origin));
                memcpy(view.axis, a->grid->axis, sizeof(view.axis));
                memcpy(view.size, a->grid->size, sizeof(view.size));
                memcpy(view.n, a->grid->n, sizeof(view.n));
                view.medium = a->grid->medium;
                view.density = a->voxels;
                grid = &view;
        }
        return tamd_k_advance(stepper->view, a->n, a->pos, a->dir, a->density, a->scale_height, grid, a->budget,
            a->distance_max, a->ceiling, a->max_steps, a->index, a->depth, a->distance, a->n_steps, a->status, stepper->d_stats,
            stepper->d_stats + TAMD_STATS_QUEUE);
}

static enum turtle_return advance_n(const struct tamd_error * error, struct turtle_stepper * stepper, long n,
    double * position, const double * direction, const double * density, const double * scale_height,
    const struct turtle_amd_grid * grid, const double * budget, const double * distance_max,
    double altitude_max, int max_steps, int * index, double * depth, double * distance, int * n_steps,
    int * status, int space)
{
        struct tamd_error error_ = *error;
        if ((stepper == NULL) || (position == NULL) || (direction == NULL) || (density == NULL) ||
            (budget == NULL) || (index == NULL) || (status == NULL))
                return TAMD_RAISE(TURTLE_RETURN_BAD_ADDRESS, "invalid null argument");
        if ((grid != NULL) && (grid->density == NULL))
                return TAMD_RAISE(TURTLE_RETURN_BAD_ADDRESS, "invalid null argument");
        if (max_steps < 0) return TAMD_RAISE(TURTLE_RETURN_DOMAIN_ERROR, "invalid input parameter(s)");
        if ((space != TURTLE_AMD_HOST) && (space != TURTLE_AMD_DEVICE))
                return TAMD_RAISE(TURTLE_RETURN_DOMAIN_ERROR, "invalid space (%d)", space);
        size_t voxels = 0;
        if (grid != NULL) {
                double count = 1.;
                int i;
                for (i = 0; i < 3; i++) {
                        if (grid->n[i] < 1)
                                return TAMD_RAISE(TURTLE_RETURN_DOMAIN_ERROR, "invalid grid: n[%d] = %d", i, grid->n[i]);
                        if (!(isfinite(grid->size[i]) && (grid->size[i] > 0.)))
                                return TAMD_RAISE(TURTLE_RETURN_DOMAIN_ERROR, "invalid grid: size[%d] = %g", i, grid->size[i]);
                        count *= grid->n[i];
                }
                if (count > INT_MAX)
                        return TAMD_RAISE(TURTLE_RETURN_DOMAIN_ERROR, "invalid grid: %d x %d x %d voxels are beyond an int",
                            grid->n[0], grid->n[1], grid->n[2]);
                if ((grid->medium < 0) || (grid->medium > stepper->n_layers))
                        return TAMD_RAISE(TURTLE_RETURN_DOMAIN_ERROR, "invalid grid: medium %d of %d", grid->medium,
                            stepper->n_layers + 1);
                voxels = (size_t)count;
        }
        if (n <= 0) return TURTLE_RETURN_SUCCESS;
        const enum turtle_return loaded =
            stepper_load_all(stepper, &error_, turtle_error_function(error_.function), "advances over");
        if (loaded != TURTLE_RETURN_SUCCESS) return loaded;
        struct advance_args a = { 0 };
        struct tamd_stage * st = &a.stage;
        a.n = n, a.ceiling = altitude_max, a.max_steps = max_steps, a.grid = grid;
        const size_t nb = (size_t)n * sizeof(double), ni = (size_t)n * sizeof(int);
        const size_t media = (size_t)stepper->n_layers + 1;
        tamd_stage_add(st, position, 3 * nb, TAMD_INOUT, &a.pos);
        tamd_stage_add(st, direction, 3 * nb, TAMD_IN, &a.dir);
        tamd_stage_add(st, density, media * sizeof(double), TAMD_IN, &a.density);
        tamd_stage_add(st, scale_height, media * sizeof(double), TAMD_IN, &a.scale_height);
        tamd_stage_add(st, (grid != NULL) ? grid->density : NULL, voxels * sizeof(double), TAMD_IN, &a.voxels);
        tamd_stage_add(st, budget, nb, TAMD_IN, &a.budget);
        tamd_stage_add(st, distance_max, nb, TAMD_IN, &a.distance_max);
        tamd_stage_add(st, index, 2 * ni, TAMD_OUT, &a.index);
        tamd_stage_add(st, depth, nb, TAMD_OUT, &a.depth);
        tamd_stage_add(st, distance, nb, TAMD_OUT, &a.distance);
        tamd_stage_add(st, n_steps, ni, TAMD_OUT, &a.n_steps);
        tamd_stage_add(st, status, ni, TAMD_OUT, &a.status);
        if (tamd_stage_open(st, space)) return TAMD_RAISE_DEVICE();
        const int rc = stepper_resident(stepper, &advance_resident, &a);
        stepper->last_rounds = 1;
        if (rc != 0) return RAISE_ROUNDS(stepper, rc);
        if (a.paged)
                return TAMD_RAISE(TURTLE_RETURN_DOMAIN_ERROR, "a tile left its stack while the call was made: try again");
        if (tamd_stage_close(st)) return TAMD_RAISE_DEVICE();
        return TURTLE_RETURN_SUCCESS;
}

enum turtle_return turtle_stepper_advance_n(struct turtle_stepper * stepper, long n, double * position,
    const double * direction, const double * density, const double * budget, const double * distance_max,
    double altitude_max, int max_steps, int * index, double * depth, double * distance, int * n_steps,
    int * status, int space)
{
        TAMD_ERROR_INIT(&turtle_stepper_advance_n);
        return advance_n(&error_, stepper, n, position, direction, density, NULL, NULL, budget, distance_max,
            altitude_max, max_steps, index, depth, distance, n_steps, status, space);
}

enum turtle_return turtle_stepper_advance_exp_n(struct turtle_stepper * stepper, long n, double * position,
    const double * direction, const double * density, const double * scale_height, const double * budget,
    const double * distance_max, double altitude_max, int max_steps, int * index, double * depth,
    double * distance, int * n_steps, int * status, int space)
{
        TAMD_ERROR_INIT(&turtle_stepper_advance_exp_n);
        return advance_n(&error_, stepper, n, position, direction, density, scale_height, NULL, budget,
            distance_max, altitude_max, max_steps, index, depth, distance, n_steps, status, space);
}

enum turtle_return turtle_stepper_advance_grid_n(struct turtle_stepper * stepper, long n, double * position,
    const double * direction, const double * density, const struct turtle_amd_grid * grid,
    const double * budget, const double * distance_max, double altitude_max, int max_steps, int * index,
    double * depth, double * distance, int * n_steps, int * status, int space)
{
        TAMD_ERROR_INIT(&turtle_stepper_advance_grid_n);
        return advance_n(&error_, stepper, n, position, direction, density, NULL, grid, budget, distance_max,
            altitude_max, max_steps, index, depth, distance, n_steps, status, space);
}

/* the east, north, up frame of turtle_ecef_from_horizontal at (latitude, longitude): host arithmetic */
void turtle_amd_grid_enu(struct turtle_amd_grid * grid, double latitude, double longitude, double height,
    double east0, double north0, double up0)
{
        int i;
        tamd_h_from_horizontal(latitude, longitude, 90., 0., grid->axis[0]);
        tamd_h_from_horizontal(latitude, longitude, 0., 0., grid->axis[1]);
        tamd_h_from_horizontal(latitude, longitude, 0., 90., grid->axis[2]);
        tamd_h_from_geodetic(latitude, longitude, height, grid->origin);
        for (i = 0; i < 3; i++)
                grid->origin[i] += east0 * grid->axis[0][i] + north0 * grid->axis[1][i] + up0 * grid->axis[2][i];
}

int turtle_amd_stepper_rounds(const struct turtle_stepper * stepper) { return stepper->last_rounds; }

enum turtle_return turtle_stepper_trace_stats(
    struct turtle_stepper * stepper, unsigned long long stats[4])
{
        TAMD_ERROR_INIT(&turtle_stepper_trace_stats);
        memset(stats, 0, 4 * sizeof(*stats));
        if (stepper->d_stats == NULL) return TURTLE_RETURN_SUCCESS;
        if (tamd_dev_d2h(stats, stepper->d_stats, 4 * sizeof(*stats)))
                return TAMD_RAISE_DEVICE();
        return TURTLE_RETURN_SUCCESS;
}

/* ---- scalar entry points: the batch ones with n = 1 ------------------------ */

/* [ref stepper.c:780-875].  Outside every data with index == NULL is the one
 * case the reference raises [ref stepper.c:751-754, :870-873]. */
enum turtle_return turtle_stepper_step(struct turtle_stepper * stepper, double * position,
    const double * direction, double * latitude, double * longitude, double * altitude,
    double * elevation, double * step, int * index)
{
        TAMD_ERROR_INIT(&turtle_stepper_step);
        if (tamd_scalar_on_host() && tamd_h_stepper_takes(stepper)) { /* (the caller's option: scalar.c) */
                const int rc = tamd_h_stepper_step(stepper, position, direction, latitude, longitude,
                    altitude, elevation, step, index, stepper->message, sizeof(stepper->message));
                if (rc == TURTLE_RETURN_DOMAIN_ERROR) return TAMD_RAISE(TURTLE_RETURN_DOMAIN_ERROR, "no valid data");
                if (rc != 0) return TAMD_RAISE((enum turtle_return)rc, "%s", stepper->message);
                return TURTLE_RETURN_SUCCESS;
        }
        int idx[2] = { -1, -1 };
        const enum turtle_return rc = step_n(&error_, stepper, 1, position, direction,
            latitude, longitude, altitude, elevation, step, idx, 0, TURTLE_AMD_HOST);
        if (rc != TURTLE_RETURN_SUCCESS) return rc;
        if (index != NULL) {
                index[0] = idx[0], index[1] = idx[1];
        } else if (idx[0] < 0)
                return TAMD_RAISE(TURTLE_RETURN_DOMAIN_ERROR, "no valid data");
        return TURTLE_RETURN_SUCCESS;
}

/* [ref stepper.c:877-931] */
enum turtle_return turtle_stepper_position(struct turtle_stepper * stepper, double latitude,
    double longitude, double height, int layer_index, double * position, int * data_index)
{
        TAMD_ERROR_INIT(&turtle_stepper_position);
        if ((layer_index < 0) || (layer_index >= stepper->n_layers))
                return TAMD_RAISE(TURTLE_RETURN_DOMAIN_ERROR, "no valid data");
        int di = -1;
        if (tamd_scalar_on_host() && tamd_h_stepper_takes(stepper)) { /* (the caller's option: scalar.c) */
                const int rc = tamd_h_stepper_position(stepper, latitude, longitude, height, layer_index,
                    position, &di, stepper->message, sizeof(stepper->message));
                if (rc != 0) return TAMD_RAISE((enum turtle_return)rc, "%s", stepper->message);
                if (data_index != NULL)
                        *data_index = di;
                else if (di < 0)
                        return TAMD_RAISE(TURTLE_RETURN_DOMAIN_ERROR, "no valid data");
                return TURTLE_RETURN_SUCCESS;
        }
        const enum turtle_return rc = turtle_stepper_position_n(stepper, 1, &latitude,
            &longitude, &height, layer_index, position, &di, TURTLE_AMD_HOST);
        if (rc != TURTLE_RETURN_SUCCESS) return rc;
        if (data_index != NULL)
                *data_index = di;
        else if (di < 0)
                return TAMD_RAISE(TURTLE_RETURN_DOMAIN_ERROR, "no valid data");
        return TURTLE_RETURN_SUCCESS;
}
