/*
 * stage_stub.c -- stage.c against a stub of the eight device calls it uses, in host memory:
 * the declared staging of the batch calls (host.h) exercised without a GPU.  The stub's arena
 * refuses to grow once a piece of it is out, as the device layer's does, and every call is
 * counted.  Prints one line of counts per scenario; tests/test_stage_host.py asserts on them.
 *
 *      gcc -std=gnu99 -Iinclude -Iturtle_amd/csrc tests/c/stage_stub.c turtle_amd/csrc/stage.c
 */
#include "host.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* ---- the stub ---------------------------------------------------------------- */
static struct {
        char * arena;
        size_t arena_size, arena_used;
        char * pinned;
        size_t pinned_size;
} dev;
static struct {
        int h2d, d2h, to_device, to_host, syncs, refused;
} count;

static int in_arena(const void * p, size_t bytes)
{
        const char * c = p;
        return (c >= dev.arena) && (c + bytes <= dev.arena + dev.arena_size);
}

const char * tamd_dev_error(void) { return "stub"; }
int tamd_dev_init(void) { return 0; }
void tamd_scratch_reset(void) { dev.arena_used = 0; }

int tamd_scratch_get(void ** ptr, size_t bytes)
{
        *ptr = NULL;
        const size_t need = (bytes + 255) & ~(size_t)255;
        if (dev.arena_used + need > dev.arena_size) {
                if (dev.arena_used != 0) {
                        count.refused++;
                        return 1;
                }
                /* exactly what was asked for: slack would hide a request that is too small */
                free(dev.arena);
                dev.arena = malloc(need ? need : 1);
                dev.arena_size = need;
        }
        *ptr = dev.arena + dev.arena_used;
        dev.arena_used += need;
        return 0;
}

int tamd_dev_pinned(void ** ptr, size_t bytes)
{
        if (bytes > dev.pinned_size) {
                free(dev.pinned);
                dev.pinned = malloc(bytes);
                dev.pinned_size = bytes;
        }
        *ptr = dev.pinned;
        return 0;
}

int tamd_dev_h2d(void * dst, const void * src, size_t bytes)
{
        if (!in_arena(dst, bytes)) return 1;
        memcpy(dst, src, bytes);
        count.h2d++;
        return 0;
}

int tamd_dev_d2h(void * dst, const void * src, size_t bytes)
{
        if (!in_arena(src, bytes)) return 1;
        memcpy(dst, src, bytes);
        count.d2h++;
        return 0;
}

int tamd_dev_copy_async(void * dst, const void * src, size_t bytes, int to_device)
{
        if (!in_arena(to_device ? dst : (void *)src, bytes)) return 1;
        memcpy(dst, src, bytes);
        if (to_device)
                count.to_device++;
        else
                count.to_host++;
        return 0;
}

int tamd_dev_sync(void)
{
        count.syncs++;
        return 0;
}

/* ---- the scenarios ------------------------------------------------------------- */

/* a "kernel": every IN / INOUT array must hold its input; every OUT / INOUT array is written */
#define N_ARRAYS 6
static const int dirs[N_ARRAYS] = { TAMD_IN, TAMD_INOUT, TAMD_OUT, TAMD_OUT, TAMD_IN, TAMD_INOUT };
static const int is_null[N_ARRAYS] = { 0, 0, 0, 1, 1, 0 };

static unsigned char pattern(int array, size_t i, int after) { return (unsigned char)(31 * array + 7 * i + 101 * after); }

static void mixed(const char * name, int space, size_t bytes)
{
        struct tamd_stage st = { 0 };
        unsigned char * user[N_ARRAYS];
        void * d[N_ARRAYS];
        int a, bad = 0, same = 1;
        size_t i;
        memset(&count, 0, sizeof(count));
        for (a = 0; a < N_ARRAYS; a++) {
                user[a] = is_null[a] ? NULL : malloc(bytes + 1);
                for (i = 0; !is_null[a] && (i < bytes); i++) user[a][i] = pattern(a, i, 0);
                tamd_stage_add(&st, user[a], bytes, dirs[a], &d[a]);
        }
        if (tamd_stage_open(&st, space)) bad |= 1;
        for (a = 0; !bad && (a < N_ARRAYS); a++) {
                if (is_null[a]) {
                        if (d[a] != NULL) bad |= 2;
                        continue;
                }
                if (d[a] != (void *)user[a]) same = 0;
                unsigned char * p = d[a];
                if (dirs[a] & TAMD_IN)
                        for (i = 0; i < bytes; i++)
                                if (p[i] != pattern(a, i, 0)) bad |= 4;
                if (dirs[a] & TAMD_OUT)
                        for (i = 0; i < bytes; i++) p[i] = pattern(a, i, 1);
        }
        if (!bad && tamd_stage_close(&st)) bad |= 8;
        for (a = 0; !bad && (a < N_ARRAYS); a++)
                for (i = 0; !is_null[a] && (i < bytes); i++)
                        if (user[a][i] != pattern(a, i, (dirs[a] & TAMD_OUT) != 0)) bad |= 16;
        printf("%s bad=%d same=%d packed=%d h2d=%d d2h=%d to_device=%d to_host=%d syncs=%d refused=%d\n", name,
            bad, same, st.packed, count.h2d, count.d2h, count.to_device, count.to_host, count.syncs, count.refused);
        for (a = 0; a < N_ARRAYS; a++) free(user[a]);
}

/* the most arrays a stage takes, of 1 byte each, on an arena that starts from nothing: the
 * request must cover the 256 bytes every piece takes; one array more fails at the open, before
 * anything is copied */
static void many(void)
{
        struct tamd_stage st = { 0 };
        unsigned char user[TAMD_STAGE_ARRAYS + 1];
        void * d[TAMD_STAGE_ARRAYS + 1];
        int a, bad = 0;
        free(dev.arena);
        dev.arena = NULL, dev.arena_size = 0, dev.arena_used = 0;
        memset(&count, 0, sizeof(count));
        for (a = 0; a < TAMD_STAGE_ARRAYS; a++) {
                user[a] = (unsigned char)a;
                tamd_stage_add(&st, &user[a], 1, TAMD_INOUT, &d[a]);
        }
        if (tamd_stage_open(&st, TURTLE_AMD_HOST)) bad |= 1;
        for (a = 0; !bad && (a < TAMD_STAGE_ARRAYS); a++) {
                if (*(unsigned char *)d[a] != a) bad |= 4;
                *(unsigned char *)d[a] = (unsigned char)(a + 100);
        }
        if (!bad && tamd_stage_close(&st)) bad |= 8;
        for (a = 0; !bad && (a < TAMD_STAGE_ARRAYS); a++)
                if (user[a] != a + 100) bad |= 16;
        const size_t arena = dev.arena_size;
        struct tamd_stage over = { 0 };
        for (a = 0; a < TAMD_STAGE_ARRAYS + 1; a++) tamd_stage_add(&over, &user[a], 1, TAMD_IN, &d[a]);
        const int copies = count.h2d + count.to_device;
        const int over_fails = (tamd_stage_open(&over, TURTLE_AMD_HOST) != 0) && (count.h2d + count.to_device == copies);
        printf("many bad=%d arrays=%d arena=%zu refused=%d to_host=%d syncs=%d over_fails=%d\n", bad,
            TAMD_STAGE_ARRAYS, arena, count.refused, count.to_host, count.syncs, over_fails);
}

/* a table of the library's own: in the arena in either space, and the close then waits */
static void table(const char * name, int space)
{
        struct tamd_stage st = { 0 };
        double blob[5] = { 1., 2., 3., 4., 5. }, x[3] = { 6., 7., 8. }, y[3] = { 0., 0., 0. };
        void *dt, *dx, *dy;
        int bad = 0, i;
        memset(&count, 0, sizeof(count));
        tamd_stage_add(&st, blob, sizeof(blob), TAMD_TABLE, &dt);
        tamd_stage_add(&st, x, sizeof(x), TAMD_IN, &dx);
        tamd_stage_add(&st, y, sizeof(y), TAMD_OUT, &dy);
        if (tamd_stage_open(&st, space)) bad |= 1;
        if (!bad && (!in_arena(dt, sizeof(blob)) || (memcmp(dt, blob, sizeof(blob)) != 0))) bad |= 4;
        for (i = 0; !bad && (i < 3); i++) ((double *)dy)[i] = ((double *)dx)[i] + ((double *)dt)[i];
        if (!bad && tamd_stage_close(&st)) bad |= 8;
        if (!bad && ((y[0] != 7.) || (y[1] != 9.) || (y[2] != 11.))) bad |= 16;
        printf("%s bad=%d same=%d h2d=%d d2h=%d to_device=%d to_host=%d syncs=%d refused=%d\n", name, bad,
            (dx == (void *)x) && (dy == (void *)y), count.h2d, count.d2h, count.to_device, count.to_host, count.syncs,
            count.refused);
}

int main(void)
{
        mixed("device", TURTLE_AMD_DEVICE, 1000);
        mixed("host_small", TURTLE_AMD_HOST, 1000);
        mixed("host_large", TURTLE_AMD_HOST, 100000);
        mixed("host_edge", TURTLE_AMD_HOST, 21504); /* 2 x 6 x 21504 + 16 x 256 = 256 KiB: the last packed size */
        mixed("host_edge1", TURTLE_AMD_HOST, 21505);
        mixed("host_empty", TURTLE_AMD_HOST, 0);
        many();
        table("table_device", TURTLE_AMD_DEVICE);
        table("table_host", TURTLE_AMD_HOST);
        free(dev.arena), free(dev.pinned);
        return 0;
}
