/*
 * stage.c -- moves the arrays of a batch call between the caller's memory and
 * HBM.  An entry point DECLARES each array once (tamd_stage_add: user pointer,
 * bytes, direction), OPENS the stage before its launches and CLOSES it after.
 * TURTLE_AMD_DEVICE arrays are used in place (nothing is copied and the call
 * stays asynchronous); TURTLE_AMD_HOST arrays go through a grow-only device
 * arena of the calling thread and the call completes before it returns.
 *
 * Small HOST calls -- the scalar drop-in entry points above all: a dozen doubles
 * in, a dozen out -- go PACKED: the arrays are copied into a pinned buffer of the
 * thread and from there to the arena by asynchronous copies on the thread's
 * stream (ordered before the kernels, nothing to wait for), the outputs come back
 * the same way, and the ONE synchronisation of the call is in tamd_stage_close.
 * (Copy by copy, each with its own wait, a scalar turtle_stepper_step spent most
 * of its 20-40 us waiting.)
 */
#include "host.h"

#include <stdio.h>
#include <string.h>

#define TAMD_PACKED_BYTES ((size_t)256 * 1024)

static size_t round_up(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

void tamd_stage_add(struct tamd_stage * st, const void * user, size_t bytes, int dir, void ** dev)
{
        if (st->n >= TAMD_STAGE_ARRAYS) {
                /* a mistake in the entry point, not of the device: said here, where it is made (the
                 * device layer owns the text of a "device error"); the open then fails */
                if (st->n == TAMD_STAGE_ARRAYS)
                        fprintf(stderr, "turtle_amd: a batch call declares more than %d arrays "
                                        "(host.h: TAMD_STAGE_ARRAYS)\n", TAMD_STAGE_ARRAYS);
                st->n = TAMD_STAGE_ARRAYS + 1;
                return;
        }
        st->array[st->n].user = (void *)user, st->array[st->n].bytes = bytes;
        st->array[st->n].dir = dir, st->array[st->n].dev = dev;
        st->n++;
}

/* does the array have a piece of the arena?  (a table has one in either space, and so has a
 * scratch piece, which has no array of the user's behind it) */
static int staged(const struct tamd_stage * st, const struct tamd_stage_array * a)
{
        if (a->dir == TAMD_SCRATCH) return 1;
        return (a->user != NULL) && ((st->space != TURTLE_AMD_DEVICE) || (a->dir == TAMD_TABLE));
}

/* NULL once the buffer is full, and the copy then goes by itself, waited for.  On purpose, and
 * next to never: the packed test leaves room for 16 roundings, 12 arrays in and the span of 12
 * back can take 24, so only a call within 2 KiB of the threshold with most arrays both ways. */
static char * pinned_piece(struct tamd_stage * st, size_t bytes)
{
        if (!st->packed || (st->pinned_used + round_up(bytes) > TAMD_PACKED_BYTES)) return NULL;
        char * piece = st->pinned + st->pinned_used;
        st->pinned_used += round_up(bytes);
        return piece;
}

int tamd_stage_open(struct tamd_stage * st, int space)
{
        st->space = space;
        st->packed = 0, st->wait = 0, st->pinned = NULL, st->pinned_used = 0;
        if ((st->n > TAMD_STAGE_ARRAYS) || tamd_dev_init()) return 1;
        struct tamd_stage_array * a;
        size_t raw = 0, arena = 0;
        for (a = st->array; a < st->array + st->n; a++) {
                *a->dev = a->user;
                raw += a->bytes;
                if (!staged(st, a)) continue;
                arena += round_up(a->bytes);
                st->wait = 1;
        }
        if (space != TURTLE_AMD_DEVICE) st->wait = 1;
        if (!st->wait) return 0;
        /* size the arena once, before any piece is handed out: it cannot grow under them
         * (never nothing, so that an array of no bytes still gets an address) */
        void * all;
        tamd_scratch_reset();
        if (tamd_scratch_get(&all, (arena > 0) ? arena : 256)) return 1;
        tamd_scratch_reset();
        if ((space != TURTLE_AMD_DEVICE) && (2 * raw + 16 * 256 <= TAMD_PACKED_BYTES) &&
            (tamd_dev_pinned((void **)&st->pinned, TAMD_PACKED_BYTES) == 0))
                st->packed = 1;
        for (a = st->array; a < st->array + st->n; a++) {
                if (!staged(st, a)) continue;
                if (tamd_scratch_get(a->dev, a->bytes)) return 1;
                if (!(a->dir & TAMD_IN)) continue;
                char * piece = pinned_piece(st, a->bytes);
                if (piece != NULL) {
                        memcpy(piece, a->user, a->bytes);
                        if (tamd_dev_copy_async(*a->dev, piece, a->bytes, 1)) return 1;
                } else if (tamd_dev_h2d(*a->dev, a->user, a->bytes))
                        return 1;
        }
        return 0;
}

int tamd_stage_close(struct tamd_stage * st)
{
        if (!st->wait) return 0;
        struct tamd_stage_array * a;
        /* the outputs are pieces of one arena: packed, ONE copy of the span they cover */
        const char *lo = NULL, *hi = NULL;
        for (a = st->array; a < st->array + st->n; a++) {
                if (!staged(st, a) || !(a->dir & TAMD_OUT)) continue;
                const char * d = *a->dev;
                if ((lo == NULL) || (d < lo)) lo = d;
                if ((hi == NULL) || (d + a->bytes > hi)) hi = d + a->bytes;
        }
        char * span = (lo != NULL) ? pinned_piece(st, (size_t)(hi - lo)) : NULL;
        if ((span != NULL) && (tamd_dev_copy_async(span, lo, (size_t)(hi - lo), 0) || tamd_dev_sync()))
                return 1;
        for (a = st->array; a < st->array + st->n; a++) {
                if (!staged(st, a) || !(a->dir & TAMD_OUT)) continue;
                if (span != NULL)
                        memcpy(a->user, span + ((const char *)*a->dev - lo), a->bytes);
                else if (tamd_dev_d2h(a->user, *a->dev, a->bytes))
                        return 1;
        }
        /* (copy by copy, or nothing to bring back: what the call queued has still to end) */
        return (span != NULL) ? 0 : tamd_dev_sync();
}
