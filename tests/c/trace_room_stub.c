/*
 * trace_room_stub.c -- the layout of a stepper's scratch block (csrc/trace_room.h) for the batch
 * sizes given on the command line: one line per size, every region's offset by name and the
 * block's size.  tests/test_trace_room_host.py asserts on them.  The header is C99 and C++: this
 * file compiles as either.
 *
 *      gcc -std=c99 -Iturtle_amd/csrc tests/c/trace_room_stub.c
 */
#include "trace_room.h"

#include <stdio.h>
#include <stdlib.h>

int main(int argc, char ** argv)
{
        int i;
        for (i = 1; i < argc; i++) {
                const long n = atol(argv[i]);
                struct tamd_trace_room room;
                const size_t bytes = tamd_trace_room_layout(&room, n);
                printf("n=%ld", n);
#define PRINT_REGION(name, size) printf(" " #name "=%zu", room.name);
                TAMD_TRACE_ROOM_REGIONS(PRINT_REGION, n)
#undef PRINT_REGION
                printf(" bytes=%zu\n", room.bytes);
                if (bytes != room.bytes) return 1;
        }
        return 0;
}
