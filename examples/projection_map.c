/*
 * projection_map.c -- a local projected map built from global data: the
 * reference's examples/example-projection.c, with its loop over the nodes
 * (turtle_map_node, turtle_projection_unproject, turtle_stack_elevation,
 * turtle_map_fill) replaced by one turtle_map_resample call.
 *
 * The map is the example's: Lambert 93 (RGF93), 201 x 201 nodes, 6 km a side
 * around the Col de Ceyssat, Auvergne, z in [500, 1500] m.  The stack is the
 * folder of global tiles given on the command line (default share/topography;
 * it needs N45E002), the map is dumped to the PNG given next (default
 * share/data/pdd-30m.png).
 *
 * Unlike the example, a node that falls outside the data keeps its value (here
 * the z0 of a new map) instead of getting 0, and an elevation outside the map's
 * span is clamped to it (TURTLE_AMD_RESAMPLE_CLAMP) instead of failing.
 *
 *   cc -Iinclude examples/projection_map.c -Lturtle_amd -lturtle_amd \
 *      -Wl,-rpath,$PWD/turtle_amd -o projection_map
 */
#include <stdio.h>
#include <stdlib.h>

#include "turtle.h"

static struct turtle_stack * stack = NULL;
static struct turtle_map * map = NULL;

static void exit_gracefully(int rc)
{
        turtle_map_destroy(&map);
        turtle_stack_destroy(&stack);
        exit(rc);
}

static void handle_error(enum turtle_return code, turtle_function_t * function, const char * message)
{
        (void)code;
        (void)function;
        fprintf(stderr, "A TURTLE library error occurred:\n%s\n", message);
        exit_gracefully(EXIT_FAILURE);
}

int main(int argc, char * argv[])
{
        const char * topography = (argc > 1) ? argv[1] : "share/topography";
        const char * output = (argc > 2) ? argv[2] : "share/data/pdd-30m.png";
        turtle_error_handler_set(&handle_error);

        /* the stack of global elevation data */
        turtle_stack_create(&stack, topography, 0, NULL, NULL);

        /* the RGF93 local projection map, centred on the Auberge des Gros Manaux */
        struct turtle_map_info info = { .nx = 201,
                .ny = 201,
                .x = { 693530.7, 699530.7 },
                .y = { 6515284.5, 6521284.5 },
                .z = { 500., 1500. } };
        turtle_map_create(&map, &info, "Lambert 93");

        /* every node from the global data, in one call */
        long outside, clamped;
        turtle_map_resample(map, stack, NULL, TURTLE_AMD_RESAMPLE_CLAMP, &outside, &clamped);
        printf("%d nodes: %ld outside the data, %ld clamped to the span\n", info.nx * info.ny,
            outside, clamped);

        turtle_map_dump(map, output);
        exit_gracefully(EXIT_SUCCESS);
}
