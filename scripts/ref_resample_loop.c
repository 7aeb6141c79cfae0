/*
 * ref_resample_loop.c -- the loop of the reference's examples/example-projection.c, timed: for
 * every node of a map, turtle_map_node, turtle_projection_unproject, turtle_stack_elevation and
 * (inside the data) turtle_map_fill.  Built by scripts/exp_resample.py against any library with
 * the reference's API (include/turtle.h): the reference itself (oracle/_ref/libturtle_ref.so)
 * for the CPU figure.
 *
 *   ref_resample_loop STACK_DIR NX NY X0 X1 Y0 Y1 Z0 Z1 PROJECTION  ->  "nodes outside seconds"
 */
#include <stdio.h>
#include <stdlib.h>
#include <time.h>

#include "turtle.h"

int main(int argc, char * argv[])
{
        if (argc < 11) return EXIT_FAILURE;
        struct turtle_stack * stack;
        if (turtle_stack_create(&stack, argv[1], 0, NULL, NULL) != TURTLE_RETURN_SUCCESS) return EXIT_FAILURE;
        turtle_stack_load(stack);
        struct turtle_map_info info = { .nx = atoi(argv[2]), .ny = atoi(argv[3]),
                .x = { atof(argv[4]), atof(argv[5]) }, .y = { atof(argv[6]), atof(argv[7]) },
                .z = { atof(argv[8]), atof(argv[9]) } };
        struct turtle_map * map;
        if (turtle_map_create(&map, &info, argv[10]) != TURTLE_RETURN_SUCCESS) return EXIT_FAILURE;
        const struct turtle_projection * projection = turtle_map_projection(map);
        struct timespec t0, t1;
        clock_gettime(CLOCK_MONOTONIC, &t0);
        long outside = 0;
        int ix, iy;
        for (ix = 0; ix < info.nx; ix++)
                for (iy = 0; iy < info.ny; iy++) {
                        double x, y, latitude, longitude, z;
                        int inside;
                        turtle_map_node(map, ix, iy, &x, &y, NULL);
                        turtle_projection_unproject(projection, x, y, &latitude, &longitude);
                        turtle_stack_elevation(stack, latitude, longitude, &z, &inside);
                        if (inside)
                                turtle_map_fill(map, ix, iy, z);
                        else
                                outside++;
                }
        clock_gettime(CLOCK_MONOTONIC, &t1);
        printf("%ld %ld %.6f\n", (long)info.nx * info.ny, outside,
            (t1.tv_sec - t0.tv_sec) + 1e-9 * (t1.tv_nsec - t0.tv_nsec));
        turtle_map_destroy(&map);
        turtle_stack_destroy(&stack);
        return EXIT_SUCCESS;
}
