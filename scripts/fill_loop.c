/*
 * fill_loop.c -- what a caller did before turtle_map_fill_n (scripts/exp_fill.py, step `loop`):
 * turtle_map_fill for every node of a side x side map, then a first turtle_map_elevation_n, which
 * lays the host rows out in blocks and uploads them, and a second one for comparison.
 * Prints the three times in seconds.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <time.h>

#include "turtle.h"

static double now(void)
{
        struct timespec t;
        clock_gettime(CLOCK_MONOTONIC, &t);
        return t.tv_sec + 1e-9 * t.tv_nsec;
}

int main(int argc, char * argv[])
{
        const int side = (argc > 1) ? atoi(argv[1]) : 3601;
        struct turtle_map * map = NULL;
        struct turtle_map_info info = {
                .nx = side, .ny = side, .x = { 3., 4. }, .y = { 45., 46. }, .z = { 0., 2000. } };
        turtle_map_create(&map, &info, NULL);
        double * z = malloc((size_t)side * side * sizeof(*z));
        int ix, iy;
        for (iy = 0; iy < side; iy++)
                for (ix = 0; ix < side; ix++)
                        z[(size_t)iy * side + ix] = 500. + 400. * sin(0.01 * ix) * cos(0.013 * iy);
        /* the device is up before the clock starts */
        double x = 3.5, y = 45.5, e;
        int inside;
        turtle_map_elevation_n(map, 1, &x, &y, &e, &inside, TURTLE_AMD_HOST);

        const double t0 = now();
        for (iy = 0; iy < side; iy++)
                for (ix = 0; ix < side; ix++) turtle_map_fill(map, ix, iy, z[(size_t)iy * side + ix]);
        const double t1 = now();
        turtle_map_elevation_n(map, 1, &x, &y, &e, &inside, TURTLE_AMD_HOST);
        const double t2 = now();
        turtle_map_elevation_n(map, 1, &x, &y, &e, &inside, TURTLE_AMD_HOST);
        const double t3 = now();
        printf("%.6f %.6f %.6f\n", t1 - t0, t2 - t1, t3 - t2);
        free(z);
        turtle_map_destroy(&map);
        return inside ? 0 : 1;
}
