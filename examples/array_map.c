/*
 * array_map.c -- a map made from an array in memory, traced over, and a window of
 * it read back: the path from a DEM that a program has computed (a fractal ground, a
 * void-filled tile, the output of its own kernel) to a stepper, without a file and
 * without a turtle_map_fill call per node.
 *
 *  1. a 301 x 201 grid of elevations -- a ridge along the map's meridian -- becomes a
 *     geographic map with one turtle_map_fill_n (rows SOUTH TO NORTH);
 *  2. 10 000 rays start 300 m above the plain, 2 to 4 km west of the ridge, heading east
 *     one degree below the horizontal: the ridge stops them all (turtle_stepper_trace_n);
 *  3. an excavation is patched into the map -- a 40 x 30 window, one more call, and
 *     only the window moves -- and the same rays are traced again: those in line with
 *     the cut pass through and leave the map; the window comes back with turtle_map_node_n.
 *
 *   cc -Iinclude examples/array_map.c -Lturtle_amd -lturtle_amd \
 *      -Wl,-rpath,$PWD/turtle_amd -lm -o array_map
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "turtle.h"

#define NX 301
#define NY 201
#define N_RAYS 10000

static void handle_error(enum turtle_return code, turtle_function_t * function, const char * message)
{
        (void)code;
        (void)function;
        fprintf(stderr, "A TURTLE library error occurred:\n%s\n", message);
        exit(EXIT_FAILURE);
}

/* rays stopped by the ground (index[0] == 0 at the end), and their mean path */
static long trace(struct turtle_stepper * stepper, const double * position, const double * direction,
    double * mean_length)
{
        static double pos[N_RAYS][3], length[N_RAYS];
        static int index[N_RAYS][2];
        long i, hits = 0;
        memcpy(pos, position, sizeof(pos));
        turtle_stepper_trace_n(stepper, N_RAYS, &pos[0][0], direction, 100000, &index[0][0], length, NULL, 0,
            TURTLE_AMD_HOST);
        *mean_length = 0.;
        for (i = 0; i < N_RAYS; i++) {
                if (index[i][0] != 0) continue;
                hits++;
                *mean_length += length[i];
        }
        if (hits > 0) *mean_length /= hits;
        return hits;
}

int main(void)
{
        turtle_error_handler_set(&handle_error);

        /* 1. the array: 0.3 x 0.2 degrees around 45.5N 3.5E, a 900 m ridge on a 400 m plain */
        static double z[NY][NX];
        int i, j;
        for (j = 0; j < NY; j++)
                for (i = 0; i < NX; i++) {
                        const double u = (i - 150) / 25.;
                        z[j][i] = 400. + 500. * exp(-u * u) + 20. * sin(0.2 * j);
                }
        struct turtle_map * map = NULL;
        struct turtle_map_info info = {
                .nx = NX, .ny = NY, .x = { 3.35, 3.65 }, .y = { 45.4, 45.6 }, .z = { 0., 2000. } };
        turtle_map_create(&map, &info, NULL);
        turtle_map_fill_n(map, 0, 0, NX, NY, &z[0][0], NX, 0, NULL, TURTLE_AMD_HOST);

        /* 2. the rays */
        struct turtle_stepper * stepper = NULL;
        turtle_stepper_create(&stepper);
        turtle_stepper_add_map(stepper, map, 0.);
        static double latitude[N_RAYS], longitude[N_RAYS], height[N_RAYS], azimuth[N_RAYS], elevation[N_RAYS];
        static double position[N_RAYS][3], direction[N_RAYS][3];
        static int data[N_RAYS];
        for (i = 0; i < N_RAYS; i++) {
                latitude[i] = 45.42 + 0.16 * (i % 100) / 99.;
                longitude[i] = 3.45 + 0.02 * (i / 100) / 99.;
                height[i] = 300.;
                azimuth[i] = 90.;
                elevation[i] = -1.;
        }
        turtle_stepper_position_n(stepper, N_RAYS, latitude, longitude, height, 0, &position[0][0], data,
            TURTLE_AMD_HOST);
        turtle_ecef_from_horizontal_n(N_RAYS, latitude, longitude, azimuth, elevation, &direction[0][0],
            TURTLE_AMD_HOST);
        double mean;
        long hits = trace(stepper, &position[0][0], &direction[0][0], &mean);
        printf("the ridge: %ld of %d rays end in the ground, after %.0f m on average\n", hits, N_RAYS, mean);

        /* 3. an excavation through the ridge: nodes 130 .. 169 x 85 .. 114 down to 450 m */
        static double pit[30][40], back[30][64];
        long clamped = 0;
        for (j = 0; j < 30; j++)
                for (i = 0; i < 40; i++) pit[j][i] = 450.;
        turtle_map_fill_n(map, 130, 85, 40, 30, &pit[0][0], 40, TURTLE_AMD_FILL_CLAMP, &clamped, TURTLE_AMD_HOST);
        hits = trace(stepper, &position[0][0], &direction[0][0], &mean);
        printf("excavated: %ld of %d rays end in the ground, after %.0f m on average\n", hits, N_RAYS, mean);

        /* the window as the map holds it now (rows 64 doubles apart: what lies between is not touched) */
        turtle_map_node_n(map, 130, 85, 40, 30, &back[0][0], 64, TURTLE_AMD_HOST);
        printf("node (130, 85): %.3f m, node (169, 114): %.3f m, %ld clamped\n", back[0][0], back[29][39], clamped);

        turtle_stepper_destroy(&stepper);
        turtle_map_destroy(&map);
        return EXIT_SUCCESS;
}
