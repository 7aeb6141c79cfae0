/*
 * rock_length.c -- the rock length along lines of sight from one detector, the
 * use the reference's examples/example-stepper.c:116-143 shows for one
 * direction (its loop: step until the ray climbs above altitude_max, adding
 * each step that started below the topography), for a whole fan of directions
 * in one turtle_stepper_traverse_n call.
 *
 * The detector sits 0.5 m above the ground at the middle of the tile given on
 * the command line (an .hgt file; default N45E003.hgt); the fan is 360 azimuths
 * x 60 elevations from 0 to 30 degrees.  Prints the rock length of a few of
 * them and the opacity image's mean.
 *
 *   cc -Iinclude examples/rock_length.c -Lturtle_amd -lturtle_amd -lm \
 *      -Wl,-rpath,$PWD/turtle_amd -o rock_length
 */
#include <stdio.h>
#include <stdlib.h>

#include "turtle_amd.h"

#define N_AZIMUTH 360
#define N_ELEVATION 60
#define N_RAYS (N_AZIMUTH * N_ELEVATION)

static void on_error(enum turtle_return code, turtle_function_t * function, const char * message)
{
        (void)function;
        fprintf(stderr, "turtle error %d: %s\n", (int)code, message);
        exit(EXIT_FAILURE);
}

int main(int argc, char * argv[])
{
        turtle_error_handler_set(&on_error);
        const char * path = (argc > 1) ? argv[1] : "N45E003.hgt";

        struct turtle_map * map;
        turtle_map_load(&map, path);
        struct turtle_map_info info;
        turtle_map_meta(map, &info, NULL);

        struct turtle_stepper * stepper;
        turtle_stepper_create(&stepper);
        turtle_stepper_add_map(stepper, map, 0.);
        const int media = turtle_amd_stepper_media(stepper); /* 2: rock (0) and air (1) */

        /* the detector, repeated for every direction of the fan */
        static double lat[N_RAYS], lon[N_RAYS], height[N_RAYS], az[N_RAYS], el[N_RAYS];
        static double position[N_RAYS][3], direction[N_RAYS][3];
        static int data_index[N_RAYS], index[N_RAYS][2], n_steps[N_RAYS];
        int r;
        for (r = 0; r < N_RAYS; r++) {
                lat[r] = 0.5 * (info.y[0] + info.y[1]), lon[r] = 0.5 * (info.x[0] + info.x[1]);
                height[r] = 0.5;
                az[r] = 360. * (r % N_AZIMUTH) / N_AZIMUTH;
                el[r] = 30. * (r / N_AZIMUTH) / N_ELEVATION;
        }
        turtle_stepper_position_n(stepper, N_RAYS, lat, lon, height, 0, &position[0][0], data_index,
            TURTLE_AMD_HOST);
        turtle_ecef_from_horizontal_n(N_RAYS, lat, lon, az, el, &direction[0][0], TURTLE_AMD_HOST);

        /* the reference's loop, every direction at once: length[m][r], the path of ray r in medium m */
        const double altitude_max = 2.0E+03;
        double * length = malloc((size_t)media * N_RAYS * sizeof(*length));
        turtle_stepper_traverse_n(stepper, N_RAYS, &position[0][0], &direction[0][0], altitude_max,
            1000000, &index[0][0], length, n_steps, NULL, TURTLE_AMD_HOST);
        const double * rock = length; /* medium 0: below the topography */

        double mean = 0.;
        long steps = 0;
        for (r = 0; r < N_RAYS; r++) mean += rock[r] / N_RAYS, steps += n_steps[r];
        for (r = 0; r < N_RAYS; r += N_RAYS / 8 + 7)
                printf("azimuth %6.1f elevation %5.2f rock %12.3f m\n", az[r], el[r], rock[r]);
        printf("%d lines of sight, %ld steps, mean rock length %.3f m\n", N_RAYS, steps, mean);

        free(length);
        turtle_stepper_destroy(&stepper);
        turtle_map_destroy(&map);
        return EXIT_SUCCESS;
}
