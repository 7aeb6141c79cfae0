/*
 * horizon.c -- the skyline around a detector: for each of 360 azimuths, how high
 * the ground stands against the sky, from one turtle_stepper_horizon_n call.
 * What the open-sky acceptance of a muography telescope, or the view of an
 * antenna on the ground, starts from.
 *
 * The detector sits 2 m above the lowest node of the middle ninth of the tile
 * given on the command line (an .hgt file; default N45E003.hgt), placed by
 * turtle_stepper_position_n.  Every line of sight is sampled at 256 distances
 * in a geometric progression from 30 m to 100 km; for each azimuth it prints
 * the elevation angle of the skyline, the horizontal distance of the sample
 * that set it and its range.
 *
 *   cc -Iinclude examples/horizon.c -Lturtle_amd -lturtle_amd -lm \
 *      -Wl,-rpath,$PWD/turtle_amd -o horizon
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "turtle_amd.h"

#define N_AZIMUTH 360
#define N_DISTANCE 256

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

        /* the detector: the lowest node of the tile's middle ninth */
        double lat0 = 0., lon0 = 0., z_min = HUGE_VAL;
        int ix, iy, a, k;
        for (iy = info.ny / 3; iy < 2 * info.ny / 3; iy++)
                for (ix = info.nx / 3; ix < 2 * info.nx / 3; ix++) {
                        double x, y, z;
                        turtle_map_node(map, ix, iy, &x, &y, &z);
                        if (z < z_min) z_min = z, lon0 = x, lat0 = y;
                }
        printf("detector %.17g %.17g\n", lat0, lon0);

        struct turtle_stepper * stepper;
        turtle_stepper_create(&stepper);
        turtle_stepper_add_map(stepper, map, 0.);

        const double height = 2.;
        double position[3];
        int data_index;
        turtle_stepper_position_n(stepper, 1, &lat0, &lon0, &height, 0, position, &data_index, TURTLE_AMD_HOST);

        static double azimuth[N_AZIMUTH], distance[N_DISTANCE];
        for (a = 0; a < N_AZIMUTH; a++) azimuth[a] = (double)a;
        for (k = 0; k < N_DISTANCE; k++) distance[k] = 30. * pow(1.0E+05 / 30., k / (N_DISTANCE - 1.));

        /* the whole profile in one call: lines that meet no data keep elevation -90 and sample 0 */
        static double elevation[N_AZIMUTH], range[N_AZIMUTH];
        static int sample[N_AZIMUTH];
        for (a = 0; a < N_AZIMUTH; a++) elevation[a] = -90., range[a] = 0.;
        turtle_stepper_horizon_n(stepper, 1, position, N_AZIMUTH, azimuth, N_DISTANCE, distance, 0, elevation,
            sample, range, TURTLE_AMD_HOST);

        double open_sky = 0.; /* the solid angle above the skyline, as a fraction of the upper half-space */
        for (a = 0; a < N_AZIMUTH; a++) {
                if (sample[a] > 0)
                        printf("azimuth %5.1f elevation %9.5f at %10.3f m range %10.3f m\n", azimuth[a],
                            elevation[a], distance[sample[a] - 1], range[a]);
                else
                        printf("azimuth %5.1f elevation none\n", azimuth[a]);
                const double el = (elevation[a] > 0.) ? elevation[a] : 0.;
                open_sky += (1. - sin(el * 3.14159265358979323846 / 180.)) / N_AZIMUTH;
        }
        printf("%d azimuths, open sky %.4f of the upper half-space\n", N_AZIMUTH, open_sky);

        turtle_stepper_destroy(&stepper);
        turtle_map_destroy(&map);
        return EXIT_SUCCESS;
}
