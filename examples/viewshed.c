/*
 * viewshed.c -- what a detector sees of the ground around it: along each of 8
 * azimuths, the ranges of horizontal distance in view, from one
 * turtle_stepper_viewshed_n call.  Which slopes the lines of sight of a muography
 * telescope enter first, or where a target on a 10 m mast comes into view of an
 * antenna.
 *
 * The detector sits 2 m above the lowest node of the middle ninth of the tile
 * given on the command line (an .hgt file; default N45E003.hgt), placed by
 * turtle_stepper_position_n.  Every line of sight is sampled every 50 m out to
 * 12.8 km.  For the ground itself and for the mast it prints, per azimuth, the
 * flags of the samples ('#' in view, '.' hidden, '?' no data) and the ranges in
 * view.
 *
 *   cc -Iinclude examples/viewshed.c -Lturtle_amd -lturtle_amd -lm \
 *      -Wl,-rpath,$PWD/turtle_amd -o viewshed
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "turtle_amd.h"

#define N_AZIMUTH 8
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
        int ix, iy, a, k, t;
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
        for (a = 0; a < N_AZIMUTH; a++) azimuth[a] = 45. * a;
        for (k = 0; k < N_DISTANCE; k++) distance[k] = 50. * (k + 1);

        const double target_height[2] = { 0., 10. };
        for (t = 0; t < 2; t++) {
                /* the flags and the counts are all this needs: no sines, no horizons */
                static signed char visible[N_AZIMUTH][N_DISTANCE];
                static int n_visible[N_AZIMUTH];
                turtle_stepper_viewshed_n(stepper, 1, position, N_AZIMUTH, azimuth, N_DISTANCE, distance, 0,
                    target_height[t], &visible[0][0], NULL, NULL, n_visible, TURTLE_AMD_HOST);

                printf("target %g m above the ground\n", target_height[t]);
                for (a = 0; a < N_AZIMUTH; a++) {
                        printf("azimuth %5.1f sees %3d of %d: ", azimuth[a], n_visible[a], N_DISTANCE);
                        for (k = 0; k < N_DISTANCE; k++)
                                putchar((visible[a][k] > 0) ? '#' : ((visible[a][k] == 0) ? '.' : '?'));
                        printf("\n  in view:");
                        for (k = 0; k < N_DISTANCE; k++) {
                                if (visible[a][k] <= 0) continue;
                                const int from = k;
                                while ((k + 1 < N_DISTANCE) && (visible[a][k + 1] > 0)) k++;
                                printf(" %g-%g m", distance[from], distance[k]);
                        }
                        printf("\n");
                }
        }

        turtle_stepper_destroy(&stepper);
        turtle_map_destroy(&map);
        return EXIT_SUCCESS;
}
