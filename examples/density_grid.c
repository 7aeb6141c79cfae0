/*
 * density_grid.c -- muography's forward model in one call: the opacity (column
 * depth, kg/m^2) along a fan of lines of sight from one point at the foot of a
 * hill, through rock whose density is a box of voxels with a light body in it
 * (turtle_stepper_advance_grid_n), printed with and without the body.  The ratio of
 * the two is what a muon telescope at that point would see of the body.
 *
 * The point sits 0.5 m above the lowest node of the middle ninth of the tile given
 * on the command line (an .hgt file; default N45E003.hgt); the fan looks north at
 * 16 elevations, 2 to 32 degrees, up to a 5 km ceiling.  The box is east-north-up at
 * the point: 16 x 16 x 8 voxels of 500 x 500 x 250 m, 4 km to either side, from the
 * point 8 km to the north, from 250 m under it to 1750 m above.  Its rock has
 * 2650 kg/m^3, the body (4 x 4 x 4 voxels, 2 to 4 km north) 1800; outside the box the rock has
 * density[0] and the air density[1].
 *
 *   cc -Iinclude examples/density_grid.c -Lturtle_amd -lturtle_amd -lm \
 *      -Wl,-rpath,$PWD/turtle_amd -o density_grid
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "turtle_amd.h"

#define N_FAN 16
#define CEILING 5.0E+03
#define N0 16
#define N1 16
#define N2 8

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

        /* the point: the lowest node of the tile's middle ninth */
        double lat0 = 0., lon0 = 0., z_min = HUGE_VAL;
        int ix, iy, r, i0, i1, i2, pass;
        for (iy = info.ny / 3; iy < 2 * info.ny / 3; iy++)
                for (ix = info.nx / 3; ix < 2 * info.nx / 3; ix++) {
                        double x, y, z;
                        turtle_map_node(map, ix, iy, &x, &y, &z);
                        if (z < z_min) z_min = z, lon0 = x, lat0 = y;
                }
        printf("point %.17g %.17g ground %.3f m\n", lat0, lon0, z_min);

        struct turtle_stepper * stepper;
        turtle_stepper_create(&stepper);
        turtle_stepper_add_map(stepper, map, 0.);

        /* medium 0 is the rock under the map, medium 1 the air above it */
        const double density[2] = { 2650., 1.205 };
        static double voxels[N2][N1][N0];
        struct turtle_amd_grid grid = { .size = { 500., 500., 250. }, .n = { N0, N1, N2 }, .medium = 0,
                .density = &voxels[0][0][0] };
        turtle_amd_grid_enu(&grid, lat0, lon0, z_min, -4000., 0., -250.);

        static double lat[N_FAN], lon[N_FAN], height[N_FAN], az[N_FAN], el[N_FAN], budget[N_FAN];
        static double origin[N_FAN][3], position[N_FAN][3], direction[N_FAN][3], depth[2][N_FAN], distance[N_FAN];
        static int data_index[N_FAN], index[N_FAN][2], status[N_FAN];
        for (r = 0; r < N_FAN; r++) {
                lat[r] = lat0, lon[r] = lon0, height[r] = 0.5, az[r] = 0.;
                el[r] = 2. + 2. * r;
                budget[r] = HUGE_VAL;
        }
        turtle_stepper_position_n(stepper, N_FAN, lat, lon, height, 0, &origin[0][0], data_index, TURTLE_AMD_HOST);
        turtle_ecef_from_horizontal_n(N_FAN, lat, lon, az, el, &direction[0][0], TURTLE_AMD_HOST);

        for (pass = 0; pass < 2; pass++) { /* with the body, then without it */
                for (i2 = 0; i2 < N2; i2++)
                        for (i1 = 0; i1 < N1; i1++)
                                for (i0 = 0; i0 < N0; i0++) {
                                        const int body = (pass == 0) && (i0 >= 6) && (i0 < 10) && (i1 >= 4) && (i1 < 8) &&
                                            (i2 >= 1) && (i2 < 5);
                                        voxels[i2][i1][i0] = body ? 1800. : 2650.;
                                }
                for (r = 0; r < N_FAN; r++)
                        position[r][0] = origin[r][0], position[r][1] = origin[r][1], position[r][2] = origin[r][2];
                turtle_stepper_advance_grid_n(stepper, N_FAN, &position[0][0], &direction[0][0], density, &grid, budget,
                    NULL, CEILING, 1000000, &index[0][0], depth[pass], distance, NULL, status, TURTLE_AMD_HOST);
        }
        for (r = 0; r < N_FAN; r++)
                printf("line %2d elevation %4.1f distance %.6f m opacity %.6e kg/m2 without %.6e kg/m2 ratio %.4f\n", r,
                    el[r], distance[r], depth[0][r], depth[1][r], depth[0][r] / depth[1][r]);

        turtle_stepper_destroy(&stepper);
        turtle_map_destroy(&map);
        return EXIT_SUCCESS;
}
