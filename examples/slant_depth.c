/*
 * slant_depth.c -- the slant depth of the atmosphere: a fan of lines of sight from
 * a point on the ground of a tile, through rock of one density (2650 kg/m^3) and
 * air whose density falls with altitude (1.205 kg/m^3 at altitude 0, by a factor e
 * every 8400 m), each advanced by turtle_stepper_advance_exp_n.  What an air-shower
 * or a muon-flux code starts from: the grammage a particle crosses on its way to or
 * from the sky, and where along its line it has crossed a given one.
 *
 * The point sits 0.5 m above the lowest node of the middle ninth of the tile given
 * on the command line (an .hgt file; default N45E003.hgt); the fan looks north at
 * 17 elevations, 10 to 90 degrees.  Two batches in one call: rays 0-16 go up to a
 * 30 km ceiling without a budget, and their depth is the slant depth to it (a ray
 * may leave the tile or meet the ground first: `stop` says); rays 17-33 stop where
 * they have crossed 3000 kg/m^2 (300 g/cm^2).
 *
 *   cc -Iinclude examples/slant_depth.c -Lturtle_amd -lturtle_amd -lm \
 *      -Wl,-rpath,$PWD/turtle_amd -o slant_depth
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "turtle_amd.h"

#define N_FAN 17
#define N_RAYS (2 * N_FAN)
#define CEILING 3.0E+04
#define DEPTH 3.0E+03

static const char * const why[] = { "spent", "distance", "left", "ceiling", "max_steps" };

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
        int ix, iy, r;
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

        /* medium 0 is the rock under the map, uniform; medium 1 the air above it */
        const double density[2] = { 2650., 1.205 };
        const double scale_height[2] = { HUGE_VAL, 8400. };

        static double lat[N_RAYS], lon[N_RAYS], height[N_RAYS], az[N_RAYS], el[N_RAYS], budget[N_RAYS];
        static double position[N_RAYS][3], direction[N_RAYS][3], depth[N_RAYS], distance[N_RAYS];
        static int data_index[N_RAYS], index[N_RAYS][2], status[N_RAYS];
        for (r = 0; r < N_RAYS; r++) {
                lat[r] = lat0, lon[r] = lon0, height[r] = 0.5, az[r] = 0.;
                el[r] = 10. + 5. * (r % N_FAN);
                budget[r] = (r < N_FAN) ? HUGE_VAL : DEPTH;
        }
        turtle_stepper_position_n(stepper, N_RAYS, lat, lon, height, 0, &position[0][0], data_index,
            TURTLE_AMD_HOST);
        turtle_ecef_from_horizontal_n(N_RAYS, lat, lon, az, el, &direction[0][0], TURTLE_AMD_HOST);

        turtle_stepper_advance_exp_n(stepper, N_RAYS, &position[0][0], &direction[0][0], density, scale_height,
            budget, NULL, CEILING, 1000000, &index[0][0], depth, distance, NULL, status, TURTLE_AMD_HOST);

        for (r = 0; r < N_FAN; r++)
                printf("slant %2d elevation %4.1f stop %-9s distance %.6f m depth %.6e kg/m2\n", r, el[r],
                    why[status[r]], distance[r], depth[r]);
        for (r = N_FAN; r < N_RAYS; r++)
                printf("reach %2d elevation %4.1f stop %-9s distance %.6f m depth %.6e kg/m2\n", r, el[r],
                    why[status[r]], distance[r], depth[r]);
        /* the vertical ray against the closed form rho0 H (exp(-a0 / H) - exp(-a1 / H)) */
        const double a0 = z_min + 0.5, a1 = a0 + distance[N_FAN - 1];
        printf("vertical %.6e kg/m2 closed form %.6e kg/m2\n", depth[N_FAN - 1],
            density[1] * scale_height[1] * (exp(-a0 / scale_height[1]) - exp(-a1 / scale_height[1])));

        turtle_stepper_destroy(&stepper);
        turtle_map_destroy(&map);
        return EXIT_SUCCESS;
}
