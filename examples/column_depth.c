/*
 * column_depth.c -- how far a particle gets: a fan of lines of sight from a point
 * on the ground of a tile, each advanced by one turtle_stepper_advance_n call
 * until the column depth it has crossed (density x path, rock 2650 kg/m^3, air
 * 1.205 kg/m^3) reaches a budget -- here the approximate ranges of 10 GeV,
 * 100 GeV and 1 TeV muons in standard rock.  What a muography acceptance, or a
 * backward Monte-Carlo that asks "where was this muon one range ago", starts
 * from.
 *
 * The point sits 0.5 m above the lowest node of the middle ninth of the tile
 * given on the command line (an .hgt file; default N45E003.hgt); the fan is 36
 * azimuths x 3 elevations (2, 8 and 14 degrees), up to a 4000 m ceiling.  For
 * each ray and budget it prints how far the ray got, the depth it crossed and why
 * it stopped.  The last line is the point-to-point recipe: the rock between the
 * point and a fixed second one, from a unit direction, distance_max = the length
 * of the chord and densities {1, 0}.
 *
 *   cc -Iinclude examples/column_depth.c -Lturtle_amd -lturtle_amd -lm \
 *      -Wl,-rpath,$PWD/turtle_amd -o column_depth
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "turtle_amd.h"

#define N_AZIMUTH 36
#define N_ELEVATION 3
#define N_FAN (N_AZIMUTH * N_ELEVATION)
#define N_BUDGET 3
#define N_RAYS (N_FAN * N_BUDGET)

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
        int ix, iy, r, j;
        for (iy = info.ny / 3; iy < 2 * info.ny / 3; iy++)
                for (ix = info.nx / 3; ix < 2 * info.nx / 3; ix++) {
                        double x, y, z;
                        turtle_map_node(map, ix, iy, &x, &y, &z);
                        if (z < z_min) z_min = z, lon0 = x, lat0 = y;
                }
        printf("point %.17g %.17g\n", lat0, lon0);

        struct turtle_stepper * stepper;
        turtle_stepper_create(&stepper);
        turtle_stepper_add_map(stepper, map, 0.);

        /* medium 0 is the rock under the map, medium 1 the air above it */
        const double density[2] = { 2650., 1.205 };
        /* kg/m^2: about the ranges of 10 GeV, 100 GeV and 1 TeV muons in standard rock */
        const double range[N_BUDGET] = { 4.84E+04, 4.08E+05, 2.45E+06 };
        const double energy[N_BUDGET] = { 10., 100., 1000. };

        /* ray r: direction r % N_FAN of the fan, budget r / N_FAN */
        static double lat[N_RAYS], lon[N_RAYS], height[N_RAYS], az[N_RAYS], el[N_RAYS], budget[N_RAYS];
        static double position[N_RAYS][3], direction[N_RAYS][3], depth[N_RAYS], distance[N_RAYS];
        static int data_index[N_RAYS], index[N_RAYS][2], status[N_RAYS];
        for (r = 0; r < N_RAYS; r++) {
                const int f = r % N_FAN;
                lat[r] = lat0, lon[r] = lon0, height[r] = 0.5;
                az[r] = 360. * (f % N_AZIMUTH) / N_AZIMUTH;
                el[r] = 2. + 6. * (f / N_AZIMUTH);
                budget[r] = range[r / N_FAN];
        }
        turtle_stepper_position_n(stepper, N_RAYS, lat, lon, height, 0, &position[0][0], data_index,
            TURTLE_AMD_HOST);
        turtle_ecef_from_horizontal_n(N_RAYS, lat, lon, az, el, &direction[0][0], TURTLE_AMD_HOST);
        const double origin[3] = { position[0][0], position[0][1], position[0][2] };

        turtle_stepper_advance_n(stepper, N_RAYS, &position[0][0], &direction[0][0], density, budget, NULL,
            4.0E+03, 1000000, &index[0][0], depth, distance, NULL, status, TURTLE_AMD_HOST);

        int spent = 0;
        for (r = 0; r < N_RAYS; r++) {
                printf("ray %3d energy %6.0f GeV azimuth %5.1f elevation %4.1f stop %-9s distance %.6f m depth %.6e kg/m2\n",
                    r, energy[r / N_FAN], az[r], el[r], why[status[r]], distance[r], depth[r]);
                if (status[r] == TURTLE_AMD_ADVANCE_SPENT) spent++;
        }
        printf("%d rays, %d stopped by their budget\n", N_RAYS, spent);

        /* point to point: the rock between the point and one 0.03 degrees north-east of it, 300 m up */
        double target[3], chord[3], length = 0., rock, there;
        const double t_lat = lat0 + 0.03, t_lon = lon0 + 0.03, t_height = 300.;
        const double rock_only[2] = { 1., 0. }, no_budget = HUGE_VAL;
        int t_data, t_index[2], t_status;
        turtle_stepper_position_n(stepper, 1, &t_lat, &t_lon, &t_height, 0, target, &t_data, TURTLE_AMD_HOST);
        for (j = 0; j < 3; j++) chord[j] = target[j] - origin[j], length += chord[j] * chord[j];
        length = sqrt(length);
        for (j = 0; j < 3; j++) chord[j] /= length;
        double from[3] = { origin[0], origin[1], origin[2] };
        turtle_stepper_advance_n(stepper, 1, from, chord, rock_only, &no_budget, &length, HUGE_VAL, 1000000,
            t_index, &rock, &there, NULL, &t_status, TURTLE_AMD_HOST);
        printf("chord %.6f m stop %s rock %.6f m\n", length, why[t_status], rock);

        turtle_stepper_destroy(&stepper);
        turtle_map_destroy(&map);
        return EXIT_SUCCESS;
}
