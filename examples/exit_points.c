/*
 * exit_points.c -- where lines of sight enter and leave the rock: a fan of
 * directions from a detector at the foot of a tile, every crossing of every
 * direction recorded by one turtle_stepper_crossings_n call, and the points
 * turned into latitude, longitude and altitude by one turtle_ecef_to_geodetic_n
 * call.  What an acceptance map on the topography, or the segments handed to a
 * transport code, start from.
 *
 * The detector sits 0.5 m above the lowest node of the middle ninth of the tile
 * given on the command line (an .hgt file; default N45E003.hgt); the fan is 36
 * azimuths x 6 elevations from 0 to 25 degrees, up to a 2000 m ceiling.  For
 * each ray that meets rock it prints the first entry into the rock (medium 0)
 * and the last exit from it (into the air or out of the data), and -- from one
 * turtle_stepper_normal_n call on the first crossing of every ray -- the cosine
 * of the angle between the ray and the normal of the surface it crossed there.
 *
 *   cc -Iinclude examples/exit_points.c -Lturtle_amd -lturtle_amd -lm \
 *      -Wl,-rpath,$PWD/turtle_amd -o exit_points
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "turtle_amd.h"

#define N_AZIMUTH 36
#define N_ELEVATION 6
#define N_RAYS (N_AZIMUTH * N_ELEVATION)
#define CAPACITY 64

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
        int ix, iy, r, c;
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

        static double lat[N_RAYS], lon[N_RAYS], height[N_RAYS], az[N_RAYS], el[N_RAYS];
        static double position[N_RAYS][3], direction[N_RAYS][3];
        static int data_index[N_RAYS], index[N_RAYS][2], n_crossings[N_RAYS];
        for (r = 0; r < N_RAYS; r++) {
                lat[r] = lat0, lon[r] = lon0, height[r] = 0.5;
                az[r] = 360. * (r % N_AZIMUTH) / N_AZIMUTH;
                el[r] = 25. * (r / N_AZIMUTH) / N_ELEVATION;
        }
        turtle_stepper_position_n(stepper, N_RAYS, lat, lon, height, 0, &position[0][0], data_index,
            TURTLE_AMD_HOST);
        turtle_ecef_from_horizontal_n(N_RAYS, lat, lon, az, el, &direction[0][0], TURTLE_AMD_HOST);

        /* the reference's line-of-sight loop with every crossing kept: slot c of ray r is [c][r] */
        static double point[CAPACITY][N_RAYS][3], distance[CAPACITY][N_RAYS];
        static int media[CAPACITY][N_RAYS][2];
        turtle_stepper_crossings_n(stepper, N_RAYS, &position[0][0], &direction[0][0], 2.0E+03, 1000000,
            &index[0][0], NULL, NULL, n_crossings, CAPACITY, &point[0][0][0], &distance[0][0],
            &media[0][0][0], TURTLE_AMD_HOST);

        /* every slot as latitude, longitude, altitude (the empty ones too: one call) */
        static double p_lat[CAPACITY][N_RAYS], p_lon[CAPACITY][N_RAYS], p_alt[CAPACITY][N_RAYS];
        turtle_ecef_to_geodetic_n((long)CAPACITY * N_RAYS, &point[0][0][0], &p_lat[0][0], &p_lon[0][0],
            &p_alt[0][0], TURTLE_AMD_HOST);

        /* the normal of the surface each ray crossed first: the top of layer min(media) */
        static double normal[N_RAYS][3];
        static int first_layer[N_RAYS], normal_data[N_RAYS];
        for (r = 0; r < N_RAYS; r++)
                first_layer[r] = (n_crossings[r] == 0) ? -1 : /* (an empty slot reads {0, 0}) */
                    ((media[0][r][0] < media[0][r][1]) ? media[0][r][0] : media[0][r][1]);
        turtle_stepper_normal_n(stepper, N_RAYS, &point[0][0][0], first_layer, &normal[0][0], normal_data,
            TURTLE_AMD_HOST);

        int through_rock = 0;
        for (r = 0; r < N_RAYS; r++) {
                const int kept = (n_crossings[r] < CAPACITY) ? n_crossings[r] : CAPACITY;
                int entry = -1, exit = -1;
                for (c = 0; c < kept; c++) {
                        if ((media[c][r][1] == 0) && (entry < 0)) entry = c;
                        if (media[c][r][0] == 0) exit = c;
                }
                if (entry < 0) continue;
                through_rock++;
                printf("ray %3d azimuth %5.1f elevation %4.1f entry %.9f %.9f %.4f", r, az[r], el[r],
                    p_lat[entry][r], p_lon[entry][r], p_alt[entry][r]);
                if (exit > entry)
                        printf(" exit %.9f %.9f %.4f", p_lat[exit][r], p_lon[exit][r], p_alt[exit][r]);
                else
                        printf(" exit none");
                printf(" span %.3f m", (exit > entry) ? distance[exit][r] - distance[entry][r] : 0.);
                if (normal_data[r] >= 0)
                        printf(" first crossing cosine %.6f\n", direction[r][0] * normal[r][0] +
                                direction[r][1] * normal[r][1] + direction[r][2] * normal[r][2]);
                else
                        printf(" first crossing cosine none\n");
        }
        printf("%d lines of sight, %d through rock\n", N_RAYS, through_rock);

        turtle_stepper_destroy(&stepper);
        turtle_map_destroy(&map);
        return EXIT_SUCCESS;
}
