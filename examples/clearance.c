/*
 * clearance.c -- which ground stations see which points in the air, and by what
 * margin: the whole matrix from one turtle_stepper_clearance_n call.  What link
 * planning and siting start from: the margin of an open line says how much of a
 * Fresnel zone is free, that of a blocked one how much mast would open it.
 *
 * Five stations stand 3 m above the ground of the tile given on the command
 * line (an .hgt file; default N45E003.hgt), placed by turtle_stepper_position_n
 * at fixed fractions of the tile; four points hang in the air between 1.2 and
 * 6 km of altitude.  Every line is the straight chord between the two points,
 * sampled at 512 interior fractions; for each pair it prints whether the two
 * see each other, the least height of the chord above the ground and where
 * along the chord that is.
 *
 *   cc -Iinclude examples/clearance.c -Lturtle_amd -lturtle_amd -lm \
 *      -Wl,-rpath,$PWD/turtle_amd -o clearance
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "turtle_amd.h"

#define N_STATION 5
#define N_POINT 4
#define N_FRACTION 512

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
        const double x0 = info.x[0], dx = info.x[1] - info.x[0], y0 = info.y[0], dy = info.y[1] - info.y[0];

        struct turtle_stepper * stepper;
        turtle_stepper_create(&stepper);
        turtle_stepper_add_map(stepper, map, 0.);

        /* the stations: 3 m above the ground, at fixed fractions of the tile (x: longitude, y: latitude) */
        static const double at[N_STATION][2] = { { 0.2, 0.3 }, { 0.7, 0.2 }, { 0.5, 0.5 }, { 0.3, 0.8 }, { 0.85, 0.75 } };
        double latitude[N_STATION], longitude[N_STATION], height[N_STATION], station[N_STATION][3];
        int data_index[N_STATION], r, t, k;
        for (r = 0; r < N_STATION; r++)
                longitude[r] = x0 + at[r][0] * dx, latitude[r] = y0 + at[r][1] * dy, height[r] = 3.;
        turtle_stepper_position_n(stepper, N_STATION, latitude, longitude, height, 0, &station[0][0], data_index,
            TURTLE_AMD_HOST);

        /* the points in the air: (x, y) fractions of the tile -- the last one outside it -- and an altitude */
        static const double air[N_POINT][3] = { { 0.4, 0.4, 1200. }, { 0.6, 0.7, 2500. }, { 0.1, 0.6, 6000. },
                { 1.2, 0.5, 4000. } };
        double point[N_POINT][3];
        for (t = 0; t < N_POINT; t++)
                turtle_ecef_from_geodetic(y0 + air[t][1] * dy, x0 + air[t][0] * dx, air[t][2], point[t]);

        static double fraction[N_FRACTION];
        for (k = 0; k < N_FRACTION; k++) fraction[k] = (2. * k + 1.) / (2. * N_FRACTION);

        /* the whole matrix in one call: a line that meets no data keeps its clearance and gets sample 0 */
        double clearance[N_STATION][N_POINT];
        int sample[N_STATION][N_POINT], n_data[N_STATION][N_POINT];
        for (r = 0; r < N_STATION; r++)
                for (t = 0; t < N_POINT; t++) clearance[r][t] = 0.;
        turtle_stepper_clearance_n(stepper, N_STATION, &station[0][0], N_POINT, &point[0][0], N_FRACTION, fraction, 0,
            0, &clearance[0][0], &sample[0][0], &n_data[0][0], TURTLE_AMD_HOST);

        int seen = 0;
        for (r = 0; r < N_STATION; r++)
                for (t = 0; t < N_POINT; t++) {
                        if (sample[r][t] == 0) {
                                printf("station %d point %d unknown\n", r, t);
                                continue;
                        }
                        const int open = clearance[r][t] >= 0.;
                        seen += open;
                        printf("station %d point %d %-7s margin %12.3f m at fraction %.6f (%d of %d samples over data)\n",
                            r, t, open ? "seen" : "blocked", clearance[r][t], fraction[sample[r][t] - 1], n_data[r][t],
                            N_FRACTION);
                }
        printf("%d of %d pairs see each other\n", seen, N_STATION * N_POINT);

        turtle_stepper_destroy(&stepper);
        turtle_map_destroy(&map);
        return EXIT_SUCCESS;
}
