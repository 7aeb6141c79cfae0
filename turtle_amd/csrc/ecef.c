/*
 * ecef.c -- host entry points of the WGS84 transforms [ref src/turtle/
 * ecef.c:41-207].  The arithmetic is in points.hip; the scalar calls launch
 * it with n = 1.  They return void, as in the reference, so a device failure
 * can only be reported through the error handler (which by default exits).
 */
#include "host.h"

#include <stddef.h>

static int run4(int (*kernel)(long, const double *, const double *, const double *,
                    const double *, double *),
    long n, const double * a, const double * b, const double * c, const double * d,
    size_t out_doubles, double * out, int space)
{
        struct tamd_stage st = { 0 };
        void *da, *db, *dc, *dd, *dout;
        const size_t nb = (size_t)n * sizeof(double);
        tamd_stage_add(&st, a, nb, TAMD_IN, &da);
        tamd_stage_add(&st, b, nb, TAMD_IN, &db);
        tamd_stage_add(&st, c, nb, TAMD_IN, &dc);
        tamd_stage_add(&st, d, nb, TAMD_IN, &dd);
        tamd_stage_add(&st, out, out_doubles * nb, TAMD_OUT, &dout);
        return tamd_stage_open(&st, space) || kernel(n, da, db, dc, dd, dout) || tamd_stage_close(&st);
}

static int run_to_geodetic(long n, const double * ecef, double * latitude, double * longitude,
    double * altitude, int space)
{
        struct tamd_stage st = { 0 };
        void *de, *dla, *dlo, *dal;
        const size_t nb = (size_t)n * sizeof(double);
        tamd_stage_add(&st, ecef, 3 * nb, TAMD_IN, &de);
        tamd_stage_add(&st, latitude, nb, TAMD_OUT, &dla);
        tamd_stage_add(&st, longitude, nb, TAMD_OUT, &dlo);
        tamd_stage_add(&st, altitude, nb, TAMD_OUT, &dal);
        return tamd_stage_open(&st, space) || tamd_k_ecef_to_geodetic(n, de, dla, dlo, dal) ||
            tamd_stage_close(&st);
}

static int run_to_horizontal(long n, const double * latitude, const double * longitude,
    const double * direction, double * azimuth, double * elevation, int space)
{
        struct tamd_stage st = { 0 };
        void *dla, *dlo, *dd, *daz, *del;
        const size_t nb = (size_t)n * sizeof(double);
        tamd_stage_add(&st, latitude, nb, TAMD_IN, &dla);
        tamd_stage_add(&st, longitude, nb, TAMD_IN, &dlo);
        tamd_stage_add(&st, direction, 3 * nb, TAMD_IN, &dd);
        /* outputs are read-modify-write: a null direction leaves them untouched
         * [ref ecef.c:194] */
        tamd_stage_add(&st, azimuth, nb, TAMD_INOUT, &daz);
        tamd_stage_add(&st, elevation, nb, TAMD_INOUT, &del);
        return tamd_stage_open(&st, space) || tamd_k_ecef_to_horizontal(n, dla, dlo, dd, daz, del) ||
            tamd_stage_close(&st);
}

static int k_from_geodetic(long n, const double * lat, const double * lon,
    const double * elev, const double * unused, double * ecef)
{
        (void)unused;
        return tamd_k_ecef_from_geodetic(n, lat, lon, elev, ecef);
}

enum turtle_return turtle_ecef_from_geodetic_n(long n, const double * latitude,
    const double * longitude, const double * elevation, double * ecef, int space)
{
        TAMD_ERROR_INIT(&turtle_ecef_from_geodetic_n);
        if (run4(&k_from_geodetic, n, latitude, longitude, elevation, NULL, 3, ecef, space))
                return TAMD_RAISE_DEVICE();
        return TURTLE_RETURN_SUCCESS;
}

enum turtle_return turtle_ecef_from_horizontal_n(long n, const double * latitude,
    const double * longitude, const double * azimuth, const double * elevation,
    double * direction, int space)
{
        TAMD_ERROR_INIT(&turtle_ecef_from_horizontal_n);
        if (run4(&tamd_k_ecef_from_horizontal, n, latitude, longitude, azimuth, elevation, 3,
                direction, space))
                return TAMD_RAISE_DEVICE();
        return TURTLE_RETURN_SUCCESS;
}

enum turtle_return turtle_ecef_to_geodetic_n(long n, const double * ecef,
    double * latitude, double * longitude, double * altitude, int space)
{
        TAMD_ERROR_INIT(&turtle_ecef_to_geodetic_n);
        if (run_to_geodetic(n, ecef, latitude, longitude, altitude, space)) return TAMD_RAISE_DEVICE();
        return TURTLE_RETURN_SUCCESS;
}

enum turtle_return turtle_ecef_to_horizontal_n(long n, const double * latitude,
    const double * longitude, const double * direction, double * azimuth,
    double * elevation, int space)
{
        TAMD_ERROR_INIT(&turtle_ecef_to_horizontal_n);
        if (run_to_horizontal(n, latitude, longitude, direction, azimuth, elevation, space))
                return TAMD_RAISE_DEVICE();
        return TURTLE_RETURN_SUCCESS;
}

/* ---- scalar forms ---------------------------------------------------------- */

static void raise_void(turtle_function_t * caller)
{
        struct tamd_error error_ = { TURTLE_RETURN_SUCCESS, caller };
        TAMD_RAISE_DEVICE();
}

void turtle_ecef_from_geodetic(
    double latitude, double longitude, double elevation, double ecef[3])
{
        if (tamd_scalar_on_host()) { /* (the caller's option: scalar.c) */
                tamd_h_from_geodetic(latitude, longitude, elevation, ecef);
                return;
        }
        if (run4(&k_from_geodetic, 1, &latitude, &longitude, &elevation, NULL, 3, ecef,
                TURTLE_AMD_HOST))
                raise_void((turtle_function_t *)&turtle_ecef_from_geodetic);
}

void turtle_ecef_from_horizontal(double latitude, double longitude, double azimuth,
    double elevation, double direction[3])
{
        if (tamd_scalar_on_host()) {
                tamd_h_from_horizontal(latitude, longitude, azimuth, elevation, direction);
                return;
        }
        if (run4(&tamd_k_ecef_from_horizontal, 1, &latitude, &longitude, &azimuth,
                &elevation, 3, direction, TURTLE_AMD_HOST))
                raise_void((turtle_function_t *)&turtle_ecef_from_horizontal);
}

void turtle_ecef_to_geodetic(
    const double ecef[3], double * latitude, double * longitude, double * altitude)
{
        if (tamd_scalar_on_host()) {
                double la, lo, al;
                tamd_h_to_geodetic(ecef, &la, &lo, &al);
                if (latitude != NULL) *latitude = la;
                if (longitude != NULL) *longitude = lo;
                if (altitude != NULL) *altitude = al;
                return;
        }
        if (run_to_geodetic(1, ecef, latitude, longitude, altitude, TURTLE_AMD_HOST))
                raise_void((turtle_function_t *)&turtle_ecef_to_geodetic);
}

void turtle_ecef_to_horizontal(double latitude, double longitude,
    const double direction[3], double * azimuth, double * elevation)
{
        if (tamd_scalar_on_host()) {
                tamd_h_to_horizontal(latitude, longitude, direction, azimuth, elevation);
                return;
        }
        if (run_to_horizontal(1, &latitude, &longitude, direction, azimuth, elevation, TURTLE_AMD_HOST))
                raise_void((turtle_function_t *)&turtle_ecef_to_horizontal);
}
