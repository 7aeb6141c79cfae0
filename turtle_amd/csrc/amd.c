/*
 * amd.c -- device/stream management and the tally reduction of the batch
 * extension (turtle_amd_* in turtle_amd.h).
 */
#include "host.h"

int turtle_amd_device_count(void) { return tamd_dev_count(); }

enum turtle_return turtle_amd_device_set(int device)
{
        TAMD_ERROR_INIT(&turtle_amd_device_set);
        /* the calling THREAD's device from here on: its steppers rebuild their tables
         * there at their next call, maps and tiles get a copy there when first needed */
        if (tamd_dev_select(device)) return TAMD_RAISE_DEVICE();
        return TURTLE_RETURN_SUCCESS;
}

int turtle_amd_device_get(void) { return tamd_dev_current(); }

void turtle_amd_thread_release(void) { tamd_dev_release(); }

enum turtle_return turtle_amd_stream_set(void * hip_stream)
{
        TAMD_ERROR_INIT(&turtle_amd_stream_set);
        if (tamd_dev_stream_set(hip_stream)) return TAMD_RAISE_DEVICE();
        return TURTLE_RETURN_SUCCESS;
}

enum turtle_return turtle_amd_synchronize(void)
{
        TAMD_ERROR_INIT(&turtle_amd_synchronize);
        if (tamd_dev_sync()) return TAMD_RAISE_DEVICE();
        return TURTLE_RETURN_SUCCESS;
}

int turtle_amd_compute_units(void) { return tamd_dev_cus(); }

void turtle_amd_in_flight_set(int batches) { tamd_dev_in_flight_set(batches); }

int turtle_amd_in_flight_get(void) { return tamd_dev_in_flight_get(); }

void turtle_amd_math_set(int mode) { tamd_dev_math_set(mode == TURTLE_AMD_MATH_STRICT); }

int turtle_amd_math_get(void)
{
        return tamd_dev_math_get() ? TURTLE_AMD_MATH_STRICT : TURTLE_AMD_MATH_FAST;
}

enum turtle_return turtle_amd_tally_n(long n, const int * index, const double * length,
    int n_media, unsigned long long * hits, int n_bins, double length_max,
    unsigned long long * histogram, int space)
{
        TAMD_ERROR_INIT(&turtle_amd_tally_n);
        if ((index == NULL) || (length == NULL) || (hits == NULL) || (histogram == NULL))
                return TAMD_RAISE(TURTLE_RETURN_BAD_ADDRESS, "invalid null argument");
        if ((n_media < 0) || (n_bins < 1) || !(length_max > 0.))
                return TAMD_RAISE(TURTLE_RETURN_DOMAIN_ERROR, "invalid input parameter(s)");
        struct tamd_stage st = { 0 };
        void *dix, *dlen, *dh, *dg;
        tamd_stage_add(&st, index, 2 * (size_t)n * sizeof(int), TAMD_IN, &dix);
        tamd_stage_add(&st, length, (size_t)n * sizeof(double), TAMD_IN, &dlen);
        tamd_stage_add(&st, hits, (size_t)(n_media + 1) * sizeof(*hits), TAMD_INOUT, &dh);
        tamd_stage_add(&st, histogram, (size_t)(n_bins + 1) * sizeof(*histogram), TAMD_INOUT, &dg);
        if (tamd_stage_open(&st, space) ||
            tamd_k_tally(n, dix, dlen, n_media, dh, n_bins, length_max, dg) || tamd_stage_close(&st))
                return TAMD_RAISE_DEVICE();
        return TURTLE_RETURN_SUCCESS;
}

enum turtle_return turtle_amd_philox_n(long n, unsigned long long seed,
    unsigned long long stream, long first_ray, unsigned int * words, int space)
{
        TAMD_ERROR_INIT(&turtle_amd_philox_n);
        struct tamd_stage st = { 0 };
        void * dw;
        if (words == NULL) return TAMD_RAISE(TURTLE_RETURN_BAD_ADDRESS, "invalid null argument");
        tamd_stage_add(&st, words, (size_t)n * 4 * sizeof(unsigned int), TAMD_OUT, &dw);
        if (tamd_stage_open(&st, space) || tamd_k_philox(n, seed, stream, first_ray, dw) ||
            tamd_stage_close(&st))
                return TAMD_RAISE_DEVICE();
        return TURTLE_RETURN_SUCCESS;
}

enum turtle_return turtle_amd_isotropic_n(long n, unsigned long long seed,
    unsigned long long stream, long first_ray, double * direction, int space)
{
        TAMD_ERROR_INIT(&turtle_amd_isotropic_n);
        struct tamd_stage st = { 0 };
        void * dd;
        if (direction == NULL)
                return TAMD_RAISE(TURTLE_RETURN_BAD_ADDRESS, "invalid null argument");
        tamd_stage_add(&st, direction, (size_t)n * 3 * sizeof(double), TAMD_OUT, &dd);
        if (tamd_stage_open(&st, space) || tamd_k_isotropic(n, seed, stream, first_ray, dd) ||
            tamd_stage_close(&st))
                return TAMD_RAISE_DEVICE();
        return TURTLE_RETURN_SUCCESS;
}
