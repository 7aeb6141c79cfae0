/*
 * crossings_loop.c -- the CPU checker of turtle_stepper_crossings_n: the loop of
 * tests/c/traverse_loop.c (the reference's examples/example-stepper.c:128-140
 * over the oracle's restatement of turtle_stepper_step, one stepper per ray)
 * that also records every crossing: where the step that changed the medium
 * left the ray, the path summed up to there, and the pair {medium left, medium
 * entered}.  The crossings go out ragged: ray r's are rows offset[r] ..
 * offset[r + 1] - 1 of point / distance / media, offset[] being the caller's
 * (an exclusive prefix sum of a first run's counts).  Built by the tests
 * against oracle/libturtle_oracle.so.
 */
#include <pthread.h>
#include <stdlib.h>

#include "turtle_oracle.h"

struct job {
        const struct orc_geometry * geometry;
        double slope, resolution, ceiling;
        long n, begin, end;
        double * position;
        const double * direction;
        int max_steps;
        int * index;
        double * length; /* [media][n] */
        int *n_steps, *n_crossings;
        const long * offset;
        double *point, *distance; /* [rows][3], [rows] */
        int * media;              /* [rows][2] */
};

static void * worker(void * p)
{
        struct job * j = p;
        long r;
        for (r = j->begin; r < j->end; r++) {
                struct orc_stepper s;
                orc_stepper_init(&s, j->geometry);
                s.slope_factor = j->slope;
                s.resolution_factor = j->resolution;
                s.local_range = 0.;
                double * pos = j->position + 3 * r;
                const double * dir = j->direction + 3 * r;
                double alt, ds, d = 0.;
                int idx[2], steps = 0, crossings = 0;
                orc_stepper_step(&s, pos, NULL, NULL, NULL, &alt, NULL, NULL, idx);
                while ((idx[0] >= 0) && (alt < j->ceiling) && (steps < j->max_steps)) {
                        const int m = idx[0];
                        orc_stepper_step(&s, pos, dir, NULL, NULL, &alt, NULL, &ds, idx);
                        j->length[m * j->n + r] += ds;
                        d += ds;
                        steps++;
                        if (idx[0] != m) {
                                const int c = crossings++;
                                if ((j->offset != NULL) && (j->offset[r] + c < j->offset[r + 1])) {
                                        const long row = j->offset[r] + c;
                                        j->point[3 * row] = pos[0], j->point[3 * row + 1] = pos[1];
                                        j->point[3 * row + 2] = pos[2];
                                        j->distance[row] = d;
                                        j->media[2 * row] = m, j->media[2 * row + 1] = idx[0];
                                }
                        }
                }
                j->index[2 * r] = idx[0], j->index[2 * r + 1] = idx[1];
                j->n_steps[r] = steps, j->n_crossings[r] = crossings;
        }
        return NULL;
}

/* length: [media][n], zeroed by the caller.  offset: [n + 1], ray r's rows are offset[r] ..
 * offset[r + 1] - 1 (the crossings beyond them are counted, not stored); or NULL: counts only,
 * point, distance and media are not touched. */
void crossings_loop(const struct orc_geometry * geometry, double slope, double resolution, long n,
    double * position, const double * direction, double ceiling, int max_steps, int * index,
    double * length, int * n_steps, int * n_crossings, const long * offset, double * point,
    double * distance, int * media, int threads)
{
        if (threads < 1) threads = 1;
        struct job * jobs = calloc(threads, sizeof(*jobs));
        pthread_t * tid = calloc(threads, sizeof(*tid));
        int t;
        for (t = 0; t < threads; t++) {
                struct job * j = &jobs[t];
                j->geometry = geometry, j->slope = slope, j->resolution = resolution;
                j->ceiling = ceiling, j->n = n;
                j->begin = n * t / threads, j->end = n * (t + 1) / threads;
                j->position = position, j->direction = direction, j->max_steps = max_steps;
                j->index = index, j->length = length, j->n_steps = n_steps, j->n_crossings = n_crossings;
                j->offset = offset, j->point = point, j->distance = distance, j->media = media;
                pthread_create(&tid[t], NULL, worker, j);
        }
        for (t = 0; t < threads; t++) pthread_join(tid[t], NULL);
        free(jobs);
        free(tid);
}
