/*
 * advance_exp_loop.c -- the CPU checker of turtle_stepper_advance_exp_n: the loop
 * that include/turtle_amd.h states (turtle_stepper_advance_n's loop with the density
 * of medium m falling as density[m] * exp(-h / scale_height[m]), the altitude taken
 * as linear in the path within a step) over the oracle's restatement of
 * turtle_stepper_step, one stepper per ray (a fresh history, kept for the ray's
 * steps).  Rays block-partitioned over pthreads.  Built by the tests against
 * oracle/libturtle_oracle.so, with -ffp-contract=off.
 */
#include <math.h>
#include <pthread.h>
#include <stdlib.h>

#include "turtle_oracle.h"

enum { SPENT = 0, DISTANCE = 1, LEFT = 2, CEILING = 3, MAX_STEPS = 4 };

struct job {
        const struct orc_geometry * geometry;
        double slope, resolution, ceiling;
        long begin, end;
        double * position;
        const double *direction, *density, *scale_height, *budget, *distance_max;
        int max_steps;
        int * index;
        double *depth, *distance;
        int *n_steps, *status;
};

/* S(f): the depth of the first f metres of a step whose density is c * exp(w * f) */
static double S(double c, double w, double f) { return (w * f == 0) ? c * f : c * expm1(w * f) / w; }

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
                const double B = j->budget[r];
                const double M = (j->distance_max != NULL) ? j->distance_max[r] : HUGE_VAL;
                double alt, ds, X = 0., d = 0.;
                int idx[2], steps = 0, status, i;
                orc_stepper_step(&s, pos, NULL, NULL, NULL, &alt, NULL, NULL, idx);
                for (;;) {
                        if (idx[0] < 0) { status = LEFT; break; }
                        if (!(X < B)) { status = SPENT; break; }
                        if (!(d < M)) { status = DISTANCE; break; }
                        if (!(alt < j->ceiling)) { status = CEILING; break; }
                        if (steps >= j->max_steps) { status = MAX_STEPS; break; }
                        const int m = idx[0], k = idx[1];
                        const double p0[3] = { pos[0], pos[1], pos[2] };
                        const double a0 = alt;
                        orc_stepper_step(&s, pos, dir, NULL, NULL, &alt, NULL, &ds, idx);
                        const double a1 = alt;
                        double c, w;
                        if ((j->scale_height == NULL) || (j->scale_height[m] == HUGE_VAL)) {
                                c = j->density[m], w = 0;
                        } else {
                                const double H = j->scale_height[m];
                                c = j->density[m] * exp(-a0 / H);
                                w = -((a1 - a0) / H) / ds;
                        }
                        const double x = S(c, w, ds);
                        const int spent = (X + x >= B), far = (d + ds >= M);
                        if (spent || far) { /* the step is cut short, inside medium m */
                                double f = ds;
                                status = SPENT;
                                if (far) f = M - d, status = DISTANCE;
                                if (spent) {
                                        const double fs = (w == 0) ? (B - X) / c : log1p((B - X) * w / c) / w;
                                        if (fs <= f) f = fs, status = SPENT;
                                }
                                if (f > ds) f = ds;
                                for (i = 0; i < 3; i++) {
                                        const double move = dir[i] * f;
                                        pos[i] = p0[i] + move;
                                }
                                if (status == SPENT)
                                        X = B, d += f;
                                else
                                        X += S(c, w, f), d = M;
                                steps++;
                                idx[0] = m, idx[1] = k;
                                break;
                        }
                        X += x, d += ds, steps++;
                }
                j->index[2 * r] = idx[0], j->index[2 * r + 1] = idx[1];
                j->depth[r] = X, j->distance[r] = d, j->n_steps[r] = steps, j->status[r] = status;
        }
        return NULL;
}

/* One ray's uncut run, step by step: path[i] and altitude[i] after step i (element 0: the origin)
 * and medium[i] of the medium step i + 1 began in, up to `capacity` steps (path and altitude hold
 * capacity + 1 elements).  -> the steps taken.
 * What the model's error is measured from (scripts/exp_advance_exp_model.py). */
int advance_exp_profile(const struct orc_geometry * geometry, double slope, double resolution,
    const double * position, const double * direction, double ceiling, int capacity, double * path,
    double * altitude, int * medium)
{
        struct orc_stepper s;
        orc_stepper_init(&s, geometry);
        s.slope_factor = slope;
        s.resolution_factor = resolution;
        s.local_range = 0.;
        double pos[3] = { position[0], position[1], position[2] };
        double alt, ds, d = 0.;
        int idx[2], steps = 0;
        orc_stepper_step(&s, pos, NULL, NULL, NULL, &alt, NULL, NULL, idx);
        path[0] = 0., altitude[0] = alt;
        while ((idx[0] >= 0) && (alt < ceiling) && (steps < capacity)) {
                medium[steps] = idx[0];
                orc_stepper_step(&s, pos, direction, NULL, NULL, &alt, NULL, &ds, idx);
                d += ds, steps++;
                path[steps] = d, altitude[steps] = alt;
        }
        return steps;
}

/* scale_height and distance_max may be NULL; every output is mandatory */
void advance_exp_loop(const struct orc_geometry * geometry, double slope, double resolution, long n,
    double * position, const double * direction, const double * density, const double * scale_height,
    const double * budget, const double * distance_max, double ceiling, int max_steps, int * index,
    double * depth, double * distance, int * n_steps, int * status, int threads)
{
        if (threads < 1) threads = 1;
        struct job * jobs = calloc(threads, sizeof(*jobs));
        pthread_t * tid = calloc(threads, sizeof(*tid));
        int t;
        for (t = 0; t < threads; t++) {
                struct job * j = &jobs[t];
                j->geometry = geometry, j->slope = slope, j->resolution = resolution, j->ceiling = ceiling;
                j->begin = n * t / threads, j->end = n * (t + 1) / threads;
                j->position = position, j->direction = direction, j->density = density;
                j->scale_height = scale_height;
                j->budget = budget, j->distance_max = distance_max, j->max_steps = max_steps;
                j->index = index, j->depth = depth, j->distance = distance;
                j->n_steps = n_steps, j->status = status;
                pthread_create(&tid[t], NULL, worker, j);
        }
        for (t = 0; t < threads; t++) pthread_join(tid[t], NULL);
        free(jobs);
        free(tid);
}
