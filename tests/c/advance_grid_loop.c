/*
 * advance_grid_loop.c -- the CPU checker of turtle_stepper_advance_grid_n: the loop
 * and the walk that include/turtle_amd.h state (turtle_stepper_advance_n's loop, one
 * walk through a box of voxels a step in the place of density[m] * ds and of the
 * cut) over the oracle's restatement of turtle_stepper_step, one stepper per ray (a
 * fresh history, kept for the ray's steps).  Rays block-partitioned over pthreads.
 * Built by the tests against oracle/libturtle_oracle.so, with -ffp-contract=off.
 */
#include <math.h>
#include <pthread.h>
#include <stdlib.h>

#include "turtle_oracle.h"

enum { SPENT = 0, DISTANCE = 1, LEFT = 2, CEILING = 3, MAX_STEPS = 4 };

/* struct turtle_amd_grid, field for field */
struct grid {
        double origin[3], axis[3][3], size[3];
        int n[3];
        int medium;
        const double * density;
};

/* what a walk met, for the tests that ask what a fixture holds */
enum { MET_VOXEL = 1, MET_FACE = 2 }; /* a voxel; the box's face in mid-step */

struct walk {
        double acc, R, f;
        int stopped, pieces;
};

static int piece(struct walk * w, double a, double b, double rho)
{
        const double x = rho * (b - a);
        w->pieces++;
        if ((x > 0) && (w->acc + x >= w->R)) {
                w->f = a + (w->R - w->acc) / rho;
                w->stopped = 1;
                return 1;
        }
        w->acc += x;
        return 0;
}

/* the pieces of [0, L] in order -> stopped; *x the depth of [0, L], *f where the walk ended */
int grid_depth(const struct grid * G, double rho_out, int m, const double * p0, const double * dir, double L,
    double R, double * x, double * f_out, int * pieces, int * met)
{
        struct walk w = { 0., R, L, 0, 0 };
        double f = 0;
        int flags = 0;
        if ((G != NULL) && (m == G->medium)) {
                double s[3], t[3], f0 = 0, f1 = L;
                int a, hit = 1;
                for (a = 0; a < 3; a++) {
                        s[a] = G->axis[a][0] * (p0[0] - G->origin[0]) + G->axis[a][1] * (p0[1] - G->origin[1]) +
                            G->axis[a][2] * (p0[2] - G->origin[2]);
                        t[a] = G->axis[a][0] * dir[0] + G->axis[a][1] * dir[1] + G->axis[a][2] * dir[2];
                }
                for (a = 0; a < 3; a++) {
                        const double E = G->n[a] * G->size[a];
                        if (t[a] == 0) {
                                if (!((s[a] >= 0) && (s[a] < E))) hit = 0;
                        } else {
                                double u = (0 - s[a]) / t[a], v = (E - s[a]) / t[a];
                                if (u > v) {
                                        const double swap = u;
                                        u = v, v = swap;
                                }
                                if (u > f0) f0 = u;
                                if (v < f1) f1 = v;
                        }
                }
                if (hit && (f0 < f1)) {
                        int i[3];
                        double next[3];
                        flags |= MET_VOXEL | (((f0 > 0) || (f1 < L)) ? MET_FACE : 0);
                        if (piece(&w, 0, f0, rho_out)) goto done;
                        for (a = 0; a < 3; a++) {
                                const double c = floor((s[a] + f0 * t[a]) / G->size[a]);
                                i[a] = (c > 0) ? ((c < G->n[a] - 1) ? (int)c : G->n[a] - 1) : 0;
                                next[a] = (t[a] == 0) ? HUGE_VAL : ((i[a] + (t[a] > 0)) * G->size[a] - s[a]) / t[a];
                        }
                        f = f0;
                        for (;;) {
                                a = ((next[0] <= next[1]) && (next[0] <= next[2])) ? 0 : ((next[1] <= next[2]) ? 1 : 2);
                                double g = (next[a] < f1) ? next[a] : f1;
                                if (g < f) g = f;
                                if (piece(&w, f, g, G->density[((long)i[2] * G->n[1] + i[1]) * G->n[0] + i[0]])) goto done;
                                f = g;
                                if (!(next[a] < f1)) break;
                                i[a] += (t[a] > 0) ? 1 : -1;
                                if ((i[a] < 0) || (i[a] >= G->n[a])) break;
                                next[a] = ((i[a] + (t[a] > 0)) * G->size[a] - s[a]) / t[a];
                        }
                }
        }
        piece(&w, f, L, rho_out);
done:
        *x = w.acc, *f_out = w.f;
        if (pieces != NULL) *pieces += w.pieces;
        if (met != NULL) *met = flags;
        return w.stopped;
}

/* n segments at once, for the tests of the walk alone: stopped[r], x[r], f[r] */
void grid_depth_n(const struct grid * G, long n, const double * rho_out, const int * m, const double * p0,
    const double * dir, const double * L, const double * R, double * x, double * f, int * stopped)
{
        long r;
        for (r = 0; r < n; r++)
                stopped[r] = grid_depth(G, rho_out[r], m[r], p0 + 3 * r, dir + 3 * r, L[r], R[r], &x[r], &f[r], NULL, NULL);
}

struct job {
        const struct orc_geometry * geometry;
        const struct grid * grid;
        double slope, resolution, ceiling;
        long begin, end;
        double * position;
        const double *direction, *density, *budget, *distance_max;
        int max_steps;
        int * index;
        double *depth, *distance;
        int *n_steps, *status;
        int * tally; /* [n][4] or NULL: steps begun in the grid's medium, those that met a voxel, those
                      * that met a face of the box in mid-step, pieces */
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
                const double B = j->budget[r];
                const double M = (j->distance_max != NULL) ? j->distance_max[r] : HUGE_VAL;
                double alt, ds, X = 0., d = 0.;
                int idx[2], steps = 0, status, i;
                int tally[4] = { 0, 0, 0, 0 };
                orc_stepper_step(&s, pos, NULL, NULL, NULL, &alt, NULL, NULL, idx);
                for (;;) {
                        if (idx[0] < 0) { status = LEFT; break; }
                        if (!(X < B)) { status = SPENT; break; }
                        if (!(d < M)) { status = DISTANCE; break; }
                        if (!(alt < j->ceiling)) { status = CEILING; break; }
                        if (steps >= j->max_steps) { status = MAX_STEPS; break; }
                        const int m = idx[0], k = idx[1];
                        const double p0[3] = { pos[0], pos[1], pos[2] };
                        orc_stepper_step(&s, pos, dir, NULL, NULL, &alt, NULL, &ds, idx);
                        const int far = (d + ds >= M);
                        double L = far ? M - d : ds, x, f;
                        int met;
                        if (L > ds) L = ds;
                        const int stopped = grid_depth(j->grid, j->density[m], m, p0, dir, L, B - X, &x, &f, &tally[3], &met);
                        if ((j->grid != NULL) && (m == j->grid->medium))
                                tally[0]++, tally[1] += (met & MET_VOXEL) ? 1 : 0, tally[2] += (met & MET_FACE) ? 1 : 0;
                        if (stopped || far) { /* the step is cut short, inside medium m */
                                const double at = stopped ? f : L;
                                for (i = 0; i < 3; i++) {
                                        const double move = dir[i] * at;
                                        pos[i] = p0[i] + move;
                                }
                                if (stopped)
                                        X = B, d += f, status = SPENT;
                                else
                                        X += x, d = M, status = DISTANCE;
                                steps++;
                                idx[0] = m, idx[1] = k;
                                break;
                        }
                        X += x, d += ds, steps++;
                }
                j->index[2 * r] = idx[0], j->index[2 * r + 1] = idx[1];
                j->depth[r] = X, j->distance[r] = d, j->n_steps[r] = steps, j->status[r] = status;
                if (j->tally != NULL)
                        for (i = 0; i < 4; i++) j->tally[4 * r + i] = tally[i];
        }
        return NULL;
}

/* grid, distance_max and tally may be NULL; every other output is mandatory */
void advance_grid_loop(const struct orc_geometry * geometry, double slope, double resolution, long n,
    double * position, const double * direction, const double * density, const struct grid * grid,
    const double * budget, const double * distance_max, double ceiling, int max_steps, int * index,
    double * depth, double * distance, int * n_steps, int * status, int * tally, int threads)
{
        if (threads < 1) threads = 1;
        struct job * jobs = calloc(threads, sizeof(*jobs));
        pthread_t * tid = calloc(threads, sizeof(*tid));
        int t;
        for (t = 0; t < threads; t++) {
                struct job * j = &jobs[t];
                j->geometry = geometry, j->grid = grid, j->slope = slope, j->resolution = resolution;
                j->ceiling = ceiling;
                j->begin = n * t / threads, j->end = n * (t + 1) / threads;
                j->position = position, j->direction = direction, j->density = density;
                j->budget = budget, j->distance_max = distance_max, j->max_steps = max_steps;
                j->index = index, j->depth = depth, j->distance = distance;
                j->n_steps = n_steps, j->status = status, j->tally = tally;
                pthread_create(&tid[t], NULL, worker, j);
        }
        for (t = 0; t < threads; t++) pthread_join(tid[t], NULL);
        free(jobs);
        free(tid);
}
