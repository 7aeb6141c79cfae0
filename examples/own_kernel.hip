/*
 * own_kernel.hip -- the stepper inside the caller's own kernel (include/turtle_amd_device.h).
 *
 * A muon-like walk over a stack of tiles: every ray carries an energy; a step costs energy by
 * the medium it was taken in; after every step the direction is deflected by a small angle from
 * the caller's own generator; a ray ends when its energy is spent, when it leaves the data, or
 * after max_steps steps.  The same physics twice:
 *   (b) one launch on turtle_amd_device::Stepping: the ray's state stays in registers;
 *   (a) generation by generation, as a caller writes it without the device API:
 *       turtle_stepper_walk_n for the step, then one physics kernel, per generation.
 * Both give every ray the same fate in the STRICT arithmetic (checked), and are timed.
 *
 *   hipcc --offload-arch=gfx950 -ffp-contract=off -O3 -std=c++17 -I include examples/own_kernel.hip \
 *         -L turtle_amd -lturtle_amd -Wl,-rpath,$PWD/turtle_amd -o own_kernel
 *   ./own_kernel <directory of tiles> [rays = 1000000] [max_steps = 256] [repeats = 5] [south = 45] [west = 3]
 */
#include <cstdio>
#include <cstdlib>
#include <chrono>

#include "turtle_amd.h"
#include "turtle_amd_device.h"

using namespace turtle_amd_device;

#define MATH STRICT /* the arithmetic of both forms (turtle_amd_math_set below) */

/* ---- the caller's physics ------------------------------------------------------- */

struct Physics {
        double loss[2]; /* energy per metre in medium 0 (rock) and 1 (air) */
        double theta;   /* deflection per step, radians per sqrt(metre) / energy */
        int max_steps;
};

/* the caller's own generator: a hash of (ray, step) to three numbers in [-1, 1) */
__device__ __forceinline__ void noise(unsigned long long ray, unsigned step, double g[3])
{
        unsigned long long x = ray * 0x9E3779B97F4A7C15ull + step * 0xBF58476D1CE4E5B9ull + 0x94D049BB133111EBull;
        for (int i = 0; i < 3; i++) {
                x ^= x >> 30, x *= 0xBF58476D1CE4E5B9ull, x ^= x >> 27, x *= 0x94D049BB133111EBull, x ^= x >> 31;
                g[i] = (double)(long long)(x >> 11) * (1. / 4503599627370496.) - 1.;
        }
}

/* One step of `length` metres was taken in `medium`: the energy it cost and the deflected
 * direction.  false: the ray ends. */
__device__ __forceinline__ bool physics(const Physics & ph, unsigned long long ray, int count, int medium,
    double length, double & energy, double d[3])
{
        energy -= ph.loss[medium > 1 ? 1 : medium] * length;
        if (!(energy > 0.) || (count >= ph.max_steps)) return false;
        double g[3];
        noise(ray, (unsigned)count, g);
        const double along = g[0] * d[0] + g[1] * d[1] + g[2] * d[2];
        const double t = ph.theta * sqrt(length) / energy;
        double e[3];
        for (int i = 0; i < 3; i++) e[i] = d[i] + t * (g[i] - along * d[i]);
        const double norm = sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
        for (int i = 0; i < 3; i++) d[i] = e[i] / norm;
        return true;
}

/* ---- (b) the whole walk in one launch ------------------------------------------- */

template <int MODE>
__global__ void __launch_bounds__(256) walk_in_one(turtle_amd_view view, long n, const double * __restrict__ pos0,
    const double * __restrict__ dir0, double energy0, Physics ph, int * __restrict__ medium, int * __restrict__ steps,
    double * __restrict__ energy_out)
{
        const Geometry<MODE, MATH> geo(view);
        const long stride = (long)gridDim.x * blockDim.x;
        for (long r0 = (long)blockIdx.x * blockDim.x; r0 < n; r0 += stride) {
                const long r = r0 + threadIdx.x;
                Stepping<MODE, MATH> ray;
                double energy = energy0;
                int count = 0;
                if (r < n) ray.start(pos0 + 3 * r, dir0 + 3 * r);
                /* every ray ends: max_steps steps of at most 1201 halvings each, and the origin */
                const long limit = 2 + (long)ph.max_steps * 1203;
                for (long trips = 0; (__ballot(ray.live) != 0) && (trips < limit); trips++) {
                        const int event = ray.trip(geo); /* one sample for every live lane */
                        if ((event == NONE) || (event == ORIGIN)) continue;
                        bool on = false;
                        if (ray.from >= 0) { /* (else: it began outside the data) */
                                count++;
                                on = physics(ph, (unsigned long long)r, count, ray.from, ray.length, energy, ray.d);
                        }
                        if (!on || (event == LEFT)) {
                                medium[r] = ray.index[0], steps[r] = count, energy_out[r] = energy;
                                ray.stop();
                        }
                }
        }
}

/* ---- (a) a physics kernel per generation, after turtle_stepper_walk_n -------------- */

__global__ void physics_per_generation(long n, Physics ph, const double * __restrict__ step, int * __restrict__ index,
    double * __restrict__ dir, double * __restrict__ energy, int * __restrict__ medium, int * __restrict__ steps,
    int * __restrict__ live)
{
        const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
        if ((r >= n) || (medium[r] < 0) || (steps[r] < 0)) return; /* steps < 0: ended, -(count) - 1 */
        const int from = medium[r], count = steps[r] + 1;
        double d[3] = { dir[3 * r], dir[3 * r + 1], dir[3 * r + 2] }, e = energy[r];
        const bool on = physics(ph, (unsigned long long)r, count, from, step[r], e, d);
        energy[r] = e, medium[r] = index[2 * r];
        dir[3 * r] = d[0], dir[3 * r + 1] = d[1], dir[3 * r + 2] = d[2];
        if (!on || (index[2 * r] < 0)) {
                steps[r] = -count - 1;
                index[2 * r] = -1; /* walk_n steps it no further */
        } else {
                steps[r] = count;
                *live = 1;
        }
}

/* ---- host ------------------------------------------------------------------------- */

#define HIP(call)                                                                               \
        do {                                                                                    \
                const hipError_t e_ = (call);                                                   \
                if (e_ != hipSuccess) {                                                         \
                        fprintf(stderr, "%s: %s\n", #call, hipGetErrorString(e_));              \
                        exit(1);                                                                \
                }                                                                               \
        } while (0)
#define TURTLE(call)                                                                            \
        do {                                                                                    \
                if ((call) != TURTLE_RETURN_SUCCESS) exit(1); /* (the default handler has printed why) */ \
        } while (0)

static double now(void)
{
        return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

int main(int argc, char ** argv)
{
        if (argc < 2) {
                fprintf(stderr, "usage: %s <directory of tiles> [rays] [max_steps] [repeats] [south] [west]\n", argv[0]);
                return 2;
        }
        const long n = (argc > 2) ? atol(argv[2]) : 1000000;
        const Physics ph = { { 5e-4, 2e-7 }, 2e-3, (argc > 3) ? atoi(argv[3]) : 256 };
        const int repeats = (argc > 4) ? atoi(argv[4]) : 5;
        const double energy0 = 1.;

        struct turtle_stack * stack;
        struct turtle_stepper * stepper;
        TURTLE(turtle_stack_create(&stack, argv[1], 0, NULL, NULL));
        TURTLE(turtle_stepper_create(&stepper));
        TURTLE(turtle_stepper_add_stack(stepper, stack, 0.));
        turtle_amd_math_set(MATH == STRICT ? TURTLE_AMD_MATH_STRICT : TURTLE_AMD_MATH_FAST);

        /* the rays: 20 m above the ground over the middle of the first tile, isotropic directions */
        double *lat, *lon, *h, *pos0, *dir0, *pos, *dir, *next, *step, *energy, *energy_b;
        int *index, *di, *medium, *steps, *medium_b, *steps_b, *live;
        HIP(hipMalloc(&lat, n * 8)); HIP(hipMalloc(&lon, n * 8)); HIP(hipMalloc(&h, n * 8));
        HIP(hipMalloc(&pos0, 3 * n * 8)); HIP(hipMalloc(&dir0, 3 * n * 8)); HIP(hipMalloc(&pos, 3 * n * 8));
        HIP(hipMalloc(&dir, 3 * n * 8)); HIP(hipMalloc(&next, n * 8)); HIP(hipMalloc(&step, n * 8));
        HIP(hipMalloc(&energy, n * 8)); HIP(hipMalloc(&energy_b, n * 8)); HIP(hipMalloc(&index, 2 * n * 4));
        HIP(hipMalloc(&di, n * 4)); HIP(hipMalloc(&medium, n * 4)); HIP(hipMalloc(&steps, n * 4));
        HIP(hipMalloc(&medium_b, n * 4)); HIP(hipMalloc(&steps_b, n * 4)); HIP(hipMalloc(&live, 4));
        {
                double * hl = (double *)malloc(3 * n * 8);
                /* over the middle of the 1 x 1 degree tile whose south-west corner the command line
                 * names (45 N, 3 E) */
                const double south = (argc > 5) ? atof(argv[5]) : 45., west = (argc > 6) ? atof(argv[6]) : 3.;
                unsigned long long x = 88172645463325252ull;
                for (long r = 0; r < 3 * n; r++) {
                        x ^= x << 13, x ^= x >> 7, x ^= x << 17;
                        const double u = (double)(x >> 11) * (1. / 9007199254740992.);
                        hl[r] = (r < n) ? south + 0.25 + 0.5 * u : ((r < 2 * n) ? west + 0.25 + 0.5 * u : 20.);
                }
                HIP(hipMemcpy(lat, hl, n * 8, hipMemcpyHostToDevice));
                HIP(hipMemcpy(lon, hl + n, n * 8, hipMemcpyHostToDevice));
                HIP(hipMemcpy(h, hl + 2 * n, n * 8, hipMemcpyHostToDevice));
                free(hl);
        }
        TURTLE(turtle_stepper_position_n(stepper, n, lat, lon, h, 0, pos0, di, TURTLE_AMD_DEVICE));
        TURTLE(turtle_amd_isotropic_n(n, 2026, 0, 0, dir0, TURTLE_AMD_DEVICE));
        TURTLE(turtle_amd_synchronize());

        const int blocks = (int)((n + 255) / 256 < 8192 ? (n + 255) / 256 : 8192);
        double best_a = 1e30, best_b = 1e30;
        long total_steps = 0;
        for (int rep = 0; rep <= repeats; rep++) { /* (the first round warms up) */
                /* (a) generation by generation */
                HIP(hipMemcpy(pos, pos0, 3 * n * 8, hipMemcpyDeviceToDevice));
                HIP(hipMemcpy(dir, dir0, 3 * n * 8, hipMemcpyDeviceToDevice));
                HIP(hipMemset(steps, 0, n * 4));
                {
                        double * e = (double *)malloc(n * 8);
                        for (long r = 0; r < n; r++) e[r] = energy0;
                        HIP(hipMemcpy(energy, e, n * 8, hipMemcpyHostToDevice));
                        free(e);
                }
                HIP(hipDeviceSynchronize());
                double t0 = now();
                TURTLE(turtle_stepper_walk_n(stepper, n, pos, NULL, next, NULL, index, TURTLE_AMD_DEVICE));
                TURTLE(turtle_amd_synchronize());
                HIP(hipMemcpy2D(medium, 4, index, 8, 4, n, hipMemcpyDeviceToDevice)); /* index[r][0] */
                for (int g = 0; g < ph.max_steps; g++) {
                        int any = 0;
                        TURTLE(turtle_stepper_walk_n(stepper, n, pos, dir, next, step, index, TURTLE_AMD_DEVICE));
                        TURTLE(turtle_amd_synchronize());
                        HIP(hipMemset(live, 0, 4));
                        physics_per_generation<<<(unsigned)((n + 255) / 256), 256>>>(n, ph, step, index, dir, energy, medium,
                            steps, live);
                        HIP(hipMemcpy(&any, live, 4, hipMemcpyDeviceToHost));
                        if (!any) break;
                }
                const double ta = now() - t0;

                /* (b) one launch on the device API */
                turtle_amd_view view;
                TURTLE(turtle_amd_stepper_view_acquire(stepper, &view, sizeof(view)));
                HIP(hipDeviceSynchronize());
                t0 = now();
                const bool known = dispatch(view, [&](auto mode) {
                        walk_in_one<decltype(mode)::value><<<blocks, 256>>>(view, n, pos0, dir0, energy0, ph, medium_b,
                            steps_b, energy_b);
                });
                HIP(hipGetLastError());
                HIP(hipDeviceSynchronize()); /* the kernel has FINISHED before the release */
                const double tb = now() - t0;
                TURTLE(turtle_amd_stepper_view_release(stepper));
                if (!known) {
                        fprintf(stderr, "the view is not this header's\n");
                        return 1;
                }

                if (rep == 0) { /* the same fate, ray by ray */
                        int *ma = (int *)malloc(n * 4), *sa = (int *)malloc(n * 4), *mb = (int *)malloc(n * 4),
                            *sb = (int *)malloc(n * 4);
                        HIP(hipMemcpy(ma, medium, n * 4, hipMemcpyDeviceToHost));
                        HIP(hipMemcpy(sa, steps, n * 4, hipMemcpyDeviceToHost));
                        HIP(hipMemcpy(mb, medium_b, n * 4, hipMemcpyDeviceToHost));
                        HIP(hipMemcpy(sb, steps_b, n * 4, hipMemcpyDeviceToHost));
                        long differ = 0;
                        total_steps = 0;
                        for (long r = 0; r < n; r++) {
                                const int count = (sa[r] < 0) ? -sa[r] - 1 : sa[r];
                                differ += ((count != sb[r]) || (ma[r] != mb[r])) ? 1 : 0;
                                total_steps += sb[r];
                        }
                        printf("%ld rays, %ld steps; rays whose fate differs between the two forms: %ld\n", n, total_steps,
                            differ);
                        free(ma), free(sa), free(mb), free(sb);
                        if ((MATH == STRICT) && (differ != 0)) return 1;
                        continue;
                }
                if (ta < best_a) best_a = ta;
                if (tb < best_b) best_b = tb;
        }
        if (repeats > 0)
                printf("(a) walk_n + a physics kernel per generation: %.2f ms, %.3g ray-steps/s\n"
                       "(b) Stepping in one launch:                  %.2f ms, %.3g ray-steps/s\n",
                    1e3 * best_a, total_steps / best_a, 1e3 * best_b, total_steps / best_b);
        turtle_stepper_destroy(&stepper);
        turtle_stack_destroy(&stack);
        return 0;
}
