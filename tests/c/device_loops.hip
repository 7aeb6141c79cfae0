/*
 * device_loops.hip -- test kernels written on include/turtle_amd_device.h alone, as a caller
 * of the device API would write them, with extern "C" launchers for the tests
 * (tests/test_device_api.py, tests/test_gpu_device_api.py).  All pointers are DEVICE pointers;
 * `view` is what turtle_amd_stepper_view_acquire filled.  Every ray loop is bounded: by
 * max_steps, and by the halving guard of the API (1200 halvings a crossing).
 *
 * Build: hipcc --offload-arch=gfx950 -ffp-contract=off -I include -shared -fPIC
 */
#include "turtle_amd_device.h"

using namespace turtle_amd_device;

extern "C" int loops_view_version(void) { return TURTLE_AMD_VIEW_VERSION; }
extern "C" long loops_view_size(void) { return (long)sizeof(turtle_amd_view); }

/* what a traverse writes, as turtle_stepper_traverse_n does */
struct TraverseOut {
        double * pos;     /* [n][3], in: the origins */
        int * index;      /* [n][2] */
        double * length;  /* [media][n], zeroed by the caller */
        int * n_steps;    /* [n] */
        int * n_cross;    /* [n] */
};

/* the most trips a ray can take: every step a crossing, every crossing halved to the guard */
__device__ __forceinline__ long trip_limit(int max_steps) { return 2 + (long)max_steps * 1203; }

/* The loop of turtle_stepper_traverse_n's header comment on Stepping::trip(): one sample per
 * live lane and trip, the path summed per medium (the sum of the medium left goes out at a
 * crossing, the new medium's comes in: the library's order of additions). */
template <int MODE, int MATH>
__global__ void __launch_bounds__(256) traverse_trip(turtle_amd_view view, long n, const double * __restrict__ dir,
    double ceiling, int max_steps, TraverseOut out)
{
        const Geometry<MODE, MATH> geo(view);
        const long stride = (long)gridDim.x * blockDim.x;
        for (long r0 = (long)blockIdx.x * blockDim.x; r0 < n; r0 += stride) { /* (wave-uniform) */
                const long r = r0 + threadIdx.x;
                Stepping<MODE, MATH> ray;
                double len = 0.;
                int count = 0, crossings = 0;
                if (r < n) ray.start(out.pos + 3 * r, dir + 3 * r);
                const long limit = trip_limit(max_steps);
                for (long trips = 0; (__ballot(ray.live) != 0) && (trips < limit); trips++) {
                        const int event = ray.trip(geo);
                        if (event == NONE) continue;
                        if (event == STEP) len += ray.length, count++;
                        if ((event == CROSSING) || ((event == LEFT) && (ray.from >= 0))) {
                                len += ray.length;
                                out.length[(long)ray.from * n + r] = len;
                                len = (ray.index[0] >= 0) ? out.length[(long)ray.index[0] * n + r] : 0.;
                                crossings++, count++;
                        }
                        const bool low = (ray.index[0] >= 0) && (ray.altitude < ceiling);
                        if (!low || (count >= max_steps)) {
                                out.pos[3 * r] = ray.x[0], out.pos[3 * r + 1] = ray.x[1], out.pos[3 * r + 2] = ray.x[2];
                                out.index[2 * r] = ray.index[0], out.index[2 * r + 1] = ray.index[1];
                                if (ray.index[0] >= 0) out.length[(long)ray.index[0] * n + r] = len;
                                out.n_steps[r] = count, out.n_cross[r] = crossings;
                                ray.stop();
                        }
                }
        }
}

/* the same loop on the simple step(): a whole turtle_stepper_step per call */
template <int MODE, int MATH>
__global__ void __launch_bounds__(256) traverse_step(turtle_amd_view view, long n, const double * __restrict__ dir,
    double ceiling, int max_steps, TraverseOut out)
{
        const Geometry<MODE, MATH> geo(view);
        const long stride = (long)gridDim.x * blockDim.x;
        for (long r = (long)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += stride) {
                double pos[3] = { out.pos[3 * r], out.pos[3 * r + 1], out.pos[3 * r + 2] };
                const double d[3] = { dir[3 * r], dir[3 * r + 1], dir[3 * r + 2] };
                State st;
                sample(geo, pos, st);
                double len = 0.;
                int count = 0, crossings = 0;
                while ((st.index[0] >= 0) && (st.altitude < ceiling) && (count < max_steps)) {
                        const int m = st.index[0];
                        step(geo, st, pos, d);
                        len += st.step_length, count++;
                        if (st.index[0] != m) {
                                out.length[(long)m * n + r] = len;
                                len = (st.index[0] >= 0) ? out.length[(long)st.index[0] * n + r] : 0.;
                                crossings++;
                        }
                }
                out.pos[3 * r] = pos[0], out.pos[3 * r + 1] = pos[1], out.pos[3 * r + 2] = pos[2];
                out.index[2 * r] = st.index[0], out.index[2 * r + 1] = st.index[1];
                if (st.index[0] >= 0) out.length[(long)st.index[0] * n + r] = len;
                out.n_steps[r] = count, out.n_cross[r] = crossings;
        }
}

/* sample() at the origin, then `k_steps` times step(), every step recorded: rec[(k * n + r) * 11]
 * = position (3), step, latitude, longitude, altitude, elevation (2), index (2, as doubles);
 * taken[r]: the steps the ray took before it left the data */
template <int MODE, int MATH>
__global__ void __launch_bounds__(256) records(turtle_amd_view view, long n, const double * __restrict__ pos0,
    const double * __restrict__ dir, int k_steps, double * __restrict__ rec, int * __restrict__ taken)
{
        const Geometry<MODE, MATH> geo(view);
        const long stride = (long)gridDim.x * blockDim.x;
        for (long r = (long)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += stride) {
                double pos[3] = { pos0[3 * r], pos0[3 * r + 1], pos0[3 * r + 2] };
                const double d[3] = { dir[3 * r], dir[3 * r + 1], dir[3 * r + 2] };
                State st;
                sample(geo, pos, st);
                int k = 0;
                for (; k < k_steps; k++) {
                        if (!step(geo, st, pos, d)) break;
                        double * o = rec + ((long)k * n + r) * 11;
                        o[0] = pos[0], o[1] = pos[1], o[2] = pos[2], o[3] = st.step_length;
                        o[4] = st.latitude, o[5] = st.longitude, o[6] = st.altitude;
                        o[7] = st.elevation[0], o[8] = st.elevation[1];
                        o[9] = (double)st.index[0], o[10] = (double)st.index[1];
                }
                taken[r] = k;
        }
}

/* turtle_stepper_scatter_n in the caller's kernel: each ray resumed from its sample (altitude,
 * elevation, index), `n_steps` generations, the direction of generation g from
 * isotropic(first + r, first_step + g; seed) */
struct WalkState {
        double * pos;    /* [n][3] */
        double * alt;    /* [n] */
        double * elev;   /* [n][2] */
        int * index;     /* [n][2] */
        double * length; /* [n], += */
        int * steps;     /* [n], += */
};

template <int MODE, int MATH>
__global__ void __launch_bounds__(256) walk(turtle_amd_view view, long n, unsigned long long seed, long first,
    int first_step, int n_steps, WalkState w)
{
        const Geometry<MODE, MATH> geo(view);
        const long stride = (long)gridDim.x * blockDim.x;
        for (long r0 = (long)blockIdx.x * blockDim.x; r0 < n; r0 += stride) {
                const long r = r0 + threadIdx.x;
                Stepping<MODE, MATH> ray;
                double len = 0.;
                int count = 0;
                if ((r < n) && (n_steps > 0)) {
                        double d[3];
                        isotropic((unsigned long long)(first + r), (unsigned long long)first_step, seed, d);
                        ray.resume(geo, w.pos + 3 * r, d, w.alt[r], w.elev[2 * r], w.elev[2 * r + 1], w.index[2 * r],
                            w.index[2 * r + 1]);
                        len = w.length[r];
                }
                const long limit = trip_limit(n_steps);
                for (long trips = 0; (__ballot(ray.live) != 0) && (trips < limit); trips++) {
                        const int event = ray.trip(geo);
                        if (event == NONE) continue;
                        len += ray.length, count++;
                        if ((event == LEFT) || (count >= n_steps)) {
                                const bool in = (ray.index[0] >= 0);
                                w.pos[3 * r] = ray.x[0], w.pos[3 * r + 1] = ray.x[1], w.pos[3 * r + 2] = ray.x[2];
                                w.alt[r] = ray.altitude;
                                w.elev[2 * r] = in ? ray.elevation[0] : 0., w.elev[2 * r + 1] = in ? ray.elevation[1] : 0.;
                                w.index[2 * r] = ray.index[0], w.index[2 * r + 1] = ray.index[1];
                                w.length[r] = len, w.steps[r] += count;
                                ray.stop();
                        } else {
                                double d[3];
                                isotropic((unsigned long long)(first + r), (unsigned long long)(first_step + count), seed, d);
                                ray.redirect(d[0], d[1], d[2]);
                        }
                }
        }
}

/* ---- launchers ------------------------------------------------------------------ */

/* 0, or: 1 the view is not this header's, 2 the launch failed, 3 the kernel failed */
template <class Launch>
static int run(const void * view_bytes, int math, void * stream, Launch && launch)
{
        turtle_amd_view view;
        __builtin_memcpy(&view, view_bytes, sizeof(view));
        const bool known = dispatch(view, [&](auto mode) {
                constexpr int MODE = decltype(mode)::value;
                if (math == STRICT)
                        launch(view, std::integral_constant<int, MODE>(), std::integral_constant<int, STRICT>());
                else
                        launch(view, std::integral_constant<int, MODE>(), std::integral_constant<int, FAST>());
        });
        if (!known) return 1;
        if (hipGetLastError() != hipSuccess) return 2;
        return (hipStreamSynchronize((hipStream_t)stream) == hipSuccess) ? 0 : 3;
}

extern "C" int loops_traverse(const void * view, int math, int simple, int blocks, void * stream, long n,
    double * pos, const double * dir, double ceiling, int max_steps, int * index, double * length, int * n_steps,
    int * n_cross)
{
        const TraverseOut out = { pos, index, length, n_steps, n_cross };
        return run(view, math, stream, [&](const turtle_amd_view & v, auto mode, auto arith) {
                constexpr int MODE = decltype(mode)::value, MATH = decltype(arith)::value;
                if (simple)
                        traverse_step<MODE, MATH><<<blocks, 256, 0, (hipStream_t)stream>>>(v, n, dir, ceiling, max_steps, out);
                else
                        traverse_trip<MODE, MATH><<<blocks, 256, 0, (hipStream_t)stream>>>(v, n, dir, ceiling, max_steps, out);
        });
}

extern "C" int loops_records(const void * view, int math, int blocks, void * stream, long n, const double * pos,
    const double * dir, int k_steps, double * rec, int * taken)
{
        return run(view, math, stream, [&](const turtle_amd_view & v, auto mode, auto arith) {
                records<decltype(mode)::value, decltype(arith)::value><<<blocks, 256, 0, (hipStream_t)stream>>>(
                    v, n, pos, dir, k_steps, rec, taken);
        });
}

extern "C" int loops_walk(const void * view, int math, int blocks, void * stream, long n, unsigned long long seed,
    long first, int first_step, int n_steps, double * pos, double * alt, double * elev, int * index, double * length,
    int * steps)
{
        const WalkState w = { pos, alt, elev, index, length, steps };
        return run(view, math, stream, [&](const turtle_amd_view & v, auto mode, auto arith) {
                walk<decltype(mode)::value, decltype(arith)::value><<<blocks, 256, 0, (hipStream_t)stream>>>(
                    v, n, seed, first, first_step, n_steps, w);
        });
}
