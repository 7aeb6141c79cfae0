/*
 * normal_loop.hip -- turtle_amd_device::normal() called from a kernel of the caller's own, as a
 * user of include/turtle_amd_device.h would (tests/test_gpu_normal.py).  All pointers are DEVICE
 * pointers; `view` is what turtle_amd_stepper_view_acquire filled.
 *
 * Build: hipcc --offload-arch=gfx950 -ffp-contract=off -I include -shared -fPIC
 */
#include "turtle_amd_device.h"

using namespace turtle_amd_device;

/* one point per thread: data_index[r], and normal[r] where there is data (else untouched) */
template <int MODE, int MATH>
__global__ void __launch_bounds__(256) normals(turtle_amd_view view, long n, const double * __restrict__ pos,
    const int * __restrict__ layer, double * __restrict__ out, int * __restrict__ data_index)
{
        const Geometry<MODE, MATH> geo(view);
        const long stride = (long)gridDim.x * blockDim.x;
        for (long r = (long)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += stride) {
                const double p[3] = { pos[3 * r], pos[3 * r + 1], pos[3 * r + 2] };
                double w[3];
                const int found = normal(geo, p, layer[r], w);
                data_index[r] = found;
                if (found >= 0) out[3 * r] = w[0], out[3 * r + 1] = w[1], out[3 * r + 2] = w[2];
        }
}

/* 0, or: 1 the view is not this header's, 2 the launch failed, 3 the kernel failed */
extern "C" int normal_loop(const void * view_bytes, int math, int blocks, void * stream, long n, const double * pos,
    const int * layer, double * out, int * data_index)
{
        turtle_amd_view view;
        __builtin_memcpy(&view, view_bytes, sizeof(view));
        const bool known = dispatch(view, [&](auto mode) {
                constexpr int MODE = decltype(mode)::value;
                if (math == STRICT)
                        normals<MODE, STRICT><<<blocks, 256, 0, (hipStream_t)stream>>>(view, n, pos, layer, out, data_index);
                else
                        normals<MODE, FAST><<<blocks, 256, 0, (hipStream_t)stream>>>(view, n, pos, layer, out, data_index);
        });
        if (!known) return 1;
        if (hipGetLastError() != hipSuccess) return 2;
        return (hipStreamSynchronize((hipStream_t)stream) == hipSuccess) ? 0 : 3;
}
