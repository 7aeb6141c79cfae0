/*
 * grid_walk.hip -- turtle_amd_device::grid_depth() called from a kernel of the caller's own, as a
 * user of include/turtle_amd_device.h would (tests/test_gpu_advance_grid.py): one segment a thread.
 * All pointers are DEVICE pointers; `grid_bytes` is a struct turtle_amd_grid_view on the host whose
 * density is a device pointer.
 *
 * Build: hipcc --offload-arch=gfx950 -ffp-contract=off -I include -shared -fPIC
 */
#include "turtle_amd_device.h"

using namespace turtle_amd_device;

__global__ void __launch_bounds__(256) walks(turtle_amd_grid_view grid, long n, const double * __restrict__ rho_out,
    const int * __restrict__ medium, const double * __restrict__ p0, const double * __restrict__ dir,
    const double * __restrict__ L, const double * __restrict__ R, double * __restrict__ x, double * __restrict__ f,
    int * __restrict__ stopped)
{
        const long stride = (long)gridDim.x * blockDim.x;
        for (long r = (long)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += stride) {
                const GridDepth w = grid_depth(grid, rho_out[r], medium[r], p0[3 * r], p0[3 * r + 1], p0[3 * r + 2],
                    dir[3 * r], dir[3 * r + 1], dir[3 * r + 2], L[r], R[r]);
                x[r] = w.x, f[r] = w.f, stopped[r] = w.stopped ? 1 : 0;
        }
}

/* 0, or: 2 the launch failed, 3 the kernel failed */
extern "C" int grid_walk(const void * grid_bytes, long n, const double * rho_out, const int * medium,
    const double * p0, const double * dir, const double * L, const double * R, double * x, double * f, int * stopped)
{
        turtle_amd_grid_view grid;
        __builtin_memcpy(&grid, grid_bytes, sizeof(grid));
        const int blocks = (int)((n + 255) / 256);
        walks<<<blocks > 0 ? blocks : 1, 256, 0, 0>>>(grid, n, rho_out, medium, p0, dir, L, R, x, f, stopped);
        if (hipGetLastError() != hipSuccess) return 2;
        return (hipStreamSynchronize(0) == hipSuccess) ? 0 : 3;
}

extern "C" long grid_walk_view_size(void) { return (long)sizeof(turtle_amd_grid_view); }
