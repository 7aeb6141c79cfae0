/*
 * maps.hip -- whole maps and windows of their nodes, and the launchers.  The arithmetic contract
 * and the citations [ref FILE:LINE] are device.hip's (see its header).
 *
 *   k_resample      a whole map from a stack or a map (turtle_map_resample)
 *   k_fill_encode, k_fill_store, k_nodes   windows of nodes (turtle_map_fill_n, _node_n)
 *   k_unblock       the host copy of a map from its HBM copy
 */
#include <hip/hip_runtime.h>

#include "device_common.h"
#include "device_launch.h"

namespace {

/* ---- turtle_map_resample ------------------------------------------------------
 * Every node of a target map filled from a stack or another map: the loop of the
 * reference's examples/example-projection.c (turtle_map_node, _unproject,
 * turtle_stack_elevation, turtle_map_fill) in one launch.  One WAVE per 8 x 8 block of
 * the target, its 64 lanes the block's 64 nodes in the HBM order (internal.h): the
 * wave's store of the new codes is one 128-byte line, and neighbouring lanes look up
 * neighbouring source cells.  The kernel writes a whole new copy of the target in that
 * layout; a node that stays as it is (outside the data, or outside the map's span
 * without TURTLE_AMD_RESAMPLE_CLAMP) gets the code of the map's current copy, so that a
 * block's work can be done again and the copy is complete whatever the host decides.
 * Lookups are the strict bilinear ones of k_elevation: the result does not depend on
 * the arithmetic mode. */
enum { RS_STACK = 0, RS_MAP = 1 };

/* page_fault for an item that is a whole wave (a target block): the block is listed
 * once if any of its nodes met a tile that is not resident, and is redone whole in a
 * later round; each tile it wants counts once per block (the usual case: one tile), a
 * seam's neighbours once per node that wants them */
__device__ __forceinline__ void page_fault_block(const Paging & pg, const TileFault & f, int item)
{
        const bool fault = f.centre >= 0;
        const ull mask = __ballot(fault);
        if (mask == 0) return;
        const int lane = (int)(threadIdx.x & 63);
        const int leader = __builtin_ctzll(mask);
        ull base = 0;
        if (lane == leader) {
                base = atomicAdd(pg.n_faulted, 1ull);
                pg.faulted[base] = item;
        }
        base = __shfl(base, leader, 64);
        const bool first = (pg.first_id >= 0) ? (item == pg.first_id) : (base == 0);
        if (fault) {
                for (int b = 0; b < 9; b++) {
                        if (!((f.mask >> b) & 1)) continue;
                        const int t = f.centre + (b / 3 - 1) * f.stride + (b % 3 - 1);
                        if (b != 4) atomicAdd(&pg.wanted[(size_t)t * TAMD_DEMAND_STRIDE], 1u);
                        if (first) atomicOr(&pg.wanted_first[t >> 5], 1u << (t & 31));
                }
        }
        const bool centre = fault && (((f.mask >> 4) & 1) != 0);
        ull left = __ballot(centre);
        while (left != 0) {
                const int lead = __builtin_ctzll(left);
                const int t0 = __shfl(f.centre, lead, 64);
                const ull same = __ballot(centre && (f.centre == t0));
                if (lane == lead) atomicAdd(&pg.wanted[(size_t)t0 * TAMD_DEMAND_STRIDE], 1u);
                left &= ~same;
        }
}

/* grids[0]: the target (nodes: its current HBM copy; x0 .. dy, nbx and proj as the
 * map holds them); grids[1]: the source map (RS_MAP).  z0, dz, is_signed: the
 * target's own encoding, as turtle_map_fill applies it.  counters (zeroed by the
 * caller, added to round after round): nodes outside the data, nodes outside the span
 * and not clamped, nodes clamped.  Items are the target's blocks; over a paged stack,
 * a block with a faulting node is listed and none of its work is kept. */
template <int SRC, int TPROJ /* the target's projection type */>
__global__ void __launch_bounds__(256) k_resample(tamd_view v, const tamd_grid * __restrict__ grids,
    double z0, double dz, int is_signed, int flags, long n_blocks, uint16_t * __restrict__ out, Paging pg,
    ull * __restrict__ counters)
{
        const tamd_grid & t = grids[0];
        const int lane = (int)(threadIdx.x & 63);
        const long waves = (long)gridDim.x * (blockDim.x >> 6);
        const long n_items = (pg.n_in != nullptr) ? (long)*pg.n_in : n_blocks;
        const double top = z0 + 65535 * dz; /* [ref map.c:196-197] */
        ull n_outside = 0, n_bad = 0, n_clamped = 0;
        for (long i = blockIdx.x * (long)(blockDim.x >> 6) + (threadIdx.x >> 6); i < n_items; i += waves) {
                const long blk = (pg.ids != nullptr) ? (long)pg.ids[i] : i;
                const int ix = (int)(blk % t.nbx) * TAMD_BLOCK + (lane & 7);
                const int iy = (int)(blk / t.nbx) * TAMD_BLOCK + (lane >> 3);
                TileFault f = { -1, 0, 0 };
                bool keep = true;
                int outside = 0, bad = 0, clamped = 0;
                uint16_t code = 0;
                if ((ix < t.nx) && (iy < t.ny)) {
                        /* turtle_map_node [ref map.c:217-218] */
                        const double x = t.x0 + ix * t.dx;
                        const double y = t.y0 + iy * t.dy;
                        double latitude, longitude;
                        if (TPROJ >= 0)
                                d_unproject_body<TPROJ>(t.proj, x, y, latitude, longitude);
                        else
                                latitude = y, longitude = x;
                        double z = 0.;
                        int in;
                        if (SRC == RS_STACK) {
                                in = d_stack_elevation<false>(v, v.stacks[0], latitude, longitude, z, f);
                                if (in >= 0) f.centre = -1;
                        } else {
                                const tamd_grid & s = grids[1];
                                double u, w;
                                if (flags & TAMD_RESAMPLE_IDENTITY)
                                        u = x, w = y;
                                else if (s.proj.type >= 0)
                                        d_project_body(s.proj, latitude, longitude, u, w);
                                else
                                        u = longitude, w = latitude;
                                in = d_grid_elevation<false>(s, u, w, z) ? 1 : 0;
                        }
                        if (in == 0) {
                                outside = 1;
                        } else if (in > 0) {
                                /* turtle_map_fill [ref map.c:192-200, :47-51] */
                                const bool off = ((dz <= 0.) && (z != z0)) || (z < z0) || (z > top);
                                if (off && !(flags & TURTLE_AMD_RESAMPLE_CLAMP)) {
                                        bad = 1;
                                } else {
                                        if (off) {
                                                clamped = 1;
                                                z = ((dz <= 0.) || (z < z0)) ? z0 : top;
                                        }
                                        if (is_signed)
                                                code = (uint16_t)(int)z; /* (int16)z */
                                        else
                                                code = (dz > 0.) ? (uint16_t)(unsigned)round((z - z0) / dz) : 0;
                                        keep = false;
                                }
                        }
                }
                if (pg.faulted != nullptr) {
                        const bool redo = __ballot(f.centre >= 0) != 0;
                        page_fault_block(pg, f, (int)blk);
                        if (redo) continue; /* (the whole wave) */
                }
                const size_t k = (size_t)blk * 64 + lane;
                if (keep) code = GLOBAL_NODES(t.nodes)[k];
                out[k] = code;
                n_outside += outside, n_bad += bad, n_clamped += clamped;
        }
        block_tally(counters, n_outside, n_bad, n_clamped, 0);
}

/* The host copy of a map from its HBM copy: rows of nx nodes, south to north */
__global__ void k_unblock(const uint16_t * __restrict__ blocked, int nx, int ny, int nbx,
    uint16_t * __restrict__ rows)
{
        const long n = (long)nx * ny;
        for (long k = blockIdx.x * (long)blockDim.x + threadIdx.x; k < n; k += (long)gridDim.x * blockDim.x) {
                const int iy = (int)(k / nx), ix = (int)(k - (long)iy * nx);
                rows[k] = GLOBAL_NODES(blocked)[d_node_index(nbx, ix, iy)];
        }
}

/* turtle_map_fill_n, first half: the window's elevations (row j at z + j * ld) to the codes
 * turtle_map_fill stores, k_resample's expressions in its operand order, into a compact
 * buffer of ny rows of nx codes.  Nothing of the map is written: the host commits
 * (k_fill_store) only after it has read counters[0] == 0.  counters (zeroed by the caller):
 * elements that fail the call, elements clamped, and the failed ones that turtle_map_fill calls
 * "inconsistent" (dz <= 0 and z != z0; a NaN is not among them). */
__global__ void __launch_bounds__(256) k_fill_encode(const double * __restrict__ z_in, long ld, int nx, long n,
    double z0, double dz, int is_signed, int flags, uint16_t * __restrict__ codes, ull * __restrict__ counters)
{
        const double top = z0 + 65535 * dz; /* [ref map.c:196-197] */
        ull n_bad = 0, n_clamped = 0, n_inconsistent = 0;
        for (long k = blockIdx.x * (long)blockDim.x + threadIdx.x; k < n; k += (long)gridDim.x * blockDim.x) {
                const long j = k / nx;
                double z = z_in[j * ld + (k - j * nx)];
                /* turtle_map_fill [ref map.c:192-200, :47-51]; a NaN passes none of its comparisons */
                const bool nan = (z != z);
                const bool off = nan || ((dz <= 0.) && (z != z0)) || (z < z0) || (z > top);
                uint16_t code = 0;
                if (off && (nan || !(flags & TURTLE_AMD_FILL_CLAMP))) {
                        n_bad++, n_inconsistent += (!nan && (dz <= 0.) && (z != z0)) ? 1 : 0;
                } else {
                        if (off) {
                                n_clamped++;
                                z = ((dz <= 0.) || (z < z0)) ? z0 : top;
                        }
                        if (is_signed)
                                code = (uint16_t)(int)z; /* (int16)z */
                        else
                                code = (dz > 0.) ? (uint16_t)(unsigned)round((z - z0) / dz) : 0;
                }
                codes[k] = code;
        }
        block_tally(counters, n_bad, n_clamped, n_inconsistent, 0);
}

/* ... second half: the codes into the map's HBM copy, in place.  One wave a touched 8 x 8
 * block (nwx of them a row of the window), its lanes in HBM order: a lane outside the window
 * keeps the code that is there (blank: the copy held nothing yet and the window is the whole
 * map -- the padding of its last blocks is zeroed), and the block goes out as its 128-byte line. */
__global__ void __launch_bounds__(256) k_fill_store(uint16_t * __restrict__ nodes, int nbx, int ix0, int iy0,
    int nx, int ny, int nwx, long n_blocks, int blank, const uint16_t * __restrict__ codes)
{
        const int lane = (int)(threadIdx.x & 63);
        const long waves = (long)gridDim.x * (blockDim.x >> 6);
        for (long i = blockIdx.x * (long)(blockDim.x >> 6) + (threadIdx.x >> 6); i < n_blocks; i += waves) {
                const int bx = (ix0 >> 3) + (int)(i % nwx), by = (iy0 >> 3) + (int)(i / nwx);
                const int ix = bx * TAMD_BLOCK + (lane & 7) - ix0, iy = by * TAMD_BLOCK + (lane >> 3) - iy0;
                const size_t k = ((size_t)by * nbx + bx) * 64 + lane;
                uint16_t code = 0;
                if ((ix >= 0) && (ix < nx) && (iy >= 0) && (iy < ny))
                        code = codes[(long)iy * nx + ix];
                else if (!blank)
                        code = GLOBAL_NODES(nodes)[k];
                nodes[k] = code;
        }
}

/* turtle_map_node_n: the window's nodes decoded as turtle_map_node decodes them [ref
 * map.c:41-44], row j to out + j * ld; consecutive lanes store consecutive doubles */
__global__ void __launch_bounds__(256) k_nodes(const uint16_t * __restrict__ nodes, int nbx, int ix0, int iy0,
    int nx, long n, double z0, double dz, int is_signed, double * __restrict__ out, long ld)
{
        for (long k = blockIdx.x * (long)blockDim.x + threadIdx.x; k < n; k += (long)gridDim.x * blockDim.x) {
                const long j = k / nx;
                const int i = (int)(k - j * nx);
                const uint16_t code = GLOBAL_NODES(nodes)[d_node_index(nbx, ix0 + i, iy0 + (int)j)];
                out[j * ld + i] = is_signed ? (double)(int16_t)code : z0 + code * dz;
        }
}
} /* namespace */

extern "C" int tamd_k_resample(struct tamd_view view, const struct tamd_grid * grids, int from_map,
    double z0, double dz, int is_signed, int flags, long n_blocks, uint16_t * out,
    struct tamd_paging pg, unsigned long long * counters)
{
        if (tamd_dev_init()) return 1;
        if (n_blocks <= 0) return 0;
        /* the target's projection: a host field, read back from its table */
        struct tamd_grid target;
        if (tamd_dev_d2h(&target, grids, sizeof(target))) return 1;
        const unsigned blocks = grid_for(n_blocks * 64, 256);
        return with_constant<RS_MAP, RS_STACK>(from_map ? RS_MAP : RS_STACK, [&](auto source) {
                return with_constant<TAMD_PROJ_LAMBERT, TAMD_PROJ_UTM, TAMD_PROJ_NONE>(target.proj.type, [&](auto type) {
                        return launch_blocks("k_resample", k_resample<decltype(source)::value, decltype(type)::value>,
                            blocks, 0, view, grids, z0, dz, is_signed, flags, n_blocks, out, pg, counters);
                });
        });
}

extern "C" int tamd_k_unblock(const uint16_t * blocked, int nx, int ny, int nbx, uint16_t * rows)
{
        return launch_items("k_unblock", k_unblock, (long)nx * ny, 0, blocked, nx, ny, nbx, rows);
}

extern "C" int tamd_k_fill_encode(const double * elevation, long ld, int nx, int ny, double z0, double dz,
    int is_signed, int flags, uint16_t * codes, unsigned long long * counters)
{
        const long n = (long)nx * ny;
        return launch_items("k_fill_encode", k_fill_encode, n, 0, elevation, ld, nx, n, z0, dz, is_signed, flags,
            codes, counters);
}

extern "C" int tamd_k_fill_store(uint16_t * nodes, int nbx, int ix0, int iy0, int nx, int ny, int blank,
    const uint16_t * codes)
{
        const int nwx = ((ix0 + nx - 1) >> 3) - (ix0 >> 3) + 1, nwy = ((iy0 + ny - 1) >> 3) - (iy0 >> 3) + 1;
        const long n_blocks = (long)nwx * nwy;
        return launch_items("k_fill_store", k_fill_store, n_blocks * 64, 0, nodes, nbx, ix0, iy0, nx, ny, nwx,
            n_blocks, blank, codes);
}

extern "C" int tamd_k_nodes(const uint16_t * nodes, int nbx, int ix0, int iy0, int nx, int ny, double z0,
    double dz, int is_signed, double * elevation, long ld)
{
        const long n = (long)nx * ny;
        return launch_items("k_nodes", k_nodes, n, 0, nodes, nbx, ix0, iy0, nx, n, z0, dz, is_signed, elevation, ld);
}
