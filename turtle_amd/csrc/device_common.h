/*
 * device_common.h -- the device code that more than one unit of kernels uses (C++ for hipcc only,
 * not installed): the wave idioms, the ray queue, the listing of page faults and the block's
 * tally.  Everything is in the unit's own anonymous namespace, as its kernels are.
 */
#ifndef TAMD_DEVICE_COMMON_H
#define TAMD_DEVICE_COMMON_H

#include <hip/hip_runtime.h>

#include "internal.h" /* includes turtle_amd_device.h: the device functions and the tables */

using namespace turtle_amd_device; /* (in every unit of kernels, and nowhere else: this header is theirs) */

namespace {

/* ---- wave idioms ---------------------------------------------------------
 *
 * What the kernels do a wave at a time. */

/* this lane's rank among the lanes of `mask` (a ballot): how many of them are below it */
__device__ __forceinline__ int lane_rank(ull mask)
{
        return __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0));
}

/* The ray queue of k_walk: a counter in HBM from which a wave draws `chunk` ray numbers at a time
 * with one atomic (wave-aggregated), so the queue sees n / chunk atomics.  (trace_body keeps a
 * refill of its own: the paged wait, the pool and the ordered input are woven in.  So does
 * k_traverse, and its own copy of the step machine: see there.) */
struct RayQueue {
        long next = 0, end = 0; /* wave-uniform: the numbers drawn and not yet given to a lane */
        bool exhausted = false; /* wave-uniform: the queue has run dry */
};

/* Refill the idle lanes (ray < 0 and not `dead`), whole wave: a lane gets its number in `ray` and
 * take() loads that ray -- or sets `ray` below 0 again for one with nothing to do, and the lane
 * draws again.  A lane that still needs a ray when the queue is dry is `dead`. */
template <class Take>
__device__ __forceinline__ void queue_refill(RayQueue & q, ull * __restrict__ queue, int chunk, long n,
    long & ray, bool & dead, Take && take)
{
        for (;;) {
                const bool need = (ray < 0) && !dead;
                const ull mask = __ballot(need);
                if (mask == 0) break;
                if (q.next >= q.end) {
                        if (q.exhausted) {
                                if (need) dead = true;
                                break;
                        }
                        ull base = 0;
                        if ((threadIdx.x & 63) == 0) base = atomicAdd(queue, (ull)chunk);
                        base = __shfl(base, 0, 64);
                        q.next = (long)base;
                        q.end = min((long)base + chunk, n);
                        if ((long)base >= n) {
                                q.exhausted = true;
                                q.next = q.end = 0;
                        }
                        continue;
                }
                const long avail = q.end - q.next;
                const int rank = lane_rank(mask);
                if (need && (rank < avail)) {
                        ray = q.next + rank;
                        take();
                }
                q.next += min((long)__popcll(mask), avail);
        }
}

/* One round of a batch call over a geometry with paged tiles (see tile_fault).
 * ids / n_in: the rays or points of this round (NULL: all of 0 .. n-1, the first
 * round); faulted / n_faulted / wanted: where to list those that need a tile
 * that is not resident, and a bitmap, over the tile table, of the tiles they
 * need.  All NULL for a geometry with every tile resident. */
typedef struct tamd_paging Paging;

/* the whole wave calls: lists the lanes with a fault (one atomic per wave), and
 * counts, tile by tile, how many listed items want it (the host keeps the tiles
 * in demand) -- the tiles of the very first item of the list go into the
 * bitmap `wanted_first` too: the host serves that one without fail, so that
 * every round completes at least one item whatever the others compete for */
__device__ __forceinline__ void page_fault(const Paging & pg, const TileFault & f, long r,
    int also = -1 /* one more tile the item wants kept: where it resumes from */)
{
        const bool fault = f.centre >= 0;
        const ull mask = __ballot(fault);
        if (mask == 0) return;
        const int leader = __builtin_ctzll(mask);
        ull base = 0;
        if ((int)(threadIdx.x & 63) == leader) base = atomicAdd(pg.n_faulted, (ull)__popcll(mask));
        base = __shfl(base, leader, 64);
        if (fault) {
                const int rank = lane_rank(mask);
                pg.faulted[base + rank] = (int)r;
                /* the item the host serves without fail: the one it named, else the
                 * first of this list (which it will name from the next round on) */
                const bool first = (pg.first_id >= 0) ? (r == (long)pg.first_id) : ((base + rank) == 0);
                for (int b = 0; b < 9; b++) {
                        if (!((f.mask >> b) & 1)) continue;
                        const int t = f.centre + (b / 3 - 1) * f.stride + (b % 3 - 1);
                        if (b != 4) atomicAdd(&pg.wanted[(size_t)t * TAMD_DEMAND_STRIDE], 1u); /* (the centre: below) */
                        if (first) atomicOr(&pg.wanted_first[t >> 5], 1u << (t & 31));
                }
                if (also >= 0) {
                        atomicAdd(&pg.wanted[(size_t)also * TAMD_DEMAND_STRIDE], 1u);
                        if (first) atomicOr(&pg.wanted_first[also >> 5], 1u << (also & 31));
                }
        }
        /* the tile an item is IN: one addition per wave and tile (the rays of a batch that start
         * over tiles not resident fault together, a wave at a time, on a handful of tiles) */
        const bool centre = fault && (((f.mask >> 4) & 1) != 0);
        ull left = __ballot(centre);
        while (left != 0) {
                const int lead = __builtin_ctzll(left);
                const int t0 = __shfl(f.centre, lead, 64);
                const ull same = __ballot(centre && (f.centre == t0));
                if ((int)(threadIdx.x & 63) == lead)
                        atomicAdd(&pg.wanted[(size_t)t0 * TAMD_DEMAND_STRIDE], (unsigned)__popcll(same));
                left &= ~same;
        }
}

/* Loop of the one-thread-per-item kernels: whole waves go round (page_fault is
 * a wave-wide call); `r` is the item of this lane, or -1 */
#define PAGED_ITEMS(pg, n, i0, r)                                                              \
        const long n_items_ = ((pg).n_in != nullptr) ? (long)*(pg).n_in : (n);                 \
        for (long i0 = blockIdx.x * (long)blockDim.x; i0 < n_items_;                           \
             i0 += (long)gridDim.x * blockDim.x)                                               \
                for (long i_ = i0 + threadIdx.x, r = (i_ < n_items_) ?                         \
                             (((pg).ids != nullptr) ? (long)(pg).ids[i_] : i_) : -1, once_ = 1; \
                     once_; once_ = 0)

__device__ __forceinline__ ull wave_sum(ull v)
{
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        return v;
}

/* Add a block's four counters to the global ones: waves -> LDS -> 4 atomics per
 * block.  (One set of atomics per WAVE is what a kernel can least afford: the
 * counters share a cache line, same-line atomics complete at ~5 ns apiece, and
 * the step kernel's 8 192 waves spent 4x their run time queueing there.) */
__device__ __forceinline__ void block_tally(ull * __restrict__ stats, ull a, ull b, ull c, ull d)
{
        __shared__ ull part[4][4]; /* [wave][counter]: blocks are 256 threads */
        a = wave_sum(a), b = wave_sum(b), c = wave_sum(c), d = wave_sum(d);
        const int wave = (int)(threadIdx.x >> 6);
        if ((threadIdx.x & 63) == 0) part[wave][0] = a, part[wave][1] = b, part[wave][2] = c, part[wave][3] = d;
        __syncthreads();
        if (threadIdx.x < 4) {
                const ull sum = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] +
                    part[3][threadIdx.x];
                if (sum != 0) atomicAdd(&stats[threadIdx.x], sum);
        }
}

constexpr int kChunk = 64; /* rays a wave draws from the global queue at once */

} /* namespace */

#endif
