/*
 * device_launch.h -- what the launchers of every unit of kernels are written with (C++ for hipcc
 * only, not installed): the calling thread's stream and its settings by name, the grid of a flat
 * and of a persistent launch, and a run-time value turned into a kernel's template parameter.
 */
#ifndef TAMD_DEVICE_LAUNCH_H
#define TAMD_DEVICE_LAUNCH_H

#include <hip/hip_runtime.h>

#include <type_traits>

#include "device_common.h" /* (ull, and turtle_amd_device's names as the kernels see them) */
#include "device_ctx.h"
#include "internal.h"

#define g_stream (g_ctx.stream)
#define g_cus (g_ctx.cus)
#define g_math_strict (g_ctx.math_strict)

/* Which arithmetic a stepping call runs in.  FAST takes its samples from closed forms and lines that
 * are a few 1e-9 m off the exact transform (kLineTau0): a stepper whose minimum step is below the
 * 1e-8 m of the bisection's bracket asks for steps finer than that noise -- a ray that creeps along
 * the ground then crosses it tens of steps earlier or later than the reference's, or not before
 * max_steps -- and is served by the STRICT kernels whatever the mode (a NaN resolution too). */
static bool strict_math(const tamd_view & view)
{
        return g_math_strict || !view.fast_ok || !(view.resolution >= 1E-08);
}

static int grid_for(long n, int block)
{
        long blocks = (n + block - 1) / block;
        /* (4, 16 or 64 blocks per CU: the same or worse, measured on the step kernel) */
        const long cap = (long)(g_cus > 0 ? g_cus : 256) * 8;
        if (blocks > cap) blocks = cap;
        if (blocks < 1) blocks = 1;
        return (int)blocks;
}

/* `blocks` blocks of 256 threads of a kernel, on the calling thread's stream */
template <class... P, class... A>
static int launch_blocks(const char * name, void (*kernel)(P...), unsigned blocks, size_t lds_bytes,
    const A &... args)
{
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), lds_bytes, g_stream, args...);
        LAUNCH_CHECK(name);
        return 0;
}
/* A whole flat entry point: n items, each the work of one thread (none: nothing to do) */
template <class... P, class... A>
static int launch_items(const char * name, void (*kernel)(P...), long n, size_t lds_bytes, const A &... args)
{
        if (tamd_dev_init()) return 1;
        if (n <= 0) return 0;
        return launch_blocks(name, kernel, grid_for(n, 256), lds_bytes, args...);
}

/* What a launcher zeroes before its kernels: the first n_stats words of `stats` (0: none, they add
 * up over the rounds of a call) and the first n_queue of `queue`.  A fill is a launch of its own,
 * 5 us between two dependent kernels: the two are ONE where they are neighbours, as in a stepper's
 * d_stats (internal.h: TAMD_STATS_QUEUE). */
static int zero_words(ull * stats, int n_stats, ull * queue, int n_queue)
{
        if ((n_stats > 0) && (queue == stats + TAMD_STATS_QUEUE) && (n_stats <= TAMD_STATS_QUEUE)) {
                HIP_TRY(hipMemsetAsync(stats, 0, (size_t)(TAMD_STATS_QUEUE + n_queue) * sizeof(ull), g_stream));
                return 0;
        }
        if (n_stats > 0) HIP_TRY(hipMemsetAsync(stats, 0, (size_t)n_stats * sizeof(ull), g_stream));
        HIP_TRY(hipMemsetAsync(queue, 0, (size_t)n_queue * sizeof(ull), g_stream));
        return 0;
}

/* A run-time value that a kernel takes as a template parameter: f is called with the
 * std::integral_constant of the first of VALUES that equals `value`, or of the last. */
template <int FIRST, int... REST, class F>
static int with_constant(int value, F && f)
{
        if constexpr (sizeof...(REST) > 0)
                if (value != FIRST) return with_constant<REST...>(value, f);
        return f(std::integral_constant<int, FIRST>());
}
/* ... the geometry's MODE (one map, one stack, else the generic instance) */
template <class F>
static int with_mode(int mode, F && f)
{
        return with_constant<TAMD_MODE_ONE_MAP, TAMD_MODE_ONE_STACK, TAMD_MODE_GENERIC>(mode, f);
}

/* ... the arithmetic (Strict, else Fast: a kernel's FAST) */
typedef std::integral_constant<int, 0> Strict;
typedef std::integral_constant<int, 1> Fast;
template <class F>
static int with_math(bool strict, F && f)
{
        return with_constant<Strict::value, Fast::value>(strict ? Strict::value : Fast::value, f);
}

/* Waves per SIMD the trace kernel is launched with.  It is fp64-VALU bound
 * with a dependent 4-node gather per sample, so a few waves per SIMD are
 * enough to cover the gather latency: as many as fit. */
static int trace_blocks_per_cu(const void * kernel)
{
        int blocks = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, kernel, 256, 0) !=
                hipSuccess ||
            blocks < 1)
                blocks = 1;
        /* batches in flight share the SIMDs: a kernel that takes one block a CU fewer than fit
         * leaves registers for a wave of another batch's kernel beside its own (three C2 batches
         * in flight: 2.38 -> 2.29 ms a pass over 10 passes, 2.39 -> 2.18 over 20; C4 25.5 -> 24.7;
         * through a stack no change -- two blocks a CU whatever fits: C2 the same, C4 24.1, but C3
         * 23.9 -> 25.3; alone a kernel would lose either way: C2 3.55 -> 3.7 with two) */
        if ((g_ctx.in_flight > 1) && (blocks > 2)) blocks -= 1;
        return blocks;
}

/* The grid of a persistent kernel over n rays: the blocks that fit the chip, or that the
 * rays can fill */
template <class... P>
static unsigned persistent_blocks(void (*kernel)(P...), long n)
{
        long blocks = (long)g_cus * trace_blocks_per_cu((const void *)kernel);
        const long useful = (n + 255) / 256;
        if (blocks > useful) blocks = useful;
        return (unsigned)blocks;
}

#endif
