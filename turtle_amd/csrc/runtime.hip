/*
 * runtime.hip -- the calling thread's share of the device: which gfx950 it works on, its stream,
 * HBM and pinned memory, the scratch arena and the grow-only blocks (internal.h: tamd_dev_*,
 * tamd_scratch_*).  No kernel is named here: they, and what launches them, are in the
 * units of kernels (device.hip and the files beside it).
 */
#include <sys/syscall.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "device_ctx.h"
#include "internal.h"

thread_local char g_error[512] = "";
thread_local Ctx g_ctx;

int fail(const char * what, hipError_t e, const char * prefix)
{
        snprintf(g_error, sizeof(g_error), "%s%s: %s (HIP error %d)", prefix, what,
            hipGetErrorString(e), (int)e);
        return 1;
}

extern "C" const char * tamd_dev_error(void) { return g_error; }

extern "C" int tamd_dev_count(void)
{
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess) return 0;
        return count;
}

/* A thread that ends without turtle_amd_thread_release() (a pool's worker, an OpenMP
 * thread) gives back its stream, arena, blocks and pinned buffer here -- while the
 * process lives: at process exit the HIP runtime may already be gone, and the
 * main thread's context is left to it. */
static thread_local struct CtxGuard {
        bool armed = false; /* (set by tamd_dev_select on any thread but the main one) */
        ~CtxGuard()
        {
                if (armed) g_ctx.release();
        }
} g_ctx_guard;

extern "C" int tamd_dev_select(int device)
{
        const int count = tamd_dev_count();
        if (count <= 0) {
                snprintf(g_error, sizeof(g_error),
                    "no HIP device is visible: libturtle_amd has no CPU path");
                return 1;
        }
        if ((device < 0) || (device >= count)) {
                snprintf(g_error, sizeof(g_error),
                    "invalid device index %d (have %d)", device, count);
                return 1;
        }
        if (g_ctx.device == device) {
                HIP_TRY(hipSetDevice(device));
                return 0;
        }
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, device));
        if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
                snprintf(g_error, sizeof(g_error),
                    "device %d is %s: libturtle_amd carries gfx950 code only",
                    device, prop.gcnArchName);
                return 1;
        }
        /* what this thread held on its previous device goes (its stream too: a
         * stream handed in by turtle_amd_stream_set belonged to that device) */
        g_ctx.release();
        HIP_TRY(hipSetDevice(device));
        g_ctx.device = device;
        g_ctx_guard.armed = ((long)syscall(SYS_gettid) != (long)getpid()); /* not the main thread: see CtxGuard */
        g_ctx.cus = prop.multiProcessorCount;
        HIP_TRY(hipStreamCreateWithFlags(&g_ctx.own_stream, hipStreamNonBlocking));
        g_ctx.stream = g_ctx.own_stream;
        return 0;
}

extern "C" int tamd_dev_init(void)
{
        if (g_ctx.device >= 0) {
                HIP_TRY(hipSetDevice(g_ctx.device)); /* HIP's current device is per thread too */
                return 0;
        }
        int device = 0;
        const char * env = getenv("LOCAL_RANK");
        if ((env != nullptr) && (*env != 0)) {
                const int count = tamd_dev_count();
                if (count > 0) device = atoi(env) % count;
        }
        return tamd_dev_select(device);
}

extern "C" int tamd_dev_current(void) { return g_ctx.device; }

/* what the calling thread holds on its device (a worker calls it before it ends:
 * nothing is freed behind a thread's back, the runtime may be gone by then) */
extern "C" void tamd_dev_release(void)
{
        g_ctx.release();
        g_ctx.device = -1;
}
extern "C" int tamd_dev_cus(void) { return (tamd_dev_init() == 0) ? g_ctx.cus : 0; }

extern "C" int tamd_dev_stream_set(void * stream)
{
        if (tamd_dev_init()) return 1;
        g_ctx.stream = (stream != nullptr) ? (hipStream_t)stream : g_ctx.own_stream;
        return 0;
}

extern "C" int tamd_dev_sync(void)
{
        if (tamd_dev_init()) return 1;
        HIP_TRY(hipStreamSynchronize(g_ctx.stream));
        return 0;
}

/* every stream of `device` (before memory that other threads' launches may still
 * read is freed); leaves the calling thread on its own device */
/* Every stream of that device has drained (non-zero: it could not be told -- the
 * caller then LEAKS what it meant to free there, rather than free memory that a
 * launch may still read).  The calling thread is back on its own device on every
 * path. */
extern "C" int tamd_dev_sync_device(int device)
{
        if (device < 0) return 0;
        hipError_t e = hipSetDevice(device);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if ((g_ctx.device >= 0) && (g_ctx.device != device)) {
                const hipError_t back = hipSetDevice(g_ctx.device);
                if (e == hipSuccess) e = back;
        }
        return (e == hipSuccess) ? 0 : fail("tamd_dev_sync_device", e);
}

extern "C" int tamd_dev_malloc(void ** ptr, size_t bytes)
{
        *ptr = nullptr;
        if (tamd_dev_init()) return 1;
        HIP_TRY(hipMalloc(ptr, bytes ? bytes : 1));
        return 0;
}

extern "C" void tamd_dev_free(void * ptr)
{
        if (ptr != nullptr) (void)hipFree(ptr);
}

/* memory of another device than the calling thread's */
extern "C" void tamd_dev_free_on(int device, void * ptr)
{
        if (ptr == nullptr) return;
        if ((device >= 0) && (device != g_ctx.device)) (void)hipSetDevice(device);
        (void)hipFree(ptr);
        if ((device >= 0) && (device != g_ctx.device) && (g_ctx.device >= 0)) (void)hipSetDevice(g_ctx.device);
}

extern "C" int tamd_dev_h2d(void * dst, const void * src, size_t bytes)
{
        if (tamd_dev_init()) return 1;
        if (bytes == 0) return 0;
        HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, g_ctx.stream));
        HIP_TRY(hipStreamSynchronize(g_ctx.stream));
        return 0;
}

extern "C" int tamd_dev_d2h(void * dst, const void * src, size_t bytes)
{
        if (tamd_dev_init()) return 1;
        if (bytes == 0) return 0;
        HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, g_ctx.stream));
        HIP_TRY(hipStreamSynchronize(g_ctx.stream));
        return 0;
}

extern "C" int tamd_dev_zero(void * dst, size_t bytes)
{
        if (tamd_dev_init()) return 1;
        HIP_TRY(hipMemsetAsync(dst, 0, bytes, g_ctx.stream));
        return 0;
}

extern "C" int tamd_dev_pinned(void ** ptr, size_t bytes)
{
        *ptr = nullptr;
        if (tamd_dev_init()) return 1;
        if (bytes > g_ctx.pinned_size) {
                HIP_TRY(hipStreamSynchronize(g_ctx.stream));
                if (g_ctx.pinned != nullptr) (void)hipHostFree(g_ctx.pinned);
                g_ctx.pinned = nullptr, g_ctx.pinned_size = 0;
                HIP_TRY(hipHostMalloc(&g_ctx.pinned, bytes, hipHostMallocDefault));
                g_ctx.pinned_size = bytes;
        }
        *ptr = g_ctx.pinned;
        return 0;
}

/* page-locked host memory that outlives the call (a stack's staging buffers for its
 * tiles: a copy from it is queued, not waited for) */
extern "C" int tamd_dev_host_alloc(void ** ptr, size_t bytes)
{
        *ptr = nullptr;
        if (tamd_dev_init()) return 1;
        HIP_TRY(hipHostMalloc(ptr, bytes, hipHostMallocDefault));
        return 0;
}

extern "C" void tamd_dev_host_free(void * ptr)
{
        if (ptr != nullptr) (void)hipHostFree(ptr);
}

extern "C" int tamd_dev_copy_async(void * dst, const void * src, size_t bytes, int to_device)
{
        if (tamd_dev_init()) return 1;
        if (bytes == 0) return 0;
        HIP_TRY(hipMemcpyAsync(dst, src, bytes, to_device ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost,
            g_ctx.stream));
        return 0;
}

extern "C" void tamd_scratch_reset(void) { g_ctx.scratch_used = 0; }

extern "C" int tamd_scratch_get(void ** ptr, size_t bytes)
{
        *ptr = nullptr;
        if (tamd_dev_init()) return 1;
        const size_t need = (bytes + 255) & ~(size_t)255;
        if (g_ctx.scratch_used + need > g_ctx.scratch_size) {
                if (g_ctx.scratch_used != 0) {
                        /* pieces already handed out would dangle: the host layer
                         * sizes the arena up front with one oversize request */
                        snprintf(g_error, sizeof(g_error), "scratch arena exhausted");
                        return 1;
                }
                HIP_TRY(hipStreamSynchronize(g_ctx.stream));
                if (g_ctx.scratch) (void)hipFree(g_ctx.scratch);
                g_ctx.scratch = nullptr, g_ctx.scratch_size = 0;
                const size_t size = need + (need >> 2) + (1u << 20);
                HIP_TRY(hipMalloc(&g_ctx.scratch, size));
                g_ctx.scratch_size = size;
        }
        *ptr = (char *)g_ctx.scratch + g_ctx.scratch_used;
        g_ctx.scratch_used += need;
        return 0;
}

/* One of the calling thread's grow-only blocks (0: the pager's lists and counters,
 * 1: the tables of a stack's own batch calls), at least `bytes` long; *grown is
 * set when it is a new allocation (what it held is gone) */
extern "C" int tamd_dev_block(int which, void ** ptr, size_t bytes, int * grown)
{
        *ptr = nullptr;
        if (grown != nullptr) *grown = 0;
        if (tamd_dev_init()) return 1;
        if (bytes > g_ctx.block_size[which]) {
                if (g_ctx.block[which] != nullptr) {
                        HIP_TRY(hipStreamSynchronize(g_ctx.stream));
                        (void)hipFree(g_ctx.block[which]);
                        g_ctx.block[which] = nullptr, g_ctx.block_size[which] = 0;
                }
                HIP_TRY(hipMalloc(&g_ctx.block[which], bytes));
                g_ctx.block_size[which] = bytes;
                if (grown != nullptr) *grown = 1;
        }
        *ptr = g_ctx.block[which];
        return 0;
}

extern "C" void tamd_dev_math_set(int strict) { g_ctx.math_strict = strict ? 1 : 0; }
extern "C" void tamd_dev_in_flight_set(int batches) { g_ctx.in_flight = (batches > 1) ? batches : 1; }
extern "C" int tamd_dev_in_flight_get(void) { return g_ctx.in_flight; }
extern "C" int tamd_dev_math_get(void) { return g_ctx.math_strict; }
