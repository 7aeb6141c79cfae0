/*
 * device_ctx.h -- what runtime.hip and the units of kernels share (C++ only, not installed): the
 * calling thread's context, which runtime.hip owns and the launchers read (device_launch.h), and
 * the error convention of all.
 */
#ifndef TAMD_DEVICE_CTX_H
#define TAMD_DEVICE_CTX_H

#include <hip/hip_runtime.h>

/* Per host THREAD: the device it works on, its stream, its scratch arena and
 * its blocks of bookkeeping memory.  The reference's rule is one stepper (and one
 * client) per thread over shared maps and stacks [ref include/turtle.h:129-132,
 * :620-626, examples/example-pthread.c:66-125]; here a thread also has a device:
 * the one LOCAL_RANK names (else 0) until it calls turtle_amd_device_set, so one
 * process can drive several GPUs, a thread each.  What threads share -- map
 * nodes, a stack's tiles -- is uploaded per device and changed under one lock
 * (host.h: tamd_geometry_lock). */
struct Ctx {
        int device = -1, cus = 0;
        hipStream_t own_stream = nullptr, stream = nullptr;
        int math_strict = 0;
        int in_flight = 1; /* batches the thread keeps in flight (tamd_dev_in_flight_set) */
        void * scratch = nullptr;
        size_t scratch_size = 0, scratch_used = 0;
        void * block[2] = { nullptr, nullptr }; /* grow-only: the pager's lists, a stack's own tables */
        size_t block_size[2] = { 0, 0 };
        void * pinned = nullptr; /* host memory the device can copy from / to without staging */
        size_t pinned_size = 0;
        void release()
        {
                if (device < 0) return;
                if (hipSetDevice(device) != hipSuccess) return;
                if (own_stream != nullptr) (void)hipStreamSynchronize(own_stream), (void)hipStreamDestroy(own_stream);
                if (scratch != nullptr) (void)hipFree(scratch);
                for (int i = 0; i < 2; i++)
                        if (block[i] != nullptr) (void)hipFree(block[i]);
                if (pinned != nullptr) (void)hipHostFree(pinned);
                pinned = nullptr, pinned_size = 0;
                own_stream = stream = nullptr, scratch = nullptr, scratch_size = scratch_used = 0;
                block[0] = block[1] = nullptr, block_size[0] = block_size[1] = 0;
        }
};

#pragma GCC visibility push(hidden)

/* (constant-initialised, and said to be: a thread's first use runs no constructor, and none is looked for) */
#define TAMD_CONSTINIT __attribute__((require_constant_initialization))
extern TAMD_CONSTINIT thread_local char g_error[512];
extern TAMD_CONSTINIT thread_local Ctx g_ctx;

/* "<prefix><what>: <HIP's text> (HIP error <n>)" as the thread's error text; returns 1 */
int fail(const char * what, hipError_t e, const char * prefix = "");

#pragma GCC visibility pop

#define HIP_TRY(call)                                                          \
        do {                                                                   \
                const hipError_t e_ = (call);                                  \
                if (e_ != hipSuccess) return fail(#call, e_);                  \
        } while (0)

#define LAUNCH_CHECK(name)                                                     \
        do {                                                                   \
                const hipError_t e_ = hipGetLastError();                       \
                if (e_ != hipSuccess) return fail(name, e_, "launch ");       \
        } while (0)

#endif
