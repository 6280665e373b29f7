// Host stand-in for the few HIP names csrc/isosurface_support.hip uses, so that its kernels compile as plain C++ and run as loops
// on the CPU under AddressSanitizer and UBSan (tests/test_isosurface_support_host.py).  A launch visits every (block, thread) in
// turn; an atomic add is a plain add; the reciprocal seed is 1.0 / x (the kernel checks whatever seed it gets); a scalar load is
// a load.  What this cannot show: the device's division, its scalar loads, visibility between workgroups.
// hipMalloc and hipFree are malloc and free -- so that AddressSanitizer sees a buffer freed twice or never -- with an allocator
// that fails on the call a test names (tests/cpp/buffer_growth_host.cpp, for csrc/dmi_buffer.h).  Streams and events are allocations
// too, counted as they are created and destroyed; the number of devices is the test's to set; a copy is a memcpy, a span between two
// events one millisecond (tests/cpp/depth_call_host.cpp, for csrc/dmi_depth_call.h).  An event holds the clock's value when it was
// recorded -- the clock goes on by a millisecond with every record, or to what the test sets --, and the creation of events fails on
// the call a test names, as the allocator does (tests/cpp/mesh_stage_host.cpp, for csrc/dmi_mesh_stage.h).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#define __device__
#define __host__
#define __global__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __restrict__
#define address_space(x)  // (inside __attribute__(( )): an empty attribute)
#define __builtin_amdgcn_rcp(x) (1.0 / (x))
#define __builtin_amdgcn_readfirstlane(x) (x)
typedef int hipError_t;
constexpr hipError_t hipSuccess = 0;
typedef void *hipStream_t;
typedef void *hipEvent_t;
struct dim3 {
  unsigned x, y, z;
  dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {}
};
struct launch_index {
  unsigned x, y, z;
};
inline launch_index blockIdx, threadIdx, gridDim, blockDim;
constexpr hipError_t hipErrorOutOfMemory = 2;
constexpr hipError_t hipErrorNoDevice = 100;
constexpr hipError_t hipErrorInvalidDevice = 101;
constexpr unsigned hipStreamNonBlocking = 1;
constexpr unsigned hipEventDisableTiming = 2;
enum hipDeviceAttribute_t { hipDeviceAttributeMultiprocessorCount };
enum hipMemcpyKind { hipMemcpyHostToDevice, hipMemcpyDeviceToHost, hipMemcpyDeviceToDevice };
struct hip_host_state {
  long mallocs = 0, frees = 0, synchronizes = 0;
  long fail_malloc_at = 0;  // the hipMalloc call (counted from 1) that fails; 0: none
  int devices = 1;          // what hipGetDeviceCount says; below 0: it fails
  int compute_units = 256;
  long device_counts = 0, set_devices = 0, attributes = 0, copies = 0, elapsed_times = 0;
  long streams_created = 0, streams_destroyed = 0, events_created = 0, events_destroyed = 0;
  long event_creations = 0;       // calls, the failed one included
  long fail_event_create_at = 0;  // the creation of an event (counted from 1) that fails; 0: none
  long events_without_timing = 0;
  float clock = 0.f;              // milliseconds: what the next hipEventRecord stamps
};
inline hip_host_state hip_host;
inline hipError_t hipGetLastError() { return hipSuccess; }
inline const char *hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : e == hipErrorOutOfMemory ? "out of memory" : "error"; }
inline hipError_t hipGetDeviceCount(int *n) {
  ++hip_host.device_counts;
  if (hip_host.devices < 0) return hipErrorNoDevice;
  *n = hip_host.devices;
  return hipSuccess;
}
inline hipError_t hipSetDevice(int device) {
  ++hip_host.set_devices;
  return device >= 0 && device < hip_host.devices ? hipSuccess : hipErrorInvalidDevice;
}
inline hipError_t hipDeviceGetAttribute(int *value, hipDeviceAttribute_t, int) {
  ++hip_host.attributes;
  *value = hip_host.compute_units;
  return hipSuccess;
}
inline hipError_t hipStreamCreateWithFlags(hipStream_t *s, unsigned) {
  ++hip_host.streams_created;
  *s = malloc(1);
  return hipSuccess;
}
inline hipError_t hipStreamDestroy(hipStream_t s) {
  ++hip_host.streams_destroyed;
  free(s);
  return hipSuccess;
}
inline hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned flags) {
  if (++hip_host.event_creations == hip_host.fail_event_create_at) return hipErrorOutOfMemory;
  ++hip_host.events_created;
  if (flags & hipEventDisableTiming) ++hip_host.events_without_timing;
  *e = calloc(1, sizeof(float));
  return hipSuccess;
}
inline hipError_t hipEventCreate(hipEvent_t *e) { return hipEventCreateWithFlags(e, 0); }
inline hipError_t hipEventDestroy(hipEvent_t e) {
  ++hip_host.events_destroyed;
  free(e);
  return hipSuccess;
}
inline hipError_t hipEventElapsedTime(float *ms, hipEvent_t start, hipEvent_t stop) {
  ++hip_host.elapsed_times;
  *ms = start && stop ? *static_cast<float *>(stop) - *static_cast<float *>(start) : 1.f;  // (no events: a span all the same)
  return hipSuccess;
}
inline hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind, hipStream_t) {
  ++hip_host.copies;
  memcpy(dst, src, bytes);
  return hipSuccess;
}
inline hipError_t hipMalloc(void **p, size_t bytes) {
  if (++hip_host.mallocs == hip_host.fail_malloc_at) return hipErrorOutOfMemory;
  *p = malloc(bytes ? bytes : 1);
  return *p ? hipSuccess : hipErrorOutOfMemory;
}
inline hipError_t hipFree(void *p) {
  ++hip_host.frees;
  free(p);
  return hipSuccess;
}
inline hipError_t hipStreamSynchronize(hipStream_t) {
  ++hip_host.synchronizes;
  return hipSuccess;
}
inline hipError_t hipEventRecord(hipEvent_t e, hipStream_t) {
  if (!e) return hipSuccess;  // (the kernels' harness has no events)
  *static_cast<float *>(e) = hip_host.clock;
  hip_host.clock += 1.f;
  return hipSuccess;
}
inline hipError_t hipMemsetAsync(void *p, int v, size_t n, hipStream_t) {
  memset(p, v, n);
  return hipSuccess;
}
template <typename T>
inline T atomicAdd(T *p, T v) {
  const T old = *p;
  *p += v;
  return old;
}
#define hipLaunchKernelGGL(kernel, grid, block, shmem, stream, ...)             \
  do {                                                                          \
    const dim3 g_ = (grid), b_ = (block);                                       \
    gridDim = {g_.x, g_.y, g_.z};                                               \
    blockDim = {b_.x, b_.y, b_.z};                                              \
    for (unsigned by_ = 0; by_ < g_.y; ++by_)                                   \
      for (unsigned bx_ = 0; bx_ < g_.x; ++bx_)                                 \
        for (unsigned tx_ = 0; tx_ < b_.x; ++tx_) {                             \
          blockIdx = {bx_, by_, 0};                                             \
          threadIdx = {tx_, 0, 0};                                              \
          kernel(__VA_ARGS__);                                                  \
        }                                                                       \
  } while (0)
