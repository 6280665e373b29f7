// dmi_buffer.h -- the device allocations of both contexts (dmi_context.h, dmi_color_context.h): a pointer with its capacity in
// bytes, and the rules by which one grows and is freed.  Needs nothing but the HIP runtime's names, so the rules also run on the
// CPU against an allocator that fails on demand (tests/test_fusion_launch_host.py).  Private: never installed.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <initializer_list>

namespace dmi {

// A grow-only device allocation of the context: the pointer and its capacity travel together (one std::swap exchanges two
// buffers whole).  Grown by grow_buffer (ensure_buffer), freed by its group's release(); owns nothing by itself.
struct DeviceBuffer {
  void *ptr = nullptr;
  uint64_t capacity = 0;  // bytes
  template <typename T>
  T *as() const { return static_cast<T *>(ptr); }
};

inline bool holds(const DeviceBuffer &buffer, uint64_t bytes) { return buffer.ptr && buffer.capacity >= bytes; }
// The growth rule of every context: a buffer that holds `bytes` is kept, any other is freed and allocated at exactly `bytes`; the
// old contents are not kept.  A failure leaves it empty with capacity 0, so that the next call allocates again.
inline hipError_t grow_buffer(DeviceBuffer &buffer, uint64_t bytes) {
  if (holds(buffer, bytes)) return hipSuccess;
  hipError_t e = buffer.ptr ? hipFree(buffer.ptr) : hipSuccess;
  buffer = DeviceBuffer{};
  if (e == hipSuccess) e = hipMalloc(&buffer.ptr, (size_t)bytes);
  if (e == hipSuccess) buffer.capacity = bytes; else buffer.ptr = nullptr;
  return e;
}

// ... and the same for a group's events
template <size_t N>
void destroy_events(hipEvent_t (&events)[N]) {
  for (hipEvent_t &e : events) {
    if (e) (void)hipEventDestroy(e);
    e = nullptr;
  }
}

// what every group's release() is made of (the caller has selected the device)
inline void free_buffers(std::initializer_list<DeviceBuffer *> buffers) {
  for (DeviceBuffer *b : buffers) {
    if (b->ptr) (void)hipFree(b->ptr);
    *b = DeviceBuffer{};
  }
}

// ---- the same with the owner's byte count following: `held` is the sum of the capacities of the owner's buffers ----

inline hipError_t grow_buffer(DeviceBuffer &buffer, uint64_t bytes, uint64_t &held) {
  const uint64_t before = buffer.capacity;
  const hipError_t e = grow_buffer(buffer, bytes);
  held += buffer.capacity - before;  // (what was freed has left even when the allocation failed)
  return e;
}
inline void free_buffers(std::initializer_list<DeviceBuffer *> buffers, uint64_t &held) {
  for (DeviceBuffer *b : buffers) held -= b->capacity;
  free_buffers(buffers);
}

// The growth rule of buffers that work queued on `stream` may still read (the tables of a fusion launch): buffers that hold what
// is needed are kept -- no call of the runtime at all --; otherwise the stream is synchronised if any of them is in use, ALL are
// freed and ALL allocated anew at `allocate` bytes (>= needed: a table that grows often asks for more than it needs), as a unit:
// after a failure every one of them is empty with capacity 0, never some new and some old.  The old contents are not kept.
// *fresh (optional) says whether the buffers are new, for the caller that fills them once.
struct BufferGrowth {
  DeviceBuffer *buffer;
  uint64_t needed, allocate;  // bytes
};
inline hipError_t grow_idle_buffers(std::initializer_list<BufferGrowth> unit, hipStream_t stream, uint64_t &held, bool *fresh = nullptr) {
  bool enough = true, in_use = false;
  for (const BufferGrowth &g : unit) {
    enough = enough && holds(*g.buffer, g.needed);
    in_use = in_use || g.buffer->ptr;
  }
  if (fresh) *fresh = !enough;
  if (enough) return hipSuccess;
  hipError_t e = in_use ? hipStreamSynchronize(stream) : hipSuccess;
  for (const BufferGrowth &g : unit) free_buffers({g.buffer}, held);  // (hipFree waits for the device by itself should the stream have failed)
  for (const BufferGrowth &g : unit)
    if (e == hipSuccess) e = grow_buffer(*g.buffer, g.allocate, held);
  if (e != hipSuccess)
    for (const BufferGrowth &g : unit) free_buffers({g.buffer}, held);
  return e;
}

}  // namespace dmi
