// host stand-in: rocprim::exclusive_scan as a sequential loop (see ../../hip/hip_runtime.h)
#pragma once
#include <hip/hip_runtime.h>
namespace rocprim {
template <typename T>
struct plus {
  T operator()(T a, T b) const { return a + b; }
};
template <typename In, typename Out, typename T, typename Op>
hipError_t exclusive_scan(void *temp, size_t &bytes, In in, Out out, T init, size_t n, Op op, hipStream_t) {
  if (!temp) {
    bytes = 64;
    return hipSuccess;
  }
  T acc = init;
  for (size_t i = 0; i < n; ++i) {
    const T v = in[i];
    out[i] = acc;
    acc = op(acc, v);
  }
  return hipSuccess;
}
}  // namespace rocprim
