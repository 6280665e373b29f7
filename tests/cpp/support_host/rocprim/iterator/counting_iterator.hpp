// host stand-in (see ../../hip/hip_runtime.h)
#pragma once
#include <cstddef>
namespace rocprim {
template <typename T>
struct counting_iterator {
  T base;
  explicit counting_iterator(T b) : base(b) {}
  T operator[](size_t i) const { return base + (T)i; }
};
}  // namespace rocprim
