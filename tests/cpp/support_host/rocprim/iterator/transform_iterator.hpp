// host stand-in (see ../../hip/hip_runtime.h)
#pragma once
#include <cstddef>
namespace rocprim {
template <typename It, typename F>
struct transform_iterator {
  It it;
  F f;
  auto operator[](size_t i) const { return f(it[i]); }
};
template <typename It, typename F>
transform_iterator<It, F> make_transform_iterator(It it, F f) {
  return {it, f};
}
}  // namespace rocprim
