// dab_warm.h — code-object warm-up. hipcc emits one code object per translation unit and the
// runtime loads each at the first launch of one of its kernels (10-40 ms, otherwise inside a
// process's first LM iteration or first covariance call). Every .hip file with __global__ code
// places DAB_WARM_TU(one of its kernels) once, at namespace scope; dab_create walks the table
// with hipFuncGetAttributes, once per device, which loads every object then.
#pragma once

namespace dab {

constexpr int kWarmMax = 32;  // translation units with kernels (at most)
struct WarmTable {
  const void* fn[kWarmMax];
  int n;  // registrations, also those past kWarmMax: dab_create then fails (raise kWarmMax)
};
WarmTable& warm_table();  // dab_handle.hip (a function-local static: filled during static initialisation)
struct WarmEntry {
  explicit WarmEntry(const void* f) {
    WarmTable& t = warm_table();
    if (t.n < kWarmMax) t.fn[t.n] = f;
    ++t.n;
  }
};
#define DAB_WARM_TU(...) static const ::dab::WarmEntry dab_warm_entry_{reinterpret_cast<const void*>(__VA_ARGS__)}

}  // namespace dab
