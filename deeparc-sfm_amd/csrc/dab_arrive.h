// dab_arrive.h — the fixed-order grid sum of the prior kernels (dab_k_prior.hip, dab_k_ptprior.hip):
// every work-group leaves its terms write-through, the last one to arrive adds them in a fixed
// order. No floating-point atomics: two runs agree bitwise.
#pragma once
#include <hip/hip_runtime.h>

#include "dab_wave.h"

namespace dab {

// The last work-group to arrive (true in all its threads). Every value the caller's threads
// stored for it went out write-through (agent-scope atomic stores) and is drained here before the
// arrival count; the last work-group reads them back with agent-scope atomic loads: no
// release/acquire fences, no waits (store_cost_partial_last's hand-off in dab_k_points.hip).
// *cnt is zero between launches: the last work-group puts it back, and prior_sync zeroes it before
// every call that launches these kernels.
__device__ inline bool arrive_last(unsigned* __restrict__ cnt) {
  __shared__ int last;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0)
    last = __hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
  __syncthreads();
  return last != 0;
}
__device__ inline void part_store(double* __restrict__ part, size_t i, double v) {
  __hip_atomic_store(reinterpret_cast<unsigned long long*>(part) + i, (unsigned long long)__double_as_longlong(v),
                     __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// Fixed-order sum of part[K * p + k], p < n, over one work-group of NW waves: thread t takes p = t,
// t + 64 NW, ..., a DPP wave sum, then the waves in order. The total is returned in thread 0.
template <int NW, int K>
__device__ inline void part_sum(const double* __restrict__ part, int n, double (&out)[K]) {
  __shared__ double red[K][NW];
  const unsigned long long* pp = reinterpret_cast<const unsigned long long*>(part);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double v = 0.0;
    for (int p = threadIdx.x; p < n; p += 64 * NW)
      v += __longlong_as_double(
          (long long)__hip_atomic_load(pp + (size_t)K * p + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    const double t = wave_sum_lane63(v);
    if (lane == 63) red[k][w] = t;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double t = red[k][0];
#pragma unroll
    for (int q = 1; q < NW; ++q) t += red[k][q];
    out[k] = t;
  }
}

}  // namespace dab
