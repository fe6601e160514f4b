// dab_reduce.h — fixed-order block reductions and the fixed-point cost commit shared by the
// kernel files. Device code only (included by .hip files).
#pragma once
#include <hip/hip_runtime.h>

#include "dab_kernels.h"
#include "dab_wave.h"

namespace dab {

// Fixed-order sum of K per-thread values over a 256-thread block: four full-mask DPP
// steps give every lane its 16-lane row sum, the 16 row sums go through LDS, and K
// threads add them in order. About 13 VALU per value and wave, against ~22 for a
// full-wave DPP reduction.
__device__ __forceinline__ double row_sum16(double v) {
  v += dpp_full_f64<0xb1>(v);   // quad_perm [1,0,3,2]
  v += dpp_full_f64<0x4e>(v);   // quad_perm [2,3,0,1]
  v += dpp_full_f64<0x141>(v);  // row_half_mirror
  v += dpp_full_f64<0x140>(v);  // row_mirror
  return v;
}
template <int K>
__device__ __forceinline__ void block_reduce_store(double (&acc)[K], double* __restrict__ out) {
  constexpr int R = kRedBlock / 16;  // rows per block
  __shared__ double sh[K][R];
  const int lane = threadIdx.x & 63;
  const int row = threadIdx.x >> 4;
#pragma unroll
  for (int i = 0; i < K; ++i) {
    const double v = row_sum16(acc[i]);
    if ((lane & 15) == 15) sh[i][row] = v;
  }
  __syncthreads();
  if (threadIdx.x < K) {
    double v = sh[threadIdx.x][0];
#pragma unroll
    for (int q = 1; q < R; ++q) v += sh[threadIdx.x][q];
    out[threadIdx.x] = v;
  }
}

// Cost sum as an exact fixed-point integer pair. Each work-group adds its (fixed-order)
// partial sum of r^2 as hi = trunc(p) and lo = (p - hi) * 2^52 with no-return 64-bit
// atomics, and its non-finite count; integer addition is associative, so the total is the
// same bits whatever order the work-groups finish in (bitwise reproducible, identical on
// every rank's copy after an integer all-reduce), and the kernel ends without the
// store-wait-count-load chain of a last-arriver sum (~2.5 us at C3). Same-address atomics
// serialize at the memory side (~12 ns each), so the adds are spread over kFxCopies
// shards of their own lines (8 work-groups per shard at C3). Readers sum the shards and
// convert: cost = hi + lo * 2^-52 (dab_solver.hip: read_scalars). Two shard sets alternate
// between consecutive passes: block 0 of a pass zeroes the set the next pass adds into
// (fx_next), so no memset or extra launch runs in front of the kernel; the set of a pass
// stays valid until the pass after next.
// One lane commits a work-group's cost partial p (sum r^2 >= 0) and its non-finite count b
// to its shard as kFxLimbs 50-bit limbs (dab_kernels.h). Each limb is taken off the top with
// a floor and an exact subtraction (the remainder of a double below 2^(50 (k+1)) after
// removing its multiple of 2^(50 k) is representable), the last one rounded. A finite p of
// 2^150 or more (a residual of ~1e22 px) cannot be held and is counted as non-finite.
__device__ __forceinline__ void cost_fx_commit(double p, double b, unsigned long long* __restrict__ shard) {
  unsigned long long limb[kFxLimbs] = {0, 0, 0, 0, 0};
  if (!(p >= 0.0 && p < 0x1p150)) {
    if (b == 0.0) b = 1.0;
  } else {
    double r = p;
    const double scale[kFxLimbs - 1] = {0x1p-100, 0x1p-50, 1.0, 0x1p50};
#pragma unroll
    for (int k = 0; k < kFxLimbs - 1; ++k) {
      const double l = floor(r * scale[k]);
      limb[k] = (unsigned long long)l;
      r -= l / scale[k];  // exact
    }
    limb[kFxLimbs - 1] = (unsigned long long)rint(r * 0x1p100);
  }
#pragma unroll
  for (int k = 0; k < kFxLimbs; ++k)
    if (limb[k]) __hip_atomic_fetch_add(shard + k, limb[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (b != 0.0) __hip_atomic_fetch_add(shard + kFxBad, (unsigned long long)b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace dab
