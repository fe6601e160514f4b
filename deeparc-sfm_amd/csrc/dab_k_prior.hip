// dab_k_prior.hip — Gaussian priors on camera extrinsics (dab_set_ext_priors): the residual
// block r = A (x_e - mu) of Ceres' NormalPrior, folded into the per-camera row ug = [U | g_c]
// after the evaluation pass and its sum over the ranks, and into the candidate pass's scalars
// after theirs. Everything downstream of an evaluation reads the camera blocks through ug, so no
// other kernel knows about priors. Launched only for a non-empty effective set. Every camera slot
// has one owner lane and every sum a fixed order (no floating-point atomics): two runs agree
// bitwise.
#include <hip/hip_runtime.h>

#include "dab_arrive.h"
#include "dab_kernels.h"
#include "dab_warm.h"
#include "dab_wave.h"

namespace dab {

namespace {
constexpr int kBlk = 256;
constexpr int kPerBlock = kBlk / 27;  // priors per work-group of k_prior_blocks: one lane per ug slot

// r = A (x - mean) of one record
__device__ inline void prior_residual(const double* __restrict__ rec, const double* __restrict__ x, double r[6]) {
  double d[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) d[k] = x[k] - rec[k];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double a = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) a += rec[6 + 6 * i + k] * d[k];
    r[i] = a;
  }
}
__device__ inline double sum_sq6(const double r[6]) {
  double a = 0.0;
#pragma unroll
  for (int i = 0; i < 6; ++i) a += r[i] * r[i];
  return a;
}
}  // namespace

// Lane (prior, slot) owns slot 0..26 of that prior's camera row, kPerBlock priors per work-group.
// Slots 0..20 add A^T A, slots 21..26 add (A^T r)_k; the lane of slot 21 leaves the prior's
// 0.5 |r|^2 in part[prior], and the last work-group to arrive adds them in a fixed order.
__global__ __launch_bounds__(kBlk) void k_prior_blocks(int n, const int2* __restrict__ idx,
                                                       const double* __restrict__ rec,
                                                       const double* __restrict__ ext, double* __restrict__ ug,
                                                       double* __restrict__ part, unsigned* __restrict__ cnt,
                                                       double* __restrict__ cost) {
  const int t = threadIdx.x, lp = t / 27, slot = t - 27 * lp;
  const int p = blockIdx.x * kPerBlock + lp;
  if (lp < kPerBlock && p < n) {
    const int2 ec = idx[p];
    const double* R = rec + (size_t)kPriorRec * p;
    double* row = ug + 27 * (size_t)ec.y;
    if (slot < 21) {
      row[slot] += R[42 + slot];
    } else {
      const int k = slot - 21;
      double r[6];
      prior_residual(R, ext + 6 * (size_t)ec.x, r);
      double g = 0.0;
#pragma unroll
      for (int i = 0; i < 6; ++i) g += R[6 + 6 * i + k] * r[i];
      row[slot] += g;
      if (k == 0) part_store(part, (size_t)p, 0.5 * sum_sq6(r));
    }
  }
  if (!arrive_last(cnt)) return;
  double total[1];
  part_sum<kBlk / 64, 1>(part, n, total);
  if (t == 0) {
    cost[0] = total[0];
    __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// One lane per prior, one wave per work-group; the last work-group to arrive adds the priors' terms
// in a fixed order and folds them into the candidate pass's scalars.
__global__ __launch_bounds__(64) void k_prior_candidate(int n, const int2* __restrict__ idx,
                                                        const double* __restrict__ rec,
                                                        const double* __restrict__ ext,
                                                        const double* __restrict__ ext_c,
                                                        const double* __restrict__ dc, double* __restrict__ part,
                                                        unsigned* __restrict__ cnt, double* __restrict__ model) {
  const int p = blockIdx.x * 64 + threadIdx.x;
  if (p < n) {
    const int2 ec = idx[p];
    const double* R = rec + (size_t)kPriorRec * p;
    double r[6], rc[6];
    prior_residual(R, ext + 6 * (size_t)ec.x, r);
    prior_residual(R, ext_c + 6 * (size_t)ec.x, rc);
    const double* d = dc + 6 * (size_t)ec.y;
    double a = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      double m = 0.0;
#pragma unroll
      for (int k = 0; k < 6; ++k) m += R[6 + 6 * i + k] * d[k];
      a -= m * (r[i] + 0.5 * m);
    }
    part_store(part, 2 * (size_t)p, a);
    part_store(part, 2 * (size_t)p + 1, sum_sq6(rc));
  }
  if (!arrive_last(cnt)) return;
  double sum[2];
  part_sum<1, 2>(part, n, sum);
  if (threadIdx.x == 0) {
    model[0] += sum[0];
    model[1] += sum[1];
    if (!isfinite(sum[1])) model[2] += 1.0;
    __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ __launch_bounds__(256) void k_prior_eval(int n, const int2* __restrict__ idx,
                                                    const double* __restrict__ rec, const double* __restrict__ ext,
                                                    double* __restrict__ res) {
  __shared__ double sh[256];
  const int t = threadIdx.x;
  double total = 0.0;
  for (int base = 0; base < n; base += 256) {
    const int p = base + t;
    if (p < n) {
      double r[6];
      prior_residual(rec + (size_t)kPriorRec * p, ext + 6 * (size_t)idx[p].x, r);
#pragma unroll
      for (int i = 0; i < 6; ++i) res[6 * (size_t)p + i] = r[i];
      sh[t] = 0.5 * sum_sq6(r);
    }
    __syncthreads();
    if (t == 0) {
      const int m = min(256, n - base);
      for (int j = 0; j < m; ++j) total += sh[j];
    }
    __syncthreads();
  }
  if (t == 0) res[6 * (size_t)n] = total;
}

void launch_prior_blocks(hipStream_t s, int n, const int2* idx, const double* rec, const double* ext, double* ug,
                         double* part, unsigned* cnt, double* cost) {
  if (n <= 0) return;
  k_prior_blocks<<<(n + kPerBlock - 1) / kPerBlock, kBlk, 0, s>>>(n, idx, rec, ext, ug, part, cnt, cost);
}
void launch_prior_candidate(hipStream_t s, int n, const int2* idx, const double* rec, const double* ext,
                            const double* ext_c, const double* delta_c, double* part, unsigned* cnt, double* model) {
  if (n <= 0) return;
  k_prior_candidate<<<(n + 63) / 64, 64, 0, s>>>(n, idx, rec, ext, ext_c, delta_c, part, cnt, model);
}
void launch_prior_eval(hipStream_t s, int n, const int2* idx, const double* rec, const double* ext, double* res) {
  if (n <= 0) return;
  k_prior_eval<<<1, 256, 0, s>>>(n, idx, rec, ext, res);
}

DAB_WARM_TU(k_prior_blocks);

}  // namespace dab
