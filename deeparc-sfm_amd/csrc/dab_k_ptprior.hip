// dab_k_ptprior.hip — Gaussian priors on points (dab_set_point_priors): the residual block
// r = A (X_p - mu) of Ceres' NormalPrior, folded into the point blocks V | g after every evaluation
// pass, and into the candidate pass's scalars before their sum over the ranks (a point belongs to
// one rank). Everything downstream of an evaluation reads the point blocks through V | g, so no
// other kernel knows about point priors. Launched only for a non-empty effective set.
//
// Up to NP priors: one lane per prior, consecutive lanes on consecutive priors, records planar
// [kPtPriorRec][n] and sorted by device point, so every record load is coalesced and the V | g
// read-modify-writes walk the planes in ascending order. Every V | g slot has one owner lane (at
// most one prior per point) and every sum a fixed order (no floating-point atomics): two runs
// agree bitwise, whatever order the priors were set in.
#include <hip/hip_runtime.h>

#include "dab_arrive.h"
#include "dab_kernels.h"
#include "dab_warm.h"
#include "dab_wave.h"

namespace dab {

namespace {
constexpr int kBlk = kPtPriorBlock;
constexpr int kNW = kBlk / 64;

struct PtRec {
  double mu[3], A[9];
};
__device__ inline void load_rec(const double* __restrict__ rec, size_t n, size_t i, PtRec& R) {
#pragma unroll
  for (int k = 0; k < 3; ++k) R.mu[k] = rec[k * n + i];
#pragma unroll
  for (int k = 0; k < 9; ++k) R.A[k] = rec[(3 + k) * n + i];
}
// r = A (x - mu)
__device__ inline void residual(const PtRec& R, const double* __restrict__ x, double r[3]) {
  const double d0 = x[0] - R.mu[0], d1 = x[1] - R.mu[1], d2 = x[2] - R.mu[2];
#pragma unroll
  for (int i = 0; i < 3; ++i) r[i] = R.A[3 * i] * d0 + R.A[3 * i + 1] * d1 + R.A[3 * i + 2] * d2;
}
// Fixed-order sums of K values per thread over the work-group, left in part[K * blockIdx.x + k]
// (write-through, for the last work-group to arrive)
template <int K>
__device__ inline void group_part_store(const double (&v)[K], double* __restrict__ part) {
  __shared__ double red[K][kNW];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const double t = wave_sum_lane63(v[k]);
    if (lane == 63) red[k][w] = t;
  }
  __syncthreads();
  if (threadIdx.x < K) {
    double t = red[threadIdx.x][0];
#pragma unroll
    for (int q = 1; q < kNW; ++q) t += red[threadIdx.x][q];
    part_store(part, (size_t)K * blockIdx.x + threadIdx.x, t);
  }
}
}  // namespace

// V[k][p] += (A^T A)_k, g[k][p] += (A^T r)_k; *cost = 0.5 sum |r|^2 (work-group sums, then the
// last work-group to arrive adds those in a fixed order)
__global__ __launch_bounds__(kBlk) void k_pt_prior_blocks(int n, int NP, const int* __restrict__ idx,
                                                          const double* __restrict__ rec,
                                                          const double* __restrict__ points, double* __restrict__ V,
                                                          double* __restrict__ g, double* __restrict__ part,
                                                          unsigned* __restrict__ cnt, double* __restrict__ cost) {
  const int i = blockIdx.x * kBlk + threadIdx.x;
  double c[1] = {0.0};
  if (i < n) {
    const size_t ns = (size_t)n, NPs = (size_t)NP;
    const int p = idx[i];
    PtRec R;
    load_rec(rec, ns, (size_t)i, R);
    double r[3];
    residual(R, points + 3 * (size_t)p, r);
#pragma unroll
    for (int k = 0; k < 6; ++k) V[k * NPs + p] += rec[(12 + k) * ns + i];
#pragma unroll
    for (int k = 0; k < 3; ++k) g[k * NPs + p] += R.A[k] * r[0] + R.A[3 + k] * r[1] + R.A[6 + k] * r[2];
    c[0] = 0.5 * (r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
  }
  group_part_store<1>(c, part);
  if (!arrive_last(cnt)) return;
  double total[1];
  part_sum<kNW, 1>(part, (int)gridDim.x, total);
  if (threadIdx.x == 0) {
    cost[0] = total[0];
    __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// With m = A delta_p (delta_p the unscaled point step, dp[3][NP]) and x_c the candidate point:
// model[0] += -sum m.(r + m/2), model[1] += sum |A (x_c - mu)|^2, model[2] += 1 when that sum is not
// finite. model = this rank's d_scal + S_MODEL after the candidate pass's final sum and before its
// sum over the ranks.
__global__ __launch_bounds__(kBlk) void k_pt_prior_candidate(int n, int NP, const int* __restrict__ idx,
                                                             const double* __restrict__ rec,
                                                             const double* __restrict__ points,
                                                             const double* __restrict__ points_c,
                                                             const double* __restrict__ dp, double* __restrict__ part,
                                                             unsigned* __restrict__ cnt, double* __restrict__ model) {
  const int i = blockIdx.x * kBlk + threadIdx.x;
  double c[2] = {0.0, 0.0};
  if (i < n) {
    const size_t NPs = (size_t)NP;
    const int p = idx[i];
    PtRec R;
    load_rec(rec, (size_t)n, (size_t)i, R);
    double r[3], rc[3];
    residual(R, points + 3 * (size_t)p, r);
    residual(R, points_c + 3 * (size_t)p, rc);
    const double d0 = dp[p], d1 = dp[NPs + p], d2 = dp[2 * NPs + p];
    double a = 0.0;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const double m = R.A[3 * q] * d0 + R.A[3 * q + 1] * d1 + R.A[3 * q + 2] * d2;
      a -= m * (r[q] + 0.5 * m);
    }
    c[0] = a;
    c[1] = rc[0] * rc[0] + rc[1] * rc[1] + rc[2] * rc[2];
  }
  group_part_store<2>(c, part);
  if (!arrive_last(cnt)) return;
  double sum[2];
  part_sum<kNW, 2>(part, (int)gridDim.x, sum);
  if (threadIdx.x == 0) {
    model[0] += sum[0];
    model[1] += sum[1];
    if (!isfinite(sum[1])) model[2] += 1.0;
    __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// res[3 i + k] = r of effective prior i (device point order), res[3 n] = 0.5 sum |r|^2 (one
// work-group, fixed order)
__global__ __launch_bounds__(kBlk) void k_pt_prior_eval(int n, const int* __restrict__ idx,
                                                        const double* __restrict__ rec,
                                                        const double* __restrict__ points, double* __restrict__ res) {
  __shared__ double red[kNW];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += kBlk) {
    PtRec R;
    load_rec(rec, (size_t)n, (size_t)i, R);
    double r[3];
    residual(R, points + 3 * (size_t)idx[i], r);
#pragma unroll
    for (int k = 0; k < 3; ++k) res[3 * (size_t)i + k] = r[k];
    acc += 0.5 * (r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
  }
  const double t = wave_sum_lane63(acc);
  if (lane == 63) red[w] = t;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = red[0];
#pragma unroll
    for (int q = 1; q < kNW; ++q) s += red[q];
    res[3 * (size_t)n] = s;
  }
}

void launch_pt_prior_blocks(hipStream_t s, int n, int NP, const int* idx, const double* rec, const double* points,
                            double* V, double* g, double* part, unsigned* cnt, double* cost) {
  if (n <= 0) return;
  k_pt_prior_blocks<<<pt_prior_groups(n), kBlk, 0, s>>>(n, NP, idx, rec, points, V, g, part, cnt, cost);
}
void launch_pt_prior_candidate(hipStream_t s, int n, int NP, const int* idx, const double* rec, const double* points,
                               const double* points_c, const double* delta_p, double* part, unsigned* cnt,
                               double* model) {
  if (n <= 0) return;
  k_pt_prior_candidate<<<pt_prior_groups(n), kBlk, 0, s>>>(n, NP, idx, rec, points, points_c, delta_p, part, cnt,
                                                           model);
}
void launch_pt_prior_eval(hipStream_t s, int n, const int* idx, const double* rec, const double* points, double* res) {
  if (n <= 0) return;
  k_pt_prior_eval<<<1, kBlk, 0, s>>>(n, idx, rec, points, res);
}

DAB_WARM_TU(k_pt_prior_blocks);

}  // namespace dab
