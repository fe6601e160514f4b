// dab_k_zprior.hip — Gaussian priors on camera intrinsics (dab_set_intr_priors): the residual
// block r = A (x_i - mu) of Ceres' NormalPrior over the active slots of a free intrinsic, folded
// into zg = [U_zz | g_z] after k_intr_eval and its sum over the ranks, and into the candidate
// pass's scalars after theirs. Everything downstream of an evaluation reads the intrinsic blocks
// through zg (k_intr_scatter, launch_intr_scale, k_intr_candidate), so no other kernel knows
// about these priors. The host zeroes the inactive columns of A and the inactive entries of mu in
// the records, so no kernel here needs the mask bits. At most kIntrFreeMax records: every kernel
// is one work-group, every zg slot has one owner lane and every sum runs in record order in one
// thread (no arrival counter, no floating-point atomics): two runs agree bitwise. Launched only
// for a non-empty effective set.
#include <hip/hip_runtime.h>

#include "dab_kernels.h"
#include "dab_warm.h"

namespace dab {

namespace {
constexpr int kZBlk = 448;  // 7 waves >= kIntrFreeMax * 27 owner lanes of k_zprior_blocks
static_assert(kZBlk >= kIntrFreeMax * 27 && kZBlk % 64 == 0, "k_zprior_blocks: one lane per zg slot");
static_assert(kIntrFreeMax <= 64, "k_zprior_candidate / k_zprior_eval: one lane per record in one wave");

// r = A (x - mean) of one record (rec = mean | A row-major | A^T A); x: the 6 slots of the
// intrinsic in the device layout (cx cy fx fy' k0 k1). An inactive slot meets a zero column.
__device__ inline void zprior_residual(const double* __restrict__ rec, const double* __restrict__ x, double r[6]) {
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
__device__ inline double zprior_sq(const double r[6]) {
  double a = 0.0;
#pragma unroll
  for (int i = 0; i < 6; ++i) a += r[i] * r[i];
  return a;
}
}  // namespace

// Lane (record, slot) owns slot 0..26 of that record's zg row. Slots 0..20 add A^T A, slots
// 21..26 add (A^T r)_k; the lane of slot 21 leaves the record's 0.5 |r|^2 in LDS and thread 0 adds
// them in record order.
__global__ __launch_bounds__(kZBlk) void k_zprior_blocks(int n, const int2* __restrict__ idx,
                                                         const double* __restrict__ rec,
                                                         const double* __restrict__ intr, double* __restrict__ zg,
                                                         double* __restrict__ cost) {
  __shared__ double half_sq[kIntrFreeMax];
  const int t = threadIdx.x, p = t / 27, slot = t - 27 * p;
  if (p < n && p < kIntrFreeMax) {
    const int2 ic = idx[p];
    const double* R = rec + (size_t)kPriorRec * p;
    double* row = zg + (size_t)kIntrRec * ic.y;
    if (slot < 21) {
      row[slot] += R[42 + slot];
    } else {
      const int k = slot - 21;
      double r[6];
      zprior_residual(R, intr + (size_t)kIntr * ic.x, r);
      double g = 0.0;
#pragma unroll
      for (int i = 0; i < 6; ++i) g += R[6 + 6 * i + k] * r[i];
      row[slot] += g;
      if (k == 0) half_sq[p] = 0.5 * zprior_sq(r);
    }
  }
  __syncthreads();
  if (t == 0) {
    double total = 0.0;
    for (int j = 0; j < n && j < kIntrFreeMax; ++j) total += half_sq[j];
    cost[0] = total;
  }
}

// One lane per record, one wave; lane 0 adds the records' terms in record order and folds them
// into the candidate pass's scalars.
__global__ __launch_bounds__(64) void k_zprior_candidate(int n, const int2* __restrict__ idx,
                                                         const double* __restrict__ rec,
                                                         const double* __restrict__ intr,
                                                         const double* __restrict__ intr_c,
                                                         const double* __restrict__ dz, double* __restrict__ model) {
  __shared__ double term[2][kIntrFreeMax];
  const int p = threadIdx.x;
  if (p < n && p < kIntrFreeMax) {
    const int2 ic = idx[p];
    const double* R = rec + (size_t)kPriorRec * p;
    double r[6], rc[6];
    zprior_residual(R, intr + (size_t)kIntr * ic.x, r);
    zprior_residual(R, intr_c + (size_t)kIntr * ic.x, rc);
    const double* d = dz + 6 * (size_t)ic.y;
    double a = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      double m = 0.0;
#pragma unroll
      for (int k = 0; k < 6; ++k) m += R[6 + 6 * i + k] * d[k];
      a -= m * (r[i] + 0.5 * m);
    }
    term[0][p] = a;
    term[1][p] = zprior_sq(rc);
  }
  __syncthreads();
  if (p == 0) {
    double sum[2] = {0.0, 0.0};
    for (int j = 0; j < n && j < kIntrFreeMax; ++j) {
      sum[0] += term[0][j];
      sum[1] += term[1][j];
    }
    model[0] += sum[0];
    model[1] += sum[1];
    if (!isfinite(sum[1])) model[2] += 1.0;
  }
}

__global__ __launch_bounds__(64) void k_zprior_eval(int n, const int2* __restrict__ idx,
                                                    const double* __restrict__ rec, const double* __restrict__ intr,
                                                    double* __restrict__ res) {
  __shared__ double half_sq[kIntrFreeMax];
  const int p = threadIdx.x;
  if (p < n && p < kIntrFreeMax) {
    double r[6];
    zprior_residual(rec + (size_t)kPriorRec * p, intr + (size_t)kIntr * idx[p].x, r);
#pragma unroll
    for (int i = 0; i < 6; ++i) res[6 * (size_t)p + i] = r[i];
    half_sq[p] = 0.5 * zprior_sq(r);
  }
  __syncthreads();
  if (p == 0) {
    double total = 0.0;
    for (int j = 0; j < n && j < kIntrFreeMax; ++j) total += half_sq[j];
    res[6 * (size_t)n] = total;
  }
}

void launch_zprior_blocks(hipStream_t s, int n, const int2* idx, const double* rec, const double* intr, double* zg,
                          double* cost) {
  if (n <= 0) return;
  k_zprior_blocks<<<1, kZBlk, 0, s>>>(n, idx, rec, intr, zg, cost);
}
void launch_zprior_candidate(hipStream_t s, int n, const int2* idx, const double* rec, const double* intr,
                             const double* intr_c, const double* dz, double* model) {
  if (n <= 0) return;
  k_zprior_candidate<<<1, 64, 0, s>>>(n, idx, rec, intr, intr_c, dz, model);
}
void launch_zprior_eval(hipStream_t s, int n, const int2* idx, const double* rec, const double* intr, double* res) {
  if (n <= 0) return;
  k_zprior_eval<<<1, 64, 0, s>>>(n, idx, rec, intr, res);
}

DAB_WARM_TU(k_zprior_blocks);

}  // namespace dab
