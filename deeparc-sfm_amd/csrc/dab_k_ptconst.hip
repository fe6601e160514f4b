// dab_k_ptconst.hip — constant points (dab_set_points_constant): the masked forms of the small
// point-side kernels of the LM step and of the covariance, and the camera step of a problem
// without any free point (k_cam_block_solve). The unmasked kernels (dab_k_step.hip,
// dab_solver.hip, dab_cov.hip) are untouched and run whenever the constant set is empty; a free
// point goes through the same arithmetic here as there, operation for operation.
#include <hip/hip_runtime.h>

#include "dab_kernels.h"
#include "dab_reduce.h"
#include "dab_warm.h"

namespace dab {

// k_point_factor over the free points; a constant point gets PU = 0 and q = 0 and never raises
// the fail flag (with radius = inf, the covariance's call, its undamped block need not factor)
__global__ __launch_bounds__(256) void k_point_factor_m(DevView v, const double* __restrict__ V,
                                                        const double* __restrict__ g,
                                                        const double* __restrict__ sp, StepScalars sc,
                                                        double* __restrict__ L, double* __restrict__ q,
                                                        int* __restrict__ fail,
                                                        const uint8_t* __restrict__ mask) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= v.NP) return;
  double* pu = L + 6 * (size_t)p;
  if (mask[p]) {
#pragma unroll
    for (int k = 0; k < 6; ++k) pu[k] = 0.0;
    reinterpret_cast<double2*>(q)[2 * (size_t)p] = make_double2(0.0, 0.0);
    reinterpret_cast<double2*>(q)[2 * (size_t)p + 1] = make_double2(0.0, 0.0);
    return;
  }
  const size_t NPs = (size_t)v.NP;
  const double s0 = sp[p], s1 = sp[NPs + p], s2 = sp[2 * NPs + p];
  double v00 = s0 * V[p] * s0, v01 = s0 * V[NPs + p] * s1, v02 = s0 * V[2 * NPs + p] * s2;
  double v11 = s1 * V[3 * NPs + p] * s1, v12 = s1 * V[4 * NPs + p] * s2, v22 = s2 * V[5 * NPs + p] * s2;
  auto lmd = [&](double d) {  // LM diagonal: clamp(diag(Js^T Js)) / radius
    d = fmin(fmax(d, sc.min_diag), sc.max_diag);
    const double D = sqrt(d / sc.radius);
    return D * D;
  };
  v00 += lmd(v00);
  v11 += lmd(v11);
  v22 += lmd(v22);
  bool ok = v00 > 0.0;
  const double l00 = sqrt(v00);
  const double l10 = v01 / l00, l20 = v02 / l00;
  const double d1 = v11 - l10 * l10;
  ok = ok && d1 > 0.0;
  const double l11 = sqrt(d1);
  const double l21 = (v12 - l20 * l10) / l11;
  const double d2 = v22 - l20 * l20 - l21 * l21;
  ok = ok && d2 > 0.0;
  const double l22 = sqrt(d2);
  const double gs0 = s0 * g[p], gs1 = s1 * g[NPs + p], gs2 = s2 * g[2 * NPs + p];
  const double q0 = gs0 / l00;
  const double q1 = (gs1 - l10 * q0) / l11;
  const double q2 = (gs2 - l20 * q0 - l21 * q1) / l22;
  ok = ok && isfinite(q0) && isfinite(q1) && isfinite(q2);
  if (!ok) atomicOr(fail, 1);
  const double ia = 1.0 / l00, ic = 1.0 / l11, iff = 1.0 / l22;
  const double ib = -l10 * ia * ic;
  const double ie = -l21 * ic * iff;
  const double id = -(l20 * ia + l21 * ib) * iff;
  pu[0] = s0 * ia;
  pu[1] = s0 * ib;
  pu[2] = s0 * id;
  pu[3] = s1 * ic;
  pu[4] = s1 * ie;
  pu[5] = s2 * iff;
  reinterpret_cast<double2*>(q)[2 * (size_t)p] = make_double2(q0, q1);
  reinterpret_cast<double2*>(q)[2 * (size_t)p + 1] = make_double2(q2, 0.0);
}

// k_scale_points; a constant point has no Jacobi scale of its own (1, read by nothing that counts)
__global__ void k_scale_points_m(int NP, const double* __restrict__ V, double* __restrict__ sp, int on,
                                 const uint8_t* __restrict__ mask) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 3 * NP) return;
  const int k = i / NP, p = i - k * NP;
  const int vi = k == 0 ? 0 : (k == 1 ? 3 : 5);
  sp[i] = (on && !mask[p]) ? 1.0 / (1.0 + sqrt(V[(size_t)vi * NP + p])) : 1.0;
}

// k_axpy_points; a constant point's candidate is its x, bit for bit, whatever d holds, and it
// adds nothing to the step norm or to the candidate's norm
__global__ __launch_bounds__(256) void k_axpy_points_m(int NP, const double* __restrict__ x,
                                                       const double* __restrict__ d, double* __restrict__ xc,
                                                       double* __restrict__ partial,
                                                       const uint8_t* __restrict__ mask) {
  double acc[2] = {0.0, 0.0};
  const size_t NPs = (size_t)NP;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < 3 * NP; i += gridDim.x * blockDim.x) {
    const int p = i / 3, k = i - 3 * (i / 3);
    const double xv = x[i];
    if (mask[p]) {
      xc[i] = xv;
      continue;
    }
    const double c = xv + d[k * NPs + p];
    xc[i] = c;
    const double dd = xv - c;
    acc[0] += dd * dd;
    acc[1] += c * c;
  }
  block_reduce_store<2>(acc, partial + 2 * (size_t)blockIdx.x);
}

// k_grad_points over the free points
__global__ __launch_bounds__(256) void k_grad_points_m(int NP, const double* __restrict__ x,
                                                       const double* __restrict__ g, double* __restrict__ partial,
                                                       const uint8_t* __restrict__ mask) {
  double acc[3] = {0.0, 0.0, 0.0};
  const size_t NPs = (size_t)NP;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < 3 * NP; i += gridDim.x * blockDim.x) {
    const int p = i / 3, k = i - 3 * (i / 3);
    if (mask[p]) continue;
    const double xv = x[i];
    const double d = xv - (xv + (-g[k * NPs + p]));
    acc[0] = fmax(acc[0], fabs(d));
    acc[1] += d * d;
    acc[2] += xv * xv;
  }
  __shared__ double shm[kRedBlock / 64];
  double m = acc[0];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_xor(m, off, 64));
  if ((threadIdx.x & 63) == 0) shm[threadIdx.x >> 6] = m;
  acc[0] = 0.0;
  block_reduce_store<3>(acc, partial + 3 * (size_t)blockIdx.x);
  if (threadIdx.x == 0) {
    double mm = shm[0];
    for (int q = 1; q < kRedBlock / 64; ++q) mm = fmax(mm, shm[q]);
    partial[3 * (size_t)blockIdx.x] = mm;
  }
}

// k_cov_point_rank over the free points: a constant point is not tested, not counted as
// deficient and does not lower the reported minimum (its ratio slot reads +inf)
__global__ __launch_bounds__(256) void k_cov_point_rank_m(int NP, const double* __restrict__ V,
                                                          const double* __restrict__ sp, double thr,
                                                          double* __restrict__ ratio, double* __restrict__ partial,
                                                          const uint8_t* __restrict__ mask) {
  __shared__ double scnt[256], sneg[256];
  double cnt = 0.0, neg = INFINITY;
  const size_t NPs = (size_t)NP;
  for (int p = blockIdx.x * 256 + threadIdx.x; p < NP; p += gridDim.x * 256) {
    if (mask[p]) {
      ratio[p] = INFINITY;
      continue;
    }
    const double s0 = sp[p], s1 = sp[NPs + p], s2 = sp[2 * NPs + p];
    const double v00 = s0 * V[p] * s0, v01 = s0 * V[NPs + p] * s1, v02 = s0 * V[2 * NPs + p] * s2;
    const double v11 = s1 * V[3 * NPs + p] * s1, v12 = s1 * V[4 * NPs + p] * s2, v22 = s2 * V[5 * NPs + p] * s2;
    const double l00 = sqrt(v00);
    const double l10 = v01 / l00, l20 = v02 / l00;
    const double d1 = v11 - l10 * l10;
    const double l21 = (v12 - l20 * l10) / sqrt(d1);
    const double d2 = v22 - l20 * l20 - l21 * l21;
    const double mx = fmax(v00, fmax(d1, d2)), mn = fmin(v00, fmin(d1, d2));
    double q = mn / mx;
    if (!(v00 > 0.0) || isnan(q)) q = -INFINITY;
    ratio[p] = q;
    if (!(q > thr)) cnt += 1.0;
    neg = fmin(neg, q);
  }
  scnt[threadIdx.x] = cnt;
  sneg[threadIdx.x] = neg;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      scnt[threadIdx.x] += scnt[threadIdx.x + w];
      sneg[threadIdx.x] = fmin(sneg[threadIdx.x], sneg[threadIdx.x + w]);
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = scnt[0];
    partial[gridDim.x + blockIdx.x] = sneg[0];
  }
}

// The camera step without free points and without cross blocks: S = s U s + D^2 is block
// diagonal, so every free camera is a 6x6 system of its own. One lane per camera: the lower
// triangle (21 values), the factor and the two triangular solves stay in registers (every loop
// is unrolled, so the arrays are never indexed at run time). The blocks are few (C3: 999) and
// the launch is latency bound: 64-thread work-groups spread them over the compute units.
// D^2 is formed as k_s_diag forms it; the solve is L L^T y = s g_c as the dense factor's.
__global__ __launch_bounds__(64) void k_cam_block_solve(int NC, const double* __restrict__ ug,
                                                        const double* __restrict__ scc, StepScalars sc,
                                                        double* __restrict__ yc, int* __restrict__ fail) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= NC) return;
  const double* u = ug + 27 * (size_t)c;
  double s[6], b[6], L[6][6];
#pragma unroll
  for (int a = 0; a < 6; ++a) s[a] = scc[6 * (size_t)c + a];
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    b[a] = s[a] * u[21 + a];
#pragma unroll
    for (int k = 0; k <= a; ++k) {
      const int q = k * 6 - (k * (k - 1)) / 2 + (a - k);  // upper-packed index of (k, a)
      double h = s[a] * u[q] * s[k];
      if (a == k) {
        const double d = fmin(fmax(h, sc.min_diag), sc.max_diag);
        const double D = sqrt(d / sc.radius);
        h += D * D;
      }
      L[a][k] = h;
    }
  }
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double d = L[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
    ok = ok && d > 0.0 && isfinite(d);
    const double ljj = sqrt(d);
    L[j][j] = ljj;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double t = L[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) t -= L[i][k] * L[j][k];
      L[i][j] = t / ljj;
    }
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) {  // L z = b
    double t = b[i];
#pragma unroll
    for (int k = 0; k < i; ++k) t -= L[i][k] * b[k];
    b[i] = t / L[i][i];
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {  // L^T y = z
    double t = b[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) t -= L[k][i] * b[k];
    b[i] = t / L[i][i];
  }
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    ok = ok && isfinite(b[a]);
    yc[6 * (size_t)c + a] = b[a];
  }
  if (!ok) atomicOr(fail, 1);
}

void launch_point_factor_m(hipStream_t s, const DevView& v, const double* V, const double* g, const double* scale_p,
                           StepScalars sc, double* PU, double* q, int* fail, const uint8_t* mask) {
  if (!mask) return launch_point_factor(s, v, V, g, scale_p, sc, PU, q, fail);
  if (v.NP <= 0) return;
  k_point_factor_m<<<grid_for(v.NP, 256, 1 << 20), 256, 0, s>>>(v, V, g, scale_p, sc, PU, q, fail, mask);
}
void launch_scale_points_m(hipStream_t s, int NP, const double* V, double* scale_p, int on, const uint8_t* mask) {
  if (NP <= 0) return;
  k_scale_points_m<<<grid_for(3 * NP, 256, 1 << 20), 256, 0, s>>>(NP, V, scale_p, on, mask);
}
void launch_axpy_points_m(hipStream_t s, int NP, const double* x, const double* d, double* xc, double* partial,
                          int grid, const uint8_t* mask) {
  if (!mask) return launch_axpy_points(s, NP, x, d, xc, partial, grid);
  k_axpy_points_m<<<grid, 256, 0, s>>>(NP, x, d, xc, partial, mask);
}
void launch_grad_points_m(hipStream_t s, int NP, const double* x, const double* g, double* partial, int grid,
                          const uint8_t* mask) {
  if (!mask) return launch_grad_points(s, NP, x, g, partial, grid);
  k_grad_points_m<<<grid, 256, 0, s>>>(NP, x, g, partial, mask);
}
void launch_cov_point_rank_m(hipStream_t s, int NP, const double* V, const double* scale_p, double thr, double* ratio,
                             double* partial, int grid, const uint8_t* mask) {
  if (!mask) return launch_cov_point_rank(s, NP, V, scale_p, thr, ratio, partial, grid);
  k_cov_point_rank_m<<<grid, 256, 0, s>>>(NP, V, scale_p, thr, ratio, partial, mask);
}
void launch_cam_block_solve(hipStream_t s, int NC, const double* ug, const double* scale_c, StepScalars sc,
                            double* yc, int* fail) {
  if (NC <= 0) return;
  k_cam_block_solve<<<(NC + 63) / 64, 64, 0, s>>>(NC, ug, scale_c, sc, yc, fail);
}

DAB_WARM_TU(k_cam_block_solve);

}  // namespace dab
