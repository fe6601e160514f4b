// dab_k_extsub.hip — constant scalars of an extrinsic (dab_set_ext_scalars_constant): the masked
// forms of the small camera-side kernels of the LM step and of the covariance. bits[NC], one byte
// per camera column, bit k = scalar k of that camera's (w0,w1,w2,t0,t1,t2) is constant. The
// unmasked kernels (dab_solver.hip, dab_kernels.hip, dab_k_step.hip, dab_k_ptconst.hip,
// dab_cov.hip) are untouched and run whenever the effective set is empty; a free scalar goes
// through the same arithmetic here as there, operation for operation.
//
// The route: a constant scalar gets the Jacobi scale 0, with jacobi_scaling off as well. Every
// consumer of a camera column multiplies by that scale, so the scalar's row and column of S, its
// rhs and its Y rows are exactly 0 in both assemblies, in the direct step and in every PCG
// product. What is left is here: the scale itself, the norms over the free scalars, the candidate
// that copies a constant scalar bit for bit, a unit diagonal where a factor or a preconditioner
// would otherwise see min_lm_diagonal / radius (or, undamped, a zero), and the covariance's rank
// test and exact zeros.
#include <hip/hip_runtime.h>

#include "dab_kernels.h"
#include "dab_reduce.h"
#include "dab_warm.h"
#include "dab_wave.h"

namespace dab {

// k_scale_cams; a constant scalar has no Jacobi scale of its own: 0 takes its column out
__global__ void k_scale_cams_x(int NC, const double* __restrict__ ug, double* __restrict__ sc, int on,
                               const uint8_t* __restrict__ bits) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 6 * NC) return;
  const int c = i / 6, a = i - 6 * c;
  const int q = a * 6 - (a * (a - 1)) / 2;  // (a,a) in the packed upper layout
  const double s = on ? 1.0 / (1.0 + sqrt(ug[27 * (size_t)c + q])) : 1.0;
  sc[i] = ((bits[c] >> a) & 1) ? 0.0 : s;
}

// k_cam_norms over the free scalars: a constant one adds nothing to the step norm, to either
// parameter norm or to the gradient's max and sum
__global__ __launch_bounds__(1024) void k_cam_norms_x(int E, const int* __restrict__ ext_col,
                                                      const double* __restrict__ ext,
                                                      const double* __restrict__ ext_c,
                                                      const double* __restrict__ ug, double* __restrict__ out,
                                                      const uint8_t* __restrict__ bits) {
  constexpr int U = 8;  // elements per thread per round (6 E <= 8192 in one round)
  double a[5] = {0, 0, 0, 0, 0};
  const int n = 6 * E;
  for (int t0 = 0; t0 < n; t0 += U * 1024) {
    int c[U];
    double x[U], xc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int t = t0 + u * 1024 + (int)threadIdx.x;
      c[u] = t < n ? ext_col[t / 6] : -1;
      x[u] = t < n ? ext[t] : 0.0;
      xc[u] = (t < n && ext_c) ? ext_c[t] : x[u];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (c[u] < 0) continue;
      const int k = (t0 + u * 1024 + (int)threadIdx.x) % 6;
      if ((bits[c[u]] >> k) & 1) continue;
      const double dd = x[u] - xc[u];
      a[0] += dd * dd;
      a[1] += xc[u] * xc[u];
      const double gg = ug ? x[u] - (x[u] + (-ug[27 * (size_t)c[u] + 21 + k])) : 0.0;
      a[2] = fmax(a[2], fabs(gg));
      a[3] += gg * gg;
      a[4] += x[u] * x[u];
    }
  }
  __shared__ double sh[16][5];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    double v = a[i];
    if (i == 2) {
      for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
      if (lane == 63) sh[w][i] = v;
    } else {
      v = wave_sum_lane63(v);
      if (lane == 63) sh[w][i] = v;
    }
  }
  __syncthreads();
  if (threadIdx.x < 5) {
    double t = sh[0][threadIdx.x];
    for (int q = 1; q < 16; ++q) t = threadIdx.x == 2 ? fmax(t, sh[q][threadIdx.x]) : t + sh[q][threadIdx.x];
    out[threadIdx.x] = t;
  }
}

// k_cam_candidate; a constant scalar's candidate is its x, bit for bit (x + (-0 * 0) would turn a
// -0.0 into +0.0), and its delta is +0 for the candidate pass and the priors' model term
__global__ void k_cam_candidate_x(int E, const int* __restrict__ ext_col, const double* __restrict__ ext,
                                  const double* __restrict__ yc, const double* __restrict__ scc,
                                  double* __restrict__ ext_c, double* __restrict__ dc,
                                  const uint8_t* __restrict__ bits) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 6 * E) return;
  const int e = t / 6, k = t - 6 * (t / 6);
  const int c = ext_col[e];
  if (c >= 0 && yc) {
    if ((bits[c] >> k) & 1) {
      ext_c[t] = ext[t];
      dc[6 * c + k] = 0.0;
      return;
    }
    const double d = -yc[6 * c + k] * scc[6 * c + k];
    ext_c[t] = ext[t] + d;
    dc[6 * c + k] = d;
  } else {
    ext_c[t] = ext[t];
  }
}

// The unit diagonal of the constant scalars. Scalar t = 6 c + k sits at A[t * step + k * inner]:
// the dense S (step = ld + 1, inner = 0) or an array of 6x6 row-major blocks (step = 6,
// inner = 1). Its row and column are exact zeros already; B (nullable) is a second array of the
// same shape.
__global__ void k_ext_unit_diag(int NC, const uint8_t* __restrict__ bits, double* __restrict__ A,
                                double* __restrict__ B, size_t step, int inner) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 6 * NC) return;
  const int c = t / 6, k = t - 6 * c;
  if (!((bits[c] >> k) & 1)) return;
  const size_t at = (size_t)t * step + (size_t)(k * inner);
  A[at] = 1.0;
  if (B) B[at] = 1.0;
}

// k_cam_block_solve with constant scalars: their rows of the 6x6 block are unit rows (the scale 0
// has emptied them), so the factor never sees min_lm_diagonal / radius there, and y = 0
__global__ __launch_bounds__(64) void k_cam_block_solve_x(int NC, const double* __restrict__ ug,
                                                          const double* __restrict__ scc, StepScalars sc,
                                                          double* __restrict__ yc, int* __restrict__ fail,
                                                          const uint8_t* __restrict__ bits) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= NC) return;
  const double* u = ug + 27 * (size_t)c;
  const int bc = bits[c];
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
        if ((bc >> a) & 1) h = 1.0;
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

// k_cov_diag_minmax(_act) without the unit rows of the constant scalars (rows < n_ext) and, with
// act, without those of inactive intrinsic slots: min / max / non-finite count of the factor's
// squared diagonal -> out[3] (one work-group)
__global__ __launch_bounds__(256) void k_cov_diag_minmax_x(int n, int n_ext, const int* __restrict__ act,
                                                           const uint8_t* __restrict__ bits,
                                                           const double* __restrict__ Ld, double* __restrict__ out) {
  __shared__ double smin[256], smax[256], sbad[256];
  double mn = INFINITY, mx = 0.0, bad = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) {
    if (i < n_ext) {
      if ((bits[i / 6] >> (i % 6)) & 1) continue;
    } else if (act && !((act[(i - n_ext) / 6] >> ((i - n_ext) % 6)) & 1)) {
      continue;
    }
    const double d = Ld[(size_t)kCholBlk * (i / 64) + kCholBlkL + (i % 64) * 65];
    const double d2 = d * d;
    if (!isfinite(d2) || !(d > 0.0)) {
      bad += 1.0;
    } else {
      mn = fmin(mn, d2);
      mx = fmax(mx, d2);
    }
  }
  smin[threadIdx.x] = mn;
  smax[threadIdx.x] = mx;
  sbad[threadIdx.x] = bad;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
      smin[threadIdx.x] = fmin(smin[threadIdx.x], smin[threadIdx.x + w]);
      smax[threadIdx.x] = fmax(smax[threadIdx.x], smax[threadIdx.x + w]);
      sbad[threadIdx.x] += sbad[threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    out[0] = smin[0];
    out[1] = smax[0];
    out[2] = sbad[0];
  }
}

// The covariance's rows and columns of the constant scalars as +0 (known exactly), in the unscaled
// n x n matrix C (its first n_ext rows are the cameras') and in the upper-packed 6x6 diagonal
// blocks taken from it (nullable)
__global__ __launch_bounds__(256) void k_cov_zero_x(int n, int n_ext, const uint8_t* __restrict__ bits,
                                                    double* __restrict__ C, int ldc, double* __restrict__ blocks) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (size_t)n * n) return;
  const int i = (int)(t / n), j = (int)(t - (size_t)i * n);
  const bool ci = i < n_ext && ((bits[i / 6] >> (i % 6)) & 1);
  const bool cj = j < n_ext && ((bits[j / 6] >> (j % 6)) & 1);
  if (!ci && !cj) return;
  C[(size_t)i * ldc + j] = 0.0;
  if (blocks && i / 6 == j / 6 && j >= i) {
    const int a = i % 6, b = j % 6;
    blocks[21 * (size_t)(i / 6) + a * 6 - (a * (a - 1)) / 2 + (b - a)] = 0.0;
  }
}

void launch_scale_cams_x(hipStream_t s, int NC, const double* ug, double* scale_c, int on, const uint8_t* bits) {
  if (NC <= 0) return;
  k_scale_cams_x<<<grid_for(6 * NC, 256, 1 << 20), 256, 0, s>>>(NC, ug, scale_c, on, bits);
}
void launch_cam_norms_x(hipStream_t s, int E, const int* ext_col, const double* ext, const double* ext_c,
                        const double* ug, double* out, const uint8_t* bits) {
  if (!bits) return launch_cam_norms(s, E, ext_col, ext, ext_c, ug, out);
  k_cam_norms_x<<<1, 1024, 0, s>>>(E, ext_col, ext, ext_c, ug, out, bits);
}
void launch_cam_candidate_x(hipStream_t s, int E, const int* ext_col, const double* ext, const double* yc,
                            const double* scale_c, double* ext_c, double* delta_c, const uint8_t* bits) {
  if (!bits) return launch_cam_candidate(s, E, ext_col, ext, yc, scale_c, ext_c, delta_c);
  if (E <= 0) return;
  k_cam_candidate_x<<<grid_for(6 * E, 256, 1 << 20), 256, 0, s>>>(E, ext_col, ext, yc, scale_c, ext_c, delta_c, bits);
}
void launch_ext_unit_diag(hipStream_t s, int NC, const uint8_t* bits, double* S, int ld) {
  if (!bits || NC <= 0) return;
  k_ext_unit_diag<<<grid_for(6 * NC, 256, 1 << 20), 256, 0, s>>>(NC, bits, S, nullptr, (size_t)ld + 1, 0);
}
void launch_ext_unit_blocks(hipStream_t s, int NC, const uint8_t* bits, double* Ad, double* Minv) {
  if (!bits || NC <= 0) return;
  k_ext_unit_diag<<<grid_for(6 * NC, 256, 1 << 20), 256, 0, s>>>(NC, bits, Ad, Minv, 6, 1);
}
void launch_cam_block_solve_x(hipStream_t s, int NC, const double* ug, const double* scale_c, StepScalars sc,
                              double* yc, int* fail, const uint8_t* bits) {
  if (!bits) return launch_cam_block_solve(s, NC, ug, scale_c, sc, yc, fail);
  if (NC <= 0) return;
  k_cam_block_solve_x<<<(NC + 63) / 64, 64, 0, s>>>(NC, ug, scale_c, sc, yc, fail, bits);
}
void launch_cov_diag_minmax_x(hipStream_t s, int n, int n_ext, const int* act, const uint8_t* bits, const double* Ld,
                              double* out) {
  k_cov_diag_minmax_x<<<1, 256, 0, s>>>(n, n_ext, act, bits, Ld, out);
}
void launch_cov_zero_x(hipStream_t s, int n, int n_ext, const uint8_t* bits, double* C, int ldc, double* blocks) {
  if (!bits || n <= 0) return;
  k_cov_zero_x<<<(unsigned)(((size_t)n * n + 255) / 256), 256, 0, s>>>(n, n_ext, bits, C, ldc, blocks);
}

DAB_WARM_TU(k_ext_unit_diag);

}  // namespace dab
