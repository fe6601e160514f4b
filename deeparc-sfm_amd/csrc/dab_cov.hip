// dab_cov.hip — covariance at the solution (dab_covariance): the inverse of the reduced camera
// system from its Cholesky factor, and the per-point fold-back of the camera covariance.
//
// With L the row-major lower factor of the Jacobi-scaled, undamped S (dab_chol.hip: the blocks
// left of the diagonal in S's buffer, the factored diagonal blocks in the factorisation's
// scratch, chol_diag_blocks), the scaled camera covariance is C = S^-1 = L^-T L^-1 = Z^T Z with
// Z = L^-1:
//   k_cov_diag_inv   Z_ii = L_ii^-1 for every 64x64 diagonal block (one launch; the blocks
//                    are independent; scalar forward substitution, 64 columns side by side)
//   k_cov_trsm_row   block row i of Z below the diagonal: Z_ij = -Z_ii sum_{k=j}^{i-1} L_ik Z_kj
//                    (fp64 MFMA; one launch per block row, rows 1..nb-1 in stream order)
//   k_cov_ztz        the lower triangle of Z^T Z by 64x64 tiles, mirrored (fp64 MFMA; one
//                    launch). C may overwrite L: only Z is read.
// Nothing here waits on another work-group: every dependency is a launch boundary. Every sum
// runs in one fixed order, so two calls give bitwise the same arrays. Indices >= n (n < 64, a
// partial last block) read as zero and are never written.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "dab_handle.h"
#include "dab_kernels.h"
#include "dab_rows.h"
#include "dab_warm.h"

namespace dab {

namespace {
constexpr int CB = 64;    // block size of the blocked inverse
constexpr int CLS = 65;   // LDS row stride of the diagonal-block kernel
typedef double dbl4 __attribute__((ext_vector_type(4)));

// min / max / non-finite count of the factor's squared diagonal -> out[3] (one work-group).
// ACT: rows n_ext .. n - 1 are the six slots of the free intrinsics (act[i]: the active bits of
// free intrinsic i); the unit rows of inactive slots are left out.
template <bool ACT>
__device__ __forceinline__ void cov_diag_minmax(int n, int n_ext, const int* __restrict__ act,
                                                const double* __restrict__ Ld, double* __restrict__ out) {
  __shared__ double smin[256], smax[256], sbad[256];
  double mn = INFINITY, mx = 0.0, bad = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) {
    if constexpr (ACT) {
      if (i >= n_ext && !((act[(i - n_ext) / 6] >> ((i - n_ext) % 6)) & 1)) continue;
    }
    const double d = Ld[(size_t)kCholBlk * (i / CB) + kCholBlkL + (i % CB) * (CB + 1)];
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
__global__ __launch_bounds__(256) void k_cov_diag_minmax(int n, const double* __restrict__ Ld,
                                                         double* __restrict__ out) {
  cov_diag_minmax<false>(n, n, nullptr, Ld, out);
}
__global__ __launch_bounds__(256) void k_cov_diag_minmax_act(int n, int n_ext, const int* __restrict__ act,
                                                             const double* __restrict__ Ld,
                                                             double* __restrict__ out) {
  cov_diag_minmax<true>(n, n_ext, act, Ld, out);
}

// Z_ii = L_ii^-1. Thread c owns column c of the block: z_r = (delta_rc - sum_{c<=k<r} L_rk z_k)
// / L_rr. The strictly lower part of the LDS tile holds L, its upper part (diagonal included)
// the columns of Z transposed (thread c writes row c only), the reciprocal diagonal apart.
__global__ __launch_bounds__(CB) void k_cov_diag_inv(int n, const double* __restrict__ Ld,
                                                     double* __restrict__ Z, int ldz) {
  __shared__ double T[CB][CLS];
  __shared__ double dinv[CB];
  const int b0 = blockIdx.x * CB, c = threadIdx.x;
  const int nr = min(CB, n - b0);
  const double* L = Ld + (size_t)kCholBlk * blockIdx.x + kCholBlkL;  // L_bb [64][64]
  for (int r = 0; r < nr; ++r) {
    if (c < nr) T[r][c] = c < r ? L[r * CB + c] : 0.0;
  }
  if (c < nr) dinv[c] = 1.0 / L[c * CB + c];
  __syncthreads();
  if (c < nr) {
    T[c][c] = dinv[c];
    for (int r = c + 1; r < nr; ++r) {
      double acc = 0.0;
      for (int k = c; k < r; ++k) acc = fma(T[r][k], T[c][k], acc);  // L[r][k] * z_k
      T[c][r] = -acc * dinv[r];
    }
  }
  __syncthreads();
  // the whole tile goes out (zeros above the diagonal): the later passes read full tiles
  for (int r = 0; r < nr; ++r)
    if (c < nr) Z[(size_t)(b0 + r) * ldz + b0 + c] = c <= r ? T[c][r] : 0.0;
}

// Block row i of Z left of the diagonal. Work-group (j, strip): the 64 x 16 strip of Z_ij,
// wave w its rows 16 w .. 16 w + 15.
__global__ __launch_bounds__(256) void k_cov_trsm_row(int i, int n, const double* __restrict__ L, int lda,
                                                      double* __restrict__ Z, int ldz) {
  __shared__ double Ts[CB][17];
  const int j = blockIdx.x >> 2, strip = blockIdx.x & 3;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
  const int i0 = i * CB, c0 = j * CB + 16 * strip;
  const int arow = i0 + 16 * w + li;
  const bool arow_ok = arow < n;
  // T = sum_k L_ik Z_kj over the block columns j .. i-1 (all indices < i0 <= n there)
  dbl4 acc = {0.0, 0.0, 0.0, 0.0};
  const double* Lr = L + (size_t)(arow_ok ? arow : 0) * lda;
  for (int k0 = j * CB; k0 < i0; k0 += 16) {
    double a[4], b[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int k = k0 + 4 * ks + lk;
      a[ks] = arow_ok ? Lr[k] : 0.0;
      b[ks] = Z[(size_t)k * ldz + c0 + li];
    }
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[ks], b[ks], acc, 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) Ts[16 * w + lk + 4 * r][li] = acc[r];
  __syncthreads();
  // Z_ij = -Z_ii T
  dbl4 out = {0.0, 0.0, 0.0, 0.0};
  const double* Zr = Z + (size_t)(arow_ok ? arow : 0) * ldz;
#pragma unroll
  for (int ks = 0; ks < CB / 4; ++ks) {
    const int k = 4 * ks + lk;
    const double a = (arow_ok && i0 + k < n) ? -Zr[i0 + k] : 0.0;
    out = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Ts[k][li], out, 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = i0 + 16 * w + lk + 4 * r;
    if (row < n) Z[(size_t)row * ldz + c0 + li] = out[r];
  }
}

// C tile (i, j <= i) = sum_{k >= 64 i} Z[k][i-block]^T Z[k][j-block]; wave w: rows 16 w.. of the
// tile, all four 16-column tiles. The tile and its mirror are written (a diagonal tile from
// its lower half), so C is symmetric bitwise.
__global__ __launch_bounds__(256) void k_cov_ztz(int n, const double* __restrict__ Z, int ldz,
                                                 double* __restrict__ C, int ldc) {
  const int i = blockIdx.y, j = blockIdx.x;
  if (j > i) return;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
  const int i0 = i * CB, j0 = j * CB;
  const int acol = i0 + 16 * w + li;
  const bool acol_ok = acol < n;
  bool bcol_ok[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) bcol_ok[t] = j0 + 16 * t + li < n;
  dbl4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = dbl4{0.0, 0.0, 0.0, 0.0};
  for (int k0 = i0; k0 < n; k0 += 4) {
    const int k = k0 + lk;
    const bool kok = k < n;
    const double* Zk = Z + (size_t)(kok ? k : 0) * ldz;
    const double a = (kok && acol_ok) ? Zk[acol] : 0.0;
    double b[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) b[t] = (kok && bcol_ok[t]) ? Zk[j0 + 16 * t + li] : 0.0;
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b[t], acc[t], 0, 0, 0);
  }
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = i0 + 16 * w + lk + 4 * r, col = j0 + 16 * t + li;
      if (row >= n || col >= n || col > row) continue;
      C[(size_t)row * ldc + col] = acc[t][r];
      C[(size_t)col * ldc + row] = acc[t][r];
    }
}

// per point: pivot ratio of the scaled undamped V (the same arithmetic as k_point_factor with a
// zero LM diagonal) -> ratio[NP]; partial[grid] = deficient counts, partial[grid + b] = min ratio
__global__ __launch_bounds__(256) void k_cov_point_rank(int NP, const double* __restrict__ V,
                                                        const double* __restrict__ sp, double thr,
                                                        double* __restrict__ ratio, double* __restrict__ partial) {
  __shared__ double scnt[256], sneg[256];
  double cnt = 0.0, neg = INFINITY;  // neg: the smallest ratio
  const size_t NPs = (size_t)NP;
  for (int p = blockIdx.x * 256 + threadIdx.x; p < NP; p += gridDim.x * 256) {
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
    // fmin / fmax skip a NaN pivot (one that follows a negative one, which is then the minimum)
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

// One record per distinct free camera of a point ("the record" of the tile path): the sum of the
// Y of the point's entries with that camera, in entry order, at slot pt_ent_ptr[p] + i of
// Ym [NE][18] / mcam [NE]; mcnt[p] = the number of distinct cameras. Thread = point.
__global__ __launch_bounds__(256) void k_cov_merge(DevView v, const double* __restrict__ Y, double* __restrict__ Ym,
                                                   int* __restrict__ mcam, int* __restrict__ mcnt) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= v.NP) return;
  const int eb = v.pt_ent_ptr[p], ee = v.pt_ent_ptr[p + 1];
  int n = 0;
  for (int e = eb; e < ee; ++e) {
    const int ce = v.ent_cam[e];
    bool lead = true;  // the first entry of its camera
    for (int g = eb; g < e; ++g) lead = lead && v.ent_cam[g] != ce;
    if (!lead) continue;
    double y[18];
    const double2* ys = reinterpret_cast<const double2*>(Y + (size_t)kYRec * v.ent_pos[e]);
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const double2 t = ys[k];
      y[2 * k] = t.x;
      y[2 * k + 1] = t.y;
    }
    for (int g = e + 1; g < ee; ++g) {
      if (v.ent_cam[g] != ce) continue;
      const double2* gs = reinterpret_cast<const double2*>(Y + (size_t)kYRec * v.ent_pos[g]);
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        const double2 t = gs[k];
        y[2 * k] += t.x;
        y[2 * k + 1] += t.y;
      }
    }
    double2* dst = reinterpret_cast<double2*>(Ym + (size_t)kYRec * (eb + n));
#pragma unroll
    for (int k = 0; k < 9; ++k) dst[k] = make_double2(y[2 * k], y[2 * k + 1]);
    mcam[eb + n] = ce;
    ++n;
  }
  mcnt[p] = n;
}

// Sigma_pp = PU (I + sum_{e,e'} Y_e^T C_{c(e) c(e')} Y_e') PU^T, thread = point. With Z_c the sum
// of the Y of the point's entries of camera c (k_cov_merge) the sum over all ordered pairs of
// entries is the sum over ordered pairs of distinct cameras of Z_c^T C_cd Z_d, folded by C's
// symmetry: the pair (c, d before c) contributes G + G^T, the pair (c, c) G, so a point of k
// distinct cameras gathers k (k + 1) / 2 blocks, in record order (fixed). C: the scaled camera
// covariance, both triangles.
__global__ __launch_bounds__(256) void k_cov_points(DevView v, int with_cams, const double* __restrict__ PU,
                                                    const double* __restrict__ Ym, const int* __restrict__ mcam,
                                                    const int* __restrict__ mcnt, const double* __restrict__ C,
                                                    int ldc, double* __restrict__ out) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= v.NP) return;
  double m00 = 1.0, m01 = 0.0, m02 = 0.0, m11 = 1.0, m12 = 0.0, m22 = 1.0;
  if (with_cams) {
    const int eb = v.pt_ent_ptr[p], ee = eb + mcnt[p];
    for (int e = eb; e < ee; ++e) {
      double ye[18];
      const double2* ys = reinterpret_cast<const double2*>(Ym + (size_t)kYRec * e);
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        const double2 t = ys[k];
        ye[2 * k] = t.x;
        ye[2 * k + 1] = t.y;
      }
      const double* Crow = C + (size_t)6 * mcam[e] * ldc;
      for (int f = eb; f <= e; ++f) {
        double yf[18];
        const double2* fs = reinterpret_cast<const double2*>(Ym + (size_t)kYRec * f);
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          const double2 t = fs[k];
          yf[2 * k] = t.x;
          yf[2 * k + 1] = t.y;
        }
        const double* Cb = Crow + (size_t)6 * mcam[f];
        double g[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
#pragma unroll
        for (int a = 0; a < 6; ++a) {
          double t0 = 0.0, t1 = 0.0, t2 = 0.0;  // row a of C_ef Y_f
#pragma unroll
          for (int b = 0; b < 6; ++b) {
            const double cab = Cb[(size_t)a * ldc + b];
            t0 = fma(cab, yf[3 * b], t0);
            t1 = fma(cab, yf[3 * b + 1], t1);
            t2 = fma(cab, yf[3 * b + 2], t2);
          }
#pragma unroll
          for (int i = 0; i < 3; ++i) {
            g[i][0] = fma(ye[3 * a + i], t0, g[i][0]);
            g[i][1] = fma(ye[3 * a + i], t1, g[i][1]);
            g[i][2] = fma(ye[3 * a + i], t2, g[i][2]);
          }
        }
        if (f == e) {  // symmetric up to rounding: its symmetric part
          m00 += g[0][0];
          m11 += g[1][1];
          m22 += g[2][2];
          m01 += 0.5 * (g[0][1] + g[1][0]);
          m02 += 0.5 * (g[0][2] + g[2][0]);
          m12 += 0.5 * (g[1][2] + g[2][1]);
        } else {
          m00 += 2.0 * g[0][0];
          m11 += 2.0 * g[1][1];
          m22 += 2.0 * g[2][2];
          m01 += g[0][1] + g[1][0];
          m02 += g[0][2] + g[2][0];
          m12 += g[1][2] + g[2][1];
        }
      }
    }
  }
  const double* pu = PU + 6 * (size_t)p;
  const double u00 = pu[0], u01 = pu[1], u02 = pu[2], u11 = pu[3], u12 = pu[4], u22 = pu[5];
  // W = PU M (PU upper triangular), Sigma = W PU^T
  const double w00 = u00 * m00 + u01 * m01 + u02 * m02, w01 = u00 * m01 + u01 * m11 + u02 * m12,
               w02 = u00 * m02 + u01 * m12 + u02 * m22;
  const double w11 = u11 * m11 + u12 * m12, w12 = u11 * m12 + u12 * m22;
  const double w10 = u11 * m01 + u12 * m02;
  const double w22 = u22 * m22, w21 = u22 * m12, w20 = u22 * m02;
  (void)w10; (void)w20; (void)w21;
  double* o = out + 6 * (size_t)p;
  o[0] = w00 * u00 + w01 * u01 + w02 * u02;
  o[1] = w01 * u11 + w02 * u12;
  o[2] = w02 * u22;
  o[3] = w11 * u11 + w12 * u12;
  o[4] = w12 * u22;
  o[5] = w22 * u22;
}

// Sigma_cc' = s_c C s_c' in place (the product of the two scales first: symmetric bitwise)
__global__ __launch_bounds__(256) void k_cov_unscale(int n, const double* __restrict__ sc, double* __restrict__ C,
                                                     int ldc) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (size_t)n * n) return;
  const size_t i = t / n, j = t - i * n;
  C[i * ldc + j] *= sc[i] * sc[j];
}
// The same over the bordered system of n = n_ext + 6 nfi rows, s = (s_c, s_z); the rows and
// columns of inactive intrinsic slots (s_z = 0: known exactly) are written as +0
__global__ __launch_bounds__(256) void k_cov_unscale_z(int n, int n_ext, const double* __restrict__ sc,
                                                       const double* __restrict__ sz, const int* __restrict__ act,
                                                       double* __restrict__ C, int ldc) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= (size_t)n * n) return;
  const int i = (int)(t / n), j = (int)(t - (size_t)i * n);
  const bool zi = i >= n_ext, zj = j >= n_ext;
  const bool off = (zi && !((act[(i - n_ext) / 6] >> ((i - n_ext) % 6)) & 1)) ||
                   (zj && !((act[(j - n_ext) / 6] >> ((j - n_ext) % 6)) & 1));
  const double si = zi ? sz[i - n_ext] : sc[i], sj = zj ? sz[j - n_ext] : sc[j];
  double* c = C + (size_t)i * ldc + j;
  *c = off ? 0.0 : *c * (si * sj);
}
// the 6x6 diagonal blocks, upper-packed -> out[NC][21]
__global__ __launch_bounds__(256) void k_cov_ext_blocks(int NC, const double* __restrict__ C, int ldc,
                                                        double* __restrict__ out) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= 21 * NC) return;
  const int c = t / 21, q = t - 21 * c;
  int a = 0, rem = q;
  while (rem >= 6 - a) {
    rem -= 6 - a;
    ++a;
  }
  const int b = a + rem;
  out[t] = C[(size_t)(6 * c + a) * ldc + 6 * c + b];
}
}  // namespace

// dab_covariance_intrinsics: the records of a point's fold-back with free intrinsics. Thread =
// point. Its merged camera records (k_cov_merge: slots pt_ent_ptr[p] .. of Ym / mcam, mcnt[p] of
// them; none when with_cams is 0) move to slot rbase[p] of rec / rcam, and behind them goes one
// record per distinct free intrinsic i the point sees, Gz_p,i = sum_{o of p with intrinsic i}
// (s_z ∘ J_z,o)^T J_p,o PU_p (6x3, laid out as a Y record, "camera" NC + i), in first-seen
// order of the point's SELL slots, each summed in slot order. rbase[p + 1] - rbase[p] = the
// point's entries + the free intrinsics it sees (ptmask), so the records of a point never
// reach the next one's. rcnt[p] = the record count.
template <int LOSS>
__global__ __launch_bounds__(256) void k_cov_gz(DevView v, const double* __restrict__ points,
                                                const double* __restrict__ camtab, const double* __restrict__ PU,
                                                const double* __restrict__ sz, const int2* __restrict__ meta,
                                                int with_cams, const int* __restrict__ rbase,
                                                const double* __restrict__ Ym, const int* __restrict__ mcam,
                                                const int* __restrict__ mcnt, double* __restrict__ rec,
                                                int* __restrict__ rcam, int* __restrict__ rcnt) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= v.NP) return;
  const GlobalTabs tb{camtab, v.intr};
  const LossK lk = loss_of(v);
  const int base = rbase[p];
  int n = 0;
  if (with_cams) {
    const int eb = v.pt_ent_ptr[p];
    n = mcnt[p];
    for (int i = 0; i < n; ++i) {
      const double2* src = reinterpret_cast<const double2*>(Ym + (size_t)kYRec * (eb + i));
      double2* dst = reinterpret_cast<double2*>(rec + (size_t)kYRec * (base + i));
#pragma unroll
      for (int k = 0; k < 9; ++k) dst[k] = src[k];
      rcam[base + i] = mcam[eb + i];
    }
  }
  const int sl = p >> 6, lane = p & 63;
  const int off = v.slice_off[sl], len = (v.slice_off[sl + 1] - off) >> 6;
  const double X[3] = {points[3 * (size_t)p], points[3 * (size_t)p + 1], points[3 * (size_t)p + 2]};
  const double* pu = PU + 6 * (size_t)p;  // upper-packed 00 01 02 11 12 22
  const double u00 = pu[0], u01 = pu[1], u02 = pu[2], u11 = pu[3], u12 = pu[4], u22 = pu[5];
  int done = 0;
  for (int k0 = 0; k0 < len; ++k0) {
    const int4 lead = v.obs_idx[off + 64 * k0 + lane];
    if (lead.x < 0) continue;  // padding slot
    const int zi = meta[lead.w].x;
    if (zi < 0 || ((done >> zi) & 1)) continue;
    done |= 1 << zi;
    double g[18];
#pragma unroll
    for (int t = 0; t < 18; ++t) g[t] = 0.0;
    for (int k = k0; k < len; ++k) {
      const int s = off + 64 * k + lane;
      const int4 id = v.obs_idx[s];
      if (id.x < 0) continue;
      const int2 mt = meta[id.w];
      if (mt.x != zi) continue;
      const double2 xy = v.obs_xy[s];
      double ru, rv, jx0[3], jx1[3], rho;
      obs_rows_l<LOSS, true, -1>(lk, rho, id, xy, X, tb, ru, rv, jx0, jx1, nullptr, nullptr);
      double P[3], Kr[6], z0[6], z1[6];
      obs_cam_point(id, X, tb, P);
      tb.k(id.w, Kr);
      intr_rows<LOSS>(P, Kr, xy.x, xy.y, lk, mt.y & 63, ((mt.y >> 16) & 1) != 0, z0, z1);
      // a_o = J_p PU_p, rows 0 and 1
      const double a0 = jx0[0] * u00, a1 = jx0[0] * u01 + jx0[1] * u11, a2 = jx0[0] * u02 + jx0[1] * u12 + jx0[2] * u22;
      const double b0 = jx1[0] * u00, b1 = jx1[0] * u01 + jx1[1] * u11, b2 = jx1[0] * u02 + jx1[1] * u12 + jx1[2] * u22;
#pragma unroll
      for (int a = 0; a < 6; ++a) {
        const double s0 = sz[6 * zi + a] * z0[a], s1 = sz[6 * zi + a] * z1[a];
        g[3 * a] += s0 * a0 + s1 * b0;
        g[3 * a + 1] += s0 * a1 + s1 * b1;
        g[3 * a + 2] += s0 * a2 + s1 * b2;
      }
    }
    double2* dst = reinterpret_cast<double2*>(rec + (size_t)kYRec * (base + n));
#pragma unroll
    for (int k = 0; k < 9; ++k) dst[k] = make_double2(g[2 * k], g[2 * k + 1]);
    rcam[base + n] = v.NC + zi;
    ++n;
  }
  rcnt[p] = n;
}
void launch_cov_gz(hipStream_t s, const DevView& v, const double* points, const double* camtab, const double* PU,
                   const double* sz, const int2* meta, bool with_cams, const int* rbase, const double* Ym,
                   const int* mcam, const int* mcnt, double* rec, int* rcam, int* rcnt) {
  if (v.NP <= 0) return;
  DAB_LOSS_SWITCH(v.loss, k_cov_gz<LOSS><<<grid_for(v.NP, 256, 1 << 20), 256, 0, s>>>(
                              v, points, camtab, PU, sz, meta, with_cams ? 1 : 0, rbase, Ym, mcam, mcnt, rec, rcam, rcnt));
}

void launch_cov_diag_minmax(hipStream_t s, int n, const double* Ld, double* out) {
  k_cov_diag_minmax<<<1, 256, 0, s>>>(n, Ld, out);
}

void launch_cov_inverse(hipStream_t s, int n, const double* L, int lda, const double* Ld, double* Z, int ldz,
                        double* C, int ldc) {
  if (n <= 0) return;
  const int nb = (n + CB - 1) / CB;
  k_cov_diag_inv<<<nb, CB, 0, s>>>(n, Ld, Z, ldz);
  for (int i = 1; i < nb; ++i) k_cov_trsm_row<<<4 * i, 256, 0, s>>>(i, n, L, lda, Z, ldz);
  k_cov_ztz<<<dim3(nb, nb), 256, 0, s>>>(n, Z, ldz, C, ldc);
}

void launch_cov_diag_minmax_act(hipStream_t s, int n, int n_ext, const int* act, const double* Ld, double* out) {
  k_cov_diag_minmax_act<<<1, 256, 0, s>>>(n, n_ext, act, Ld, out);
}

int cov_rank_grid(int NP) { return std::max(1, std::min(256, (NP + 255) / 256)); }
void launch_cov_point_rank(hipStream_t s, int NP, const double* V, const double* scale_p, double thr, double* ratio,
                           double* partial, int grid) {
  k_cov_point_rank<<<grid, 256, 0, s>>>(NP, V, scale_p, thr, ratio, partial);
}

void launch_cov_points(hipStream_t s, const DevView& v, bool with_cams, const double* PU, const double* Y,
                       double* Ym, int* mcam, int* mcnt, const double* C, int ldc, double* out) {
  if (v.NP <= 0) return;
  const int g = (v.NP + 255) / 256;
  if (with_cams) k_cov_merge<<<g, 256, 0, s>>>(v, Y, Ym, mcam, mcnt);
  k_cov_points<<<g, 256, 0, s>>>(v, with_cams ? 1 : 0, PU, Ym, mcam, mcnt, C, ldc, out);
}

void launch_cov_points_z(hipStream_t s, const DevView& v, bool with_cams, const double* points,
                         const double* camtab, const double* PU, const double* sz, const int2* meta,
                         const double* Y, double* Ym, int* mcam, int* mcnt, const int* rbase, double* rec, int* rcam,
                         int* rcnt, const double* C, int ldc, double* out) {
  if (v.NP <= 0) return;
  const int g = (v.NP + 255) / 256;
  if (with_cams) k_cov_merge<<<g, 256, 0, s>>>(v, Y, Ym, mcam, mcnt);
  launch_cov_gz(s, v, points, camtab, PU, sz, meta, with_cams, rbase, Ym, mcam, mcnt, rec, rcam, rcnt);
  // k_cov_points reads of the view only NP and where each point's records begin
  DevView vr = v;
  vr.pt_ent_ptr = rbase;
  k_cov_points<<<g, 256, 0, s>>>(vr, 1, PU, rec, rcam, rcnt, C, ldc, out);
}

void launch_cov_unscale_z(hipStream_t s, int NC, int nfi, const double* scale_c, const double* sz, const int* act,
                          double* C, int ldc, double* blocks) {
  const size_t n = (size_t)6 * (NC + nfi);
  if (n == 0) return;
  k_cov_unscale_z<<<(unsigned)((n * n + 255) / 256), 256, 0, s>>>((int)n, 6 * NC, scale_c, sz, act, C, ldc);
  if (blocks) k_cov_ext_blocks<<<(21 * (NC + nfi) + 255) / 256, 256, 0, s>>>(NC + nfi, C, ldc, blocks);
}

void launch_cov_unscale(hipStream_t s, int NC, const double* scale_c, double* C, int ldc, double* ext_cov) {
  if (NC <= 0) return;
  const size_t n = (size_t)6 * NC;
  k_cov_unscale<<<(unsigned)((n * n + 255) / 256), 256, 0, s>>>((int)n, scale_c, C, ldc);
  if (ext_cov) k_cov_ext_blocks<<<(21 * NC + 255) / 256, 256, 0, s>>>(NC, C, ldc, ext_cov);
}

DAB_WARM_TU(k_cov_diag_minmax);

}  // namespace dab

using namespace dab;

// ------------------------------------------------------------------------------------
// dab_covariance: Sigma = (J^T J)^-1 at the current parameters, by the exact Schur route
// ------------------------------------------------------------------------------------
// In the solver's scaled variables (s = the Jacobi scaling dab_solve would use here), with
// PU_p = s_p L_p^-T, Y_e = (s_c ∘ Jc^T Jp) PU_p and C = (scaled S)^-1:
//   Sigma_cc' = s_c C_cc' s_c',  Sigma_pp = PU_p (I + sum_{e,e'} Y_e^T C_c(e)c(e') Y_e') PU_p^T.
// The LM kernels run unchanged with radius = +inf: their sqrt(clamp(d) / radius) is exactly 0.
//
// with_intr (dab_covariance_intrinsics): the free intrinsics of the handle's mask join the camera
// system as in the exact step, S' of n' = 6 NC + 6 nfi rows in the handle's z buffer with the
// border rows of one undamped LM step; C' = S'^-1, s = (s_c, s_z), and a point's fold-back gains
// one record Gz_p,i per free intrinsic it sees (k_cov_gz). With nfi = 0 every launch and buffer
// is dab_covariance's. ext_full: [n'][n'] then, intr_cov [nfi][21].
//
// xb (dab_covariance_blocks): cross blocks for the request's pairs, folded from the same C and the
// same record store by the kernels of dab_k_covx.hip, after the point blocks and before the
// unscale. With xb null or empty every launch and buffer is as without it.
namespace {
struct CovBlocks {
  const dab_cov_blocks_request* req = nullptr;
  double *pp = nullptr, *pe = nullptr, *pz = nullptr;
  double* ms = nullptr;
  bool any() const { return req && (req->num_pp > 0 || req->num_pe > 0 || req->num_pz > 0); }
};
// how each pair is answered
enum : uint8_t { kXDev = 0, kXDevT = 1, kXZero = 2, kXNan = 3 };
struct CovxPlan {
  std::vector<int2> pairs;   // [pp | pe | pz] device pairs; x < 0: answered on the host
  std::vector<uint8_t> how;  // [pp | pe | pz]
  std::vector<double> out;   // [pp 9 | pe 18 | pz 18 each] as the device left them
};
// where the fold-back's records are (launch_cov_points / launch_cov_points_z)
struct CovRecs {
  bool with_recs = false;
  const int *rbase = nullptr, *rcnt = nullptr, *rcam = nullptr;
  const double* rec = nullptr;
  const double* C = nullptr;
  int ldc = 0;
};
}  // namespace

// the request's lists and indices, before anything on the handle changes
static int cov_blocks_check(const dab_handle* h, const CovBlocks& xb) {
  const dab_cov_blocks_request& r = *xb.req;
  if (r.num_pp < 0 || r.num_pe < 0 || r.num_pz < 0) return set_error(DAB_E_INVALID, "negative pair count");
  if ((r.num_pp > 0 && (!r.pp || !xb.pp)) || (r.num_pe > 0 && (!r.pe || !xb.pe)) ||
      (r.num_pz > 0 && (!r.pz || !xb.pz)))
    return set_error(DAB_E_INVALID, "a pair list with a null index or output array");
  const int npts = h->prob.num_points, E = h->E, NI = h->NI;
  for (int i = 0; i < 2 * r.num_pp; ++i)
    if (r.pp[i] < 0 || r.pp[i] >= npts) return set_error(DAB_E_INVALID, "pp: point index out of range");
  for (int i = 0; i < r.num_pe; ++i) {
    if (r.pe[2 * i] < 0 || r.pe[2 * i] >= npts) return set_error(DAB_E_INVALID, "pe: point index out of range");
    if (r.pe[2 * i + 1] < 0 || r.pe[2 * i + 1] >= E)
      return set_error(DAB_E_INVALID, "pe: extrinsic index out of range");
  }
  for (int i = 0; i < r.num_pz; ++i) {
    if (r.pz[2 * i] < 0 || r.pz[2 * i] >= npts) return set_error(DAB_E_INVALID, "pz: point index out of range");
    if (r.pz[2 * i + 1] < 0 || r.pz[2 * i + 1] >= NI)
      return set_error(DAB_E_INVALID, "pz: intrinsic index out of range");
  }
  return 0;
}

// Translate the pairs (caller's ids -> device points and column blocks), upload them once and
// launch the two kernels between cov_ev_x[0] and [1]; the blocks come back into plan.out on the
// stream (the caller synchronises). A pair with a point this rank does not reference, or with a
// free extrinsic nothing references, carries no information (NaN); else one with a constant
// point, a constant extrinsic or an intrinsic outside the free set is known exactly (+0).
static int cov_blocks_run(dab_handle* h, const CovBlocks& xb, int nfi, const CovRecs& rc, CovxPlan* plan) {
  const dab_cov_blocks_request& r = *xb.req;
  const int NP = h->NP, NC = h->NC;
  hipStream_t s = h->stream;
  const size_t npp = (size_t)r.num_pp, npe = (size_t)r.num_pe, npz = (size_t)r.num_pz, nall = npp + npe + npz;
  std::vector<int> dev_of((size_t)std::max(1, h->prob.num_points), -1);
  for (int i = 0; i < NP; ++i) dev_of[(size_t)h->pt_of[(size_t)i]] = i;
  const bool any_const = h->d_ptc != nullptr && !h->pt_const.empty();
  auto is_const = [&](int id) { return any_const && h->pt_const[(size_t)id] != 0; };
  plan->pairs.assign(nall, make_int2(-1, -1));
  plan->how.assign(nall, kXNan);
  for (size_t i = 0; i < npp; ++i) {
    const int a = r.pp[2 * i], b = r.pp[2 * i + 1];
    const int da = dev_of[(size_t)a], db = dev_of[(size_t)b];
    if (da < 0 || db < 0) continue;
    if (is_const(a) || is_const(b)) {
      plan->how[i] = kXZero;
      continue;
    }
    plan->pairs[i] = make_int2(std::min(da, db), std::max(da, db));
    plan->how[i] = da <= db ? kXDev : kXDevT;
  }
  for (size_t i = 0; i < npe; ++i) {
    const int a = r.pe[2 * i], e = r.pe[2 * i + 1];
    const int da = dev_of[(size_t)a], c = h->ext_col[(size_t)e];
    if (da < 0 || (c < 0 && !h->ext_fixed[(size_t)e])) continue;
    if (c < 0 || is_const(a) || !rc.with_recs) {
      plan->how[npp + i] = kXZero;
      continue;
    }
    plan->pairs[npp + i] = make_int2(da, c);
    plan->how[npp + i] = kXDev;
  }
  for (size_t i = 0; i < npz; ++i) {
    const int a = r.pz[2 * i], z = r.pz[2 * i + 1];
    const int da = dev_of[(size_t)a];
    if (da < 0) continue;
    const int zi = nfi > 0 ? h->intr_meta[(size_t)z].x : -1;
    if (zi < 0 || is_const(a) || !rc.with_recs) {
      plan->how[npp + npe + i] = kXZero;
      continue;
    }
    plan->pairs[npp + npe + i] = make_int2(da, NC + zi);
    plan->how[npp + npe + i] = kXDev;
  }
  const size_t nout = 9 * npp + 18 * (npe + npz);
  if (nall > h->lz.covx_pairs_cap) {
    h->dev.drop(h->lz.d_covx_pairs);
    h->lz.d_covx_pairs = nullptr;
    h->lz.covx_pairs_cap = 0;
    CHECK_RC(h->dev.alloc(&h->lz.d_covx_pairs, nall));
    h->lz.covx_pairs_cap = nall;
  }
  if (nout > h->lz.covx_out_cap) {
    h->dev.drop(h->lz.d_covx_out);
    h->lz.d_covx_out = nullptr;
    h->lz.covx_out_cap = 0;
    CHECK_RC(h->dev.alloc(&h->lz.d_covx_out, nout));
    h->lz.covx_out_cap = nout;
  }
  int2* const d_pairs = h->lz.d_covx_pairs;
  double* const d_out = h->lz.d_covx_out;
  HIP_OK(hipMemcpyAsync(d_pairs, plan->pairs.data(), sizeof(int2) * nall, hipMemcpyHostToDevice, s));
  HIP_OK(hipEventRecord(h->cov_ev_x[0], s));
  launch_covx_pp(s, (int)npp, d_pairs, rc.with_recs, rc.rbase, rc.rcnt, rc.rec, rc.rcam, h->d_L, rc.C, rc.ldc, d_out);
  if (rc.with_recs) {
    launch_covx_pc(s, (int)npe, d_pairs + npp, rc.rbase, rc.rcnt, rc.rec, rc.rcam, h->d_L, rc.C, rc.ldc, NC,
                   h->d_scale_c, h->lz.d_sz, d_out + 9 * npp);
    launch_covx_pc(s, (int)npz, d_pairs + npp + npe, rc.rbase, rc.rcnt, rc.rec, rc.rcam, h->d_L, rc.C, rc.ldc, NC,
                   h->d_scale_c, h->lz.d_sz, d_out + 9 * npp + 18 * npe);
  }
  HIP_OK(hipEventRecord(h->cov_ev_x[1], s));
  plan->out.resize(nout);
  HIP_OK(hipMemcpyAsync(plan->out.data(), d_out, sizeof(double) * nout, hipMemcpyDeviceToHost, s));
  return 0;
}

// the caller's arrays from the plan, after the last check that can fail
static void cov_blocks_write(const CovBlocks& xb, const CovxPlan& plan) {
  const dab_cov_blocks_request& r = *xb.req;
  const size_t npp = (size_t)r.num_pp, npe = (size_t)r.num_pe, npz = (size_t)r.num_pz;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (size_t i = 0; i < npp; ++i) {
    double* o = xb.pp + 9 * i;
    const double* d = plan.out.data() + 9 * i;
    const uint8_t how = plan.how[i];
    for (int a = 0; a < 3; ++a)
      for (int b = 0; b < 3; ++b)
        o[3 * a + b] = how == kXDev ? d[3 * a + b] : how == kXDevT ? d[3 * b + a] : how == kXZero ? 0.0 : nan;
  }
  auto rect = [&](size_t n, size_t first, const double* d, double* o) {
    for (size_t i = 0; i < n; ++i) {
      const uint8_t how = plan.how[first + i];
      if (how == kXDev) std::memcpy(o + 18 * i, d + 18 * i, 18 * sizeof(double));
      else std::fill(o + 18 * i, o + 18 * i + 18, how == kXZero ? 0.0 : nan);
    }
  };
  rect(npe, npp, plan.out.data() + 9 * npp, xb.pe);
  rect(npz, npp + npe, plan.out.data() + 9 * npp + 18 * npe, xb.pz);
}

static int covariance_impl(dab_handle* h, const dab_covariance_options* opt_in, double* point_cov, double* ext_cov,
                           double* intr_cov, double* ext_full, dab_covariance_info* info,
                           dab_covariance_intr_info* zinfo, bool with_intr, const CovBlocks* xb = nullptr) {
  if (!with_intr && h && h->have_problem && intr_mask_any(h)) {
    // free intrinsics are not part of the covariance: it would report them as exactly known
    int nfi_cov = 0;
    HIP_OK(hipSetDevice(h->device));
    CHECK_RC(intr_free_set(h, true, &nfi_cov));
    if (nfi_cov > 0)
      return set_error(DAB_E_UNSUPPORTED,
                       "dab_covariance with free intrinsics is not supported (dab_covariance_intrinsics is)");
  }
  clear_error();
  if (!h) return set_error(DAB_E_INVALID, "null handle");
  dab_covariance_options opt;
  if (opt_in) opt = *opt_in;
  else dab_covariance_options_init(&opt);
  if (!(std::isfinite(opt.min_pivot_ratio) && opt.min_pivot_ratio > 0.0))
    return set_error(DAB_E_INVALID, "min_pivot_ratio must be finite and > 0");
  const bool want_x = xb && xb->any();
  if (!info && !point_cov && !ext_cov && !intr_cov && !ext_full && !want_x)
    return set_error(DAB_E_INVALID, "null info and null arrays");
  if (!h->have_problem) return set_error(DAB_E_STATE, "no problem set");
  if (want_x) CHECK_RC(cov_blocks_check(h, *xb));
  HIP_OK(hipSetDevice(h->device));
  // free intrinsics: dab_solve's rule and refusals, before anything on the handle changes
  CamSystem cs;
  if (with_intr) CHECK_RC(cam_system_free_set(h, nullptr, &cs));
  // constant points: PU = 0 and q = 0 take them out of S and of the fold-back (their rows of
  // point_cov come out exactly 0), and the rank test leaves them out
  CHECK_RC(pt_const_sync(h));
  // constant scalars of an extrinsic: the Jacobi scale 0 empties their rows and columns of S, a
  // unit diagonal keeps the factor, the rank test leaves them out and the outputs get exact zeros
  CHECK_RC(ext_sub_sync(h));
  CHECK_RC(prior_sync(h));  // extrinsic priors: eval_jacobian_and_blocks folds them into U | g_c
  CHECK_RC(pt_prior_sync(h));  // point priors: ... into V | g, so the point factor and the rank test see them
  CHECK_RC(call_state(h, nullptr));  // whether any rank has one (several ranks: one small max-reduce)
  CHECK_RC(zprior_sync(h, cs.nfi));  // intrinsic priors: into U_zz | g_z after intr_eval (plain dab_covariance: none)
  const int nfree_pts = h->NP - h->n_pt_const;
  hipStream_t s = h->stream;
  const DevView& v = h->view;
  const int NP = h->NP, NC = h->NC;
  if (NC > 0) CHECK_RC(build_schur_tables(h));
  CHECK_RC(cam_system_buffers(h, true, &cs));
  const int nfi = cs.nfi, n = cs.n, n2 = cs.n2, ld_ = cs.ld;
  double* const S_ = cs.S;
  dab_covariance_intr_info zout{};
  zout.num_free_intr = nfi;
  zout.num_free_scalars = cs.nz_scal;
  dab_covariance_info out{};
  out.status = DAB_COV_OK;
  out.num_free_ext = NC;
  out.num_free_points = nfree_pts;
  out.first_deficient_point = -1;
  out.schur_assembly = h->schur_tiles ? DAB_SCHUR_TILES : DAB_SCHUR_PAIRS;
  out.num_residuals = 2 * h->N + 6 * h->n_prior + 3 * h->n_pt_prior + 6 * h->n_zprior;
  out.num_parameters = 3 * nfree_pts + 6 * NC - h->n_ext_sub + cs.nz_scal;
  out.point_pivot_ratio_min = out.camera_pivot_ratio = std::numeric_limits<double>::quiet_NaN();
  for (hipEvent_t& e : h->cov_ev)
    if (!e) HIP_OK(hipEventCreate(&e));
  if (nfi > 0)
    for (hipEvent_t& e : h->cov_ev_z)
      if (!e) HIP_OK(hipEventCreate(&e));
  if (want_x)
    for (hipEvent_t& e : h->cov_ev_x)
      if (!e) HIP_OK(hipEventCreate(&e));
  const int rgrid = cov_rank_grid(NP);
  if (!h->lz.d_cov_stat) CHECK_RC(h->dev.alloc(&h->lz.d_cov_stat, (size_t)8 + 2 * (size_t)rgrid));
  double* d_stat = h->lz.d_cov_stat;         // [0] deficient points, [4..6] diagonal min / max / bad
  double* d_rpart = h->lz.d_cov_stat + 8;    // the rank kernel's work-group partials

  // ---- undamped linearisation at the current parameters ----
  HIP_OK(hipMemsetAsync(h->d_scal + S_XERR, 0, sizeof(double), s));
  HIP_OK(hipEventRecord(h->cov_ev[0], s));
  CHECK_RC(eval_jacobian_and_blocks(h, false));
  if (nfi > 0) {
    CHECK_RC(intr_eval(h));
    zprior_blocks(h);  // before the Jacobi scale and the border rows read zg
  }
  launch_jacobi_scale(h, nfi, opt.jacobi_scaling);
  HIP_OK(hipEventRecord(h->cov_ev[1], s));
  CHECK_RC(read_scalars(h));
  if (h->h_scal[S_COST_BAD] != 0.0 || !std::isfinite(pt_prior_cost(h)) || !std::isfinite(zprior_cost(h)))
    return set_error(DAB_E_INVALID, "residuals are not finite at the current parameters");
  // x_cost bounds the tile assembly's fixed-point rhs: the observations' cost and the point
  // priors' (all ranks), which both enter q_p; the extrinsic priors' never does
  const double x_obs = 0.5 * h->h_scal[S_COST];
  const double x_cost = h->pt_prior_any ? x_obs + pt_prior_cost(h) : x_obs;
  out.cost = h->n_prior > 0 ? x_obs + prior_cost(h) : x_obs;
  if (h->pt_prior_any) out.cost += pt_prior_cost(h);
  if (h->n_zprior > 0) out.cost += zprior_cost(h);

  // ---- point factor without LM diagonal, and the point-side rank test ----
  dab_options lm;
  dab_options_init(&lm);
  const StepScalars sc{std::numeric_limits<double>::infinity(), lm.min_lm_diagonal, lm.max_lm_diagonal};
  HIP_OK(hipMemsetAsync(h->d_flags, 0, sizeof(int) * 4, s));
  launch_point_factor_m(s, v, h->d_V, h->d_g, h->d_scale_p, sc, h->d_L, h->d_q, h->d_flags, h->d_ptc);
  double* d_ratio = h->d_dp;  // [NP] of the step buffer (scratch between LM steps)
  launch_cov_point_rank_m(s, NP, h->d_V, h->d_scale_p, opt.min_pivot_ratio, d_ratio, d_rpart, rgrid, h->d_ptc);
  launch_final_sum(s, rgrid, 1, d_rpart, d_stat);
  CHECK_RC(h->allreduce(d_stat, 1, ncclMax));  // every rank takes the same exit
  double hstat[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  std::vector<double> hmin((size_t)rgrid);
  HIP_OK(hipMemcpyAsync(hstat, d_stat, sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(hmin.data(), d_rpart + rgrid, sizeof(double) * (size_t)rgrid, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  CHECK_RC(p2p_check(h->p2p_main));
  if (nfree_pts > 0) out.point_pivot_ratio_min = *std::min_element(hmin.begin(), hmin.end());
  auto finish = [&](hipEvent_t last) -> int {
    float ms = 0.f;
    HIP_OK(hipEventSynchronize(last));
    HIP_OK(hipEventElapsedTime(&ms, h->cov_ev[0], h->cov_ev[1]));
    out.evaluate_ms = ms;
    if (last != h->cov_ev[1]) {
      HIP_OK(hipEventElapsedTime(&ms, h->cov_ev[1], h->cov_ev[2]));
      out.factor_ms = ms;
    }
    if (last == h->cov_ev[4]) {
      HIP_OK(hipEventElapsedTime(&ms, h->cov_ev[2], h->cov_ev[3]));
      out.inverse_ms = ms;
      HIP_OK(hipEventElapsedTime(&ms, h->cov_ev[3], h->cov_ev[4]));
      out.points_ms = ms;
    }
    if (nfi > 0 && last != h->cov_ev[1]) {
      HIP_OK(hipEventElapsedTime(&ms, h->cov_ev_z[0], h->cov_ev_z[1]));
      zout.border_ms = ms;
    }
    if (info) *info = out;
    if (zinfo) *zinfo = zout;
    return 0;
  };
  if (hstat[0] > 0.0) {
    out.status = DAB_COV_RANK_DEFICIENT;
    out.deficient_points = (int)hstat[0];
    std::vector<double> ratio((size_t)NP);
    if (NP > 0) HIP_OK(hipMemcpy(ratio.data(), d_ratio, sizeof(double) * (size_t)NP, hipMemcpyDeviceToHost));
    int first = -1;
    for (int i = 0; i < NP; ++i)
      if (!(ratio[i] > opt.min_pivot_ratio) && (first < 0 || h->pt_of[i] < first)) first = h->pt_of[i];
    out.first_deficient_point = first;
    return finish(h->cov_ev[1]);
  }

  // ---- S and its factor (the exact step's assembly) ----
  if (NC > 0) {
    CHECK_RC(cam_system_assemble(h, cs, sc, x_cost, false));
    if (h->schur_tiles) {
      // the point kernel reads per-entry records: the tile path keeps per-(point, camera) sums only
      if (!h->lz.d_Yrec) CHECK_RC(h->dev.alloc(&h->lz.d_Yrec, (size_t)kYRec * std::max(1, h->NE)));
      if (point_cov || want_x)
        launch_entry_y(s, v, h->d_points, h->d_camtab, h->d_scale_c, h->d_L, YBufs{h->d_Y, h->d_Yp, false}, false,
                       h->lz.d_Yrec);
    }
    if (nfi > 0) {
      HIP_OK(hipEventRecord(h->cov_ev_z[0], s));
      CHECK_RC(intr_border_rows(h, nfi, sc, S_, ld_));
      HIP_OK(hipEventRecord(h->cov_ev_z[1], s));
    }
    launch_ext_unit_diag(s, NC, h->d_exs, S_, ld_);
    if (chol_factor_solve(h->chol, s, n2, S_, ld_, cs.yc, h->d_flags + 1) != 0)
      return set_error(DAB_E_DEVICE, "dense Cholesky launch failed");
    if (h->d_exs)
      launch_cov_diag_minmax_x(s, n2, n, nfi > 0 ? h->lz.d_intr_act : nullptr, h->d_exs, chol_diag_blocks(h->chol),
                               d_stat + 4);
    else if (nfi > 0) launch_cov_diag_minmax_act(s, n2, n, h->lz.d_intr_act, chol_diag_blocks(h->chol), d_stat + 4);
    else launch_cov_diag_minmax(s, n, chol_diag_blocks(h->chol), d_stat + 4);
  }
  HIP_OK(hipEventRecord(h->cov_ev[2], s));
  HIP_OK(hipMemcpyAsync(hstat + 4, d_stat + 4, sizeof(double) * 3, hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(h->h_flags, h->d_flags, sizeof(int) * 4, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  CHECK_RC(p2p_check(h->p2p_main));
  if (h->h_flags[0] != 0) return set_error(DAB_E_DEVICE, "point factor failed after the rank test passed");
  if (NC > 0) {
    if (h->h_flags[1] & 2)
      return set_error(DAB_E_DEVICE, "dense Cholesky: a bounded wait between work-groups timed out");
    const bool flagged = h->h_flags[1] != 0 || hstat[6] != 0.0;
    out.camera_pivot_ratio = flagged ? 0.0 : hstat[4] / hstat[5];
    if (!(out.camera_pivot_ratio > opt.min_pivot_ratio)) {
      out.status = DAB_COV_RANK_DEFICIENT;
      return finish(h->cov_ev[2]);
    }
  }
  if (!point_cov && !ext_cov && !intr_cov && !ext_full && !want_x) return finish(h->cov_ev[2]);  // the size / rank query

  // ---- C = S^-1 from the factor, the point blocks, the unscaled camera part ----
  const bool want_c = NC > 0 && (point_cov || ext_cov || intr_cov || ext_full || want_x);
  if (want_c && nfi > 0) {
    // the second n' x n' buffer (n' changes with the free set: kept while it fits)
    const size_t need = (size_t)n2 * ld_;
    if (need > h->lz.covZz_cap) {
      h->dev.drop(h->lz.d_covZz);
      h->lz.d_covZz = nullptr;
      h->lz.covZz_cap = 0;
      CHECK_RC(h->dev.alloc(&h->lz.d_covZz, need));
      h->lz.covZz_cap = need;
    }
    launch_cov_inverse(s, n2, S_, ld_, chol_diag_blocks(h->chol), h->lz.d_covZz, ld_, S_, ld_);
  } else if (want_c) {
    if (!h->lz.d_covZ) CHECK_RC(h->dev.alloc(&h->lz.d_covZ, (size_t)n * h->lds));
    launch_cov_inverse(s, n, h->d_S, h->lds, chol_diag_blocks(h->chol), h->lz.d_covZ, h->lds, h->d_S, h->lds);
  }
  HIP_OK(hipEventRecord(h->cov_ev[3], s));
  CovRecs xr;  // the cross blocks read the record store the point blocks leave
  if (point_cov || want_x) {
    if (!h->lz.d_cov_pts) CHECK_RC(h->dev.alloc(&h->lz.d_cov_pts, (size_t)6 * std::max(1, NP)));
    if (!h->lz.d_cov_idx) CHECK_RC(h->dev.alloc(&h->lz.d_cov_idx, (size_t)std::max(1, h->NE) + (size_t)std::max(1, NP)));
    if (nfi > 0) {
      // where each point's records begin: its entries, then the free intrinsics it sees
      std::vector<int> ptmask((size_t)std::max(1, NP)), ent_ptr((size_t)NP + 1), rbase((size_t)NP + 1);
      HIP_OK(hipMemcpyAsync(ptmask.data(), h->lz.d_ptmask, sizeof(int) * (size_t)NP, hipMemcpyDeviceToHost, s));
      HIP_OK(hipMemcpyAsync(ent_ptr.data(), h->d_pt_ent_ptr, sizeof(int) * ((size_t)NP + 1), hipMemcpyDeviceToHost, s));
      HIP_OK(hipStreamSynchronize(s));
      long long nz_rec = 0;
      for (int p = 0; p < NP; ++p) {
        rbase[(size_t)p] = (int)(ent_ptr[(size_t)p] + nz_rec);
        nz_rec += __builtin_popcount((unsigned)ptmask[(size_t)p]);
      }
      const long long total = (long long)ent_ptr[(size_t)NP] + nz_rec;
      if (total > INT_MAX) return set_error(DAB_E_UNSUPPORTED, "too many fold-back records for 32-bit indices");
      rbase[(size_t)NP] = (int)total;
      const size_t cap = (size_t)std::max<long long>(1, total);
      if (cap > h->lz.cov_rec_cap) {
        h->dev.drop(h->lz.d_cov_rec);
        h->dev.drop(h->lz.d_cov_ridx);
        h->lz.d_cov_rec = nullptr;
        h->lz.d_cov_ridx = nullptr;
        h->lz.cov_rec_cap = 0;
        CHECK_RC(h->dev.alloc(&h->lz.d_cov_rec, (size_t)kYRec * cap));
        CHECK_RC(h->dev.alloc(&h->lz.d_cov_ridx, cap + 2 * (size_t)NP + 1));
        h->lz.cov_rec_cap = cap;
      }
      int* const rcam = h->lz.d_cov_ridx;
      int* const rcnt = rcam + h->lz.cov_rec_cap;
      int* const d_rbase = rcnt + NP;
      HIP_OK(hipMemcpyAsync(d_rbase, rbase.data(), sizeof(int) * ((size_t)NP + 1), hipMemcpyHostToDevice, s));
      launch_cov_points_z(s, v, h->NE > 0, h->d_points, h->d_camtab, h->d_L, h->lz.d_sz, h->lz.d_intr_meta, h->lz.d_Yrec, h->d_Y,
                          h->lz.d_cov_idx, h->lz.d_cov_idx + std::max(1, h->NE), d_rbase, h->lz.d_cov_rec, rcam, rcnt, S_, ld_,
                          h->lz.d_cov_pts);
      HIP_OK(hipStreamSynchronize(s));  // rbase's host copy goes out of scope
      xr = CovRecs{true, d_rbase, rcnt, rcam, h->lz.d_cov_rec, S_, ld_};
    } else {
      // d_Y (the step's camera-major Y planes, unused on this route) takes the merged records
      launch_cov_points(s, v, NC > 0 && h->NE > 0, h->d_L, h->lz.d_Yrec, h->d_Y, h->lz.d_cov_idx,
                        h->lz.d_cov_idx + std::max(1, h->NE), h->d_S, h->lds, h->lz.d_cov_pts);
      xr = CovRecs{NC > 0 && h->NE > 0, h->d_pt_ent_ptr, h->lz.d_cov_idx + std::max(1, h->NE), h->lz.d_cov_idx, h->d_Y,
                   h->d_S, h->lds};
    }
  }
  HIP_OK(hipEventRecord(h->cov_ev[4], s));
  CovxPlan xplan;
  if (want_x) CHECK_RC(cov_blocks_run(h, *xb, nfi, xr, &xplan));
  double* d_ext21 = nullptr;
  if (want_c && (ext_cov || intr_cov || ext_full)) {
    if (ext_cov || intr_cov) {
      if (!h->lz.d_cov_ext) CHECK_RC(h->dev.alloc(&h->lz.d_cov_ext, (size_t)21 * (NC + kIntrFreeMax)));
      d_ext21 = h->lz.d_cov_ext;
    }
    if (nfi > 0) launch_cov_unscale_z(s, NC, nfi, h->d_scale_c, h->lz.d_sz, h->lz.d_intr_act, S_, ld_, d_ext21);
    else launch_cov_unscale(s, NC, h->d_scale_c, h->d_S, h->lds, d_ext21);
    launch_cov_zero_x(s, n2, n, h->d_exs, S_, ld_, d_ext21);
  }
  std::vector<double> hp;
  if (point_cov && NP > 0) {
    hp.resize((size_t)6 * NP);
    HIP_OK(hipMemcpyAsync(hp.data(), h->lz.d_cov_pts, hp.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  }
  HIP_OK(hipStreamSynchronize(s));
  // every array is written from here on, after the last check that can fail
  if (want_x) {
    float xms = 0.f;
    HIP_OK(hipEventElapsedTime(&xms, h->cov_ev_x[0], h->cov_ev_x[1]));
    if (xb->ms) *xb->ms = xms;
    cov_blocks_write(*xb, xplan);
  }
  if (point_cov) {
    const size_t npts = (size_t)h->prob.num_points;
    std::fill(point_cov, point_cov + 6 * npts, std::numeric_limits<double>::quiet_NaN());
    for (int i = 0; i < NP; ++i)
      std::memcpy(point_cov + 6 * (size_t)h->pt_of[i], hp.data() + 6 * (size_t)i, 6 * sizeof(double));
  }
  if (ext_cov && NC > 0)
    HIP_OK(hipMemcpy(ext_cov, d_ext21, sizeof(double) * 21 * (size_t)NC, hipMemcpyDeviceToHost));
  if (intr_cov && nfi > 0)
    HIP_OK(hipMemcpy(intr_cov, d_ext21 + 21 * (size_t)NC, sizeof(double) * 21 * (size_t)nfi, hipMemcpyDeviceToHost));
  if (ext_full && NC > 0)
    HIP_OK(hipMemcpy2D(ext_full, (size_t)n2 * sizeof(double), S_, (size_t)ld_ * sizeof(double),
                       (size_t)n2 * sizeof(double), (size_t)n2, hipMemcpyDeviceToHost));
  return finish(h->cov_ev[4]);
}
extern "C" int dab_covariance(dab_handle* h, const dab_covariance_options* opt, double* point_cov, double* ext_cov,
                              double* ext_full, dab_covariance_info* info) {
  const int rc = covariance_impl(h, opt, point_cov, ext_cov, nullptr, ext_full, info, nullptr, false);
  if (h) CHECK_RC(guard_fail(h, "dab_covariance"));
  return rc;
}
extern "C" int dab_covariance_intrinsics(dab_handle* h, const dab_covariance_options* opt, double* point_cov,
                                         double* ext_cov, double* intr_cov, double* cam_full,
                                         dab_covariance_info* info, dab_covariance_intr_info* zinfo) {
  const int rc = covariance_impl(h, opt, point_cov, ext_cov, intr_cov, cam_full, info, zinfo, true);
  if (h) CHECK_RC(guard_fail(h, "dab_covariance_intrinsics"));
  return rc;
}
extern "C" int dab_covariance_blocks(dab_handle* h, const dab_covariance_options* opt,
                                     const dab_cov_blocks_request* req, double* pp_cov, double* pe_cov,
                                     double* pz_cov, dab_covariance_info* info, dab_covariance_intr_info* zinfo,
                                     double* blocks_ms) {
  if (blocks_ms) *blocks_ms = 0.0;
  const CovBlocks xb{req, pp_cov, pe_cov, pz_cov, blocks_ms};
  const int rc = covariance_impl(h, opt, nullptr, nullptr, nullptr, nullptr, info, zinfo, true, &xb);
  if (h) CHECK_RC(guard_fail(h, "dab_covariance_blocks"));
  return rc;
}
