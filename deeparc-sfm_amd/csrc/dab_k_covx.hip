// dab_k_covx.hip — cross blocks of the covariance (dab_covariance_blocks): the fold-back of the
// scaled camera covariance C = S^-1 (C' with the block z of free intrinsics) for a caller-given
// list of pairs, where k_cov_points (dab_cov.hip) folds the pair (p, p) of every point only.
//
// A point p has records r = 0 .. rcnt[p] - 1 at slot rbase[p] + r of rec [.][18] / rcam: one per
// distinct free camera (k_cov_merge) and, behind them, one per free intrinsic the point sees
// ("camera" NC + i, k_cov_gz), Z_r 6x3 row-major, in that fixed order. With PU_p = s_p L_p^-T
// (upper triangular, packed 00 01 02 11 12 22) and Sigma = -V^-1 W^T C on the point-camera part:
//   Sigma_pp' = PU_p (delta_pp' I + sum_{r in p} sum_{r' in p'} Z_r^T C_c(r)c(r') Z_r') PU_p'^T
//   Sigma_pc  = -PU_p (sum_{r in p} Z_r^T C_c(r)c) diag(s_c)     c: a camera or NC + i, s = (s_c, s_z)
// C is read before k_cov_unscale(_z) touches it, so the column scale is explicit here. A column
// of scale 0 (a constant scalar of an extrinsic, an inactive intrinsic slot) is known exactly and
// comes out +0. Thread = pair; every block is summed by its one owner in record order, so two
// calls give bitwise the same arrays. ld of C is a multiple of 8 and a block column starts at a
// multiple of 6 doubles, so a row segment of a 6x6 block is three aligned double2.
#include <hip/hip_runtime.h>

#include "dab_kernels.h"
#include "dab_warm.h"

namespace dab {

namespace {
__device__ __forceinline__ void covx_load_rec(const double* __restrict__ rec, int slot, double y[18]) {
  const double2* ys = reinterpret_cast<const double2*>(rec + (size_t)kYRec * slot);
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    const double2 t = ys[k];
    y[2 * k] = t.x;
    y[2 * k + 1] = t.y;
  }
}
// the 6x6 block (rows of camera cr, columns of camera cc) of C
__device__ __forceinline__ void covx_load_block(const double* __restrict__ C, int ldc, int cr, int cc,
                                                double c[6][6]) {
  const double* Cb = C + (size_t)6 * cr * ldc + (size_t)6 * cc;
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    const double2* row = reinterpret_cast<const double2*>(Cb + (size_t)a * ldc);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double2 t = row[k];
      c[a][2 * k] = t.x;
      c[a][2 * k + 1] = t.y;
    }
  }
}
}  // namespace

// Point-camera blocks. pairs[i] = (device point, column block: a camera column or NC + free
// intrinsic column); x < 0: the host answers that pair (exact zeros, NaN) and nothing is written.
// out[i][18]: 3x6 row-major. with_recs = 0: no record exists (no launch then: the host answers).
__global__ __launch_bounds__(64) void k_covx_pc(int npairs, const int2* __restrict__ pairs,
                                                const int* __restrict__ rbase, const int* __restrict__ rcnt,
                                                const double* __restrict__ rec, const int* __restrict__ rcam,
                                                const double* __restrict__ PU, const double* __restrict__ C, int ldc,
                                                int NC, const double* __restrict__ sc, const double* __restrict__ sz,
                                                double* __restrict__ out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= npairs) return;
  const int2 pr = pairs[i];
  if (pr.x < 0) return;
  const int p = pr.x, cb = pr.y;
  double acc[3][6];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 6; ++b) acc[a][b] = 0.0;
  const int base = rbase[p], n = rcnt[p];
  for (int r = 0; r < n; ++r) {
    double y[18], c[6][6];
    covx_load_rec(rec, base + r, y);
    covx_load_block(C, ldc, rcam[base + r], cb, c);
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int b = 0; b < 6; ++b) acc[k][b] = fma(y[3 * a + k], c[a][b], acc[k][b]);
  }
  const double* pu = PU + 6 * (size_t)p;
  const double u00 = pu[0], u01 = pu[1], u02 = pu[2], u11 = pu[3], u12 = pu[4], u22 = pu[5];
  const double* s = cb < NC ? sc + 6 * (size_t)cb : sz + 6 * (size_t)(cb - NC);
  double* o = out + 18 * (size_t)i;
#pragma unroll
  for (int b = 0; b < 6; ++b) {
    const double sb = s[b];
    const double w0 = u00 * acc[0][b] + u01 * acc[1][b] + u02 * acc[2][b];
    const double w1 = u11 * acc[1][b] + u12 * acc[2][b];
    const double w2 = u22 * acc[2][b];
    // -(w s) + 0: a zero product is written as +0
    o[b] = sb == 0.0 ? 0.0 : -(w0 * sb) + 0.0;
    o[6 + b] = sb == 0.0 ? 0.0 : -(w1 * sb) + 0.0;
    o[12 + b] = sb == 0.0 ? 0.0 : -(w2 * sb) + 0.0;
  }
}

// Point-point blocks. pairs[i] = (p, p') device points with p <= p' (the host puts every pair in
// that order and transposes on output, so (a, b) and (b, a) are one computation); x < 0: the host
// answers. out[i][9]: 3x3 row-major, rows p, columns p'; a block (p, p) is symmetric bitwise.
// with_recs = 0 (no camera system): Sigma_pp' = delta_pp' PU_p PU_p^T.
__global__ __launch_bounds__(64) void k_covx_pp(int npairs, const int2* __restrict__ pairs, int with_recs,
                                                const int* __restrict__ rbase, const int* __restrict__ rcnt,
                                                const double* __restrict__ rec, const int* __restrict__ rcam,
                                                const double* __restrict__ PU, const double* __restrict__ C, int ldc,
                                                double* __restrict__ out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= npairs) return;
  const int2 pr = pairs[i];
  if (pr.x < 0) return;
  const int p = pr.x, q = pr.y;
  double m[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) m[a][b] = (a == b && p == q) ? 1.0 : 0.0;
  if (with_recs) {
    const int pb = rbase[p], pn = rcnt[p], qb = rbase[q], qn = rcnt[q];
    for (int r = 0; r < pn; ++r) {
      double ye[18];
      covx_load_rec(rec, pb + r, ye);
      const int cr = rcam[pb + r];
      for (int f = 0; f < qn; ++f) {
        double yf[18], c[6][6];
        covx_load_rec(rec, qb + f, yf);
        covx_load_block(C, ldc, cr, rcam[qb + f], c);
#pragma unroll
        for (int a = 0; a < 6; ++a) {
          double t0 = 0.0, t1 = 0.0, t2 = 0.0;  // row a of C_rf Z_f
#pragma unroll
          for (int b = 0; b < 6; ++b) {
            t0 = fma(c[a][b], yf[3 * b], t0);
            t1 = fma(c[a][b], yf[3 * b + 1], t1);
            t2 = fma(c[a][b], yf[3 * b + 2], t2);
          }
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            m[k][0] = fma(ye[3 * a + k], t0, m[k][0]);
            m[k][1] = fma(ye[3 * a + k], t1, m[k][1]);
            m[k][2] = fma(ye[3 * a + k], t2, m[k][2]);
          }
        }
      }
    }
  }
  if (p == q) {  // a diagonal block: the symmetric part of the sum, and below the upper triangle mirrored
    m[0][1] = m[1][0] = 0.5 * (m[0][1] + m[1][0]);
    m[0][2] = m[2][0] = 0.5 * (m[0][2] + m[2][0]);
    m[1][2] = m[2][1] = 0.5 * (m[1][2] + m[2][1]);
  }
  const double* pu = PU + 6 * (size_t)p;
  const double* qu = PU + 6 * (size_t)q;
  const double u00 = pu[0], u01 = pu[1], u02 = pu[2], u11 = pu[3], u12 = pu[4], u22 = pu[5];
  const double v00 = qu[0], v01 = qu[1], v02 = qu[2], v11 = qu[3], v12 = qu[4], v22 = qu[5];
  double* o = out + 9 * (size_t)i;
  // W = PU_p M (row k), Sigma = W PU_p'^T
  double w[3][3];
#pragma unroll
  for (int b = 0; b < 3; ++b) {
    w[0][b] = u00 * m[0][b] + u01 * m[1][b] + u02 * m[2][b];
    w[1][b] = u11 * m[1][b] + u12 * m[2][b];
    w[2][b] = u22 * m[2][b];
  }
  double r[3][3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    r[a][0] = w[a][0] * v00 + w[a][1] * v01 + w[a][2] * v02;
    r[a][1] = w[a][1] * v11 + w[a][2] * v12;
    r[a][2] = w[a][2] * v22;
  }
  if (p == q) {
    r[1][0] = r[0][1];
    r[2][0] = r[0][2];
    r[2][1] = r[1][2];
  }
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) o[3 * a + b] = r[a][b];
}

void launch_covx_pc(hipStream_t s, int npairs, const int2* pairs, const int* rbase, const int* rcnt,
                    const double* rec, const int* rcam, const double* PU, const double* C, int ldc, int NC,
                    const double* sc, const double* sz, double* out) {
  if (npairs <= 0) return;
  k_covx_pc<<<(npairs + 63) / 64, 64, 0, s>>>(npairs, pairs, rbase, rcnt, rec, rcam, PU, C, ldc, NC, sc, sz, out);
}
void launch_covx_pp(hipStream_t s, int npairs, const int2* pairs, bool with_recs, const int* rbase, const int* rcnt,
                    const double* rec, const int* rcam, const double* PU, const double* C, int ldc, double* out) {
  if (npairs <= 0) return;
  k_covx_pp<<<(npairs + 63) / 64, 64, 0, s>>>(npairs, pairs, with_recs ? 1 : 0, rbase, rcnt, rec, rcam, PU, C, ldc,
                                             out);
}

DAB_WARM_TU(k_covx_pc);

}  // namespace dab
