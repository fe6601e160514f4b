// dab_rows.h — row arithmetic of the gfx950 kernels of the BA hot path:
// projection, loss, per-extrinsic tables and the residual / Jacobian rows of one observation,
// shared by the kernel files (dab_kernels.hip, dab_k_*.hip, dab_cov.hip). Device code only.
//
// Data layout in HBM (all wave64, coalesced on the dominant streams):
//   point-major observation streams ("s" order, observations of one point contiguous)
//     obs_idx int4 (point, ext0, ext1, intr) 16 B, obs_xy double2 16 B
//   camera-major entry inputs (one per observation slot whose extrinsic is free, static):
//     cm_idx int4 16 B, cm_xy double2 16 B
//     Y[pos][18]   = Schur factor of the entry, per LM iteration       144 B
//   per-point V[6][NP], g[3][NP], PU[NP][6], q[NP][4]; per-camera ug[NC][27].
// Matrix-free: the Jacobian is never stored. Each pass re-evaluates the rows it needs
// from the 32-B inputs (point side in point-major order, camera side from the
// camera-major copy) and reduces them on chip: V, g by a deterministic segmented wave
// scan, U, g_c by fixed-shape chunk reductions. Per observation that moves ~32 B instead
// of writing and re-reading a 144-240 B Jacobian.
// Per-extrinsic rotation data is precomputed once per parameter state (k_cam_tables):
// d(R(w)X)/dw = -R [X]x J_r(w) (right Jacobian of SO(3)); in Ceres' first-order branch
// (|w|^2 <= DBL_EPSILON, rotation.h) R = I + [w]x and the derivative is -[X]x, encoded as
// Rd = I, Jd = I. No transcendental runs per observation.
// Every reduction has a fixed shape and order: results are bitwise reproducible.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>

#include "dab_kernels.h"

namespace dab {

// ------------------------------------------------------------------------------------
// per-extrinsic tables (R, t, Rd, Jd)
// ------------------------------------------------------------------------------------
// Rodrigues' coefficients as power series in th2 = |w|^2 (|w| <= pi: 16 Horner terms each,
// absolute error <= 2.6e-16 against 40-digit values): sin(th)/th, (1 - cos th)/th^2 and
// (th - sin th)/th^3. No square root, division or sincos: a chain of 16 dependent FMAs
// (three independent chains) instead of ~120 instructions with long-latency steps — the
// table build is on the critical path of every evaluation pass (k_eval_bal's ablation: the
// tables alone took 4 of a C3 launch's 23.5 us)
// fma(a, b, k) with the 64-bit constant k in an SGPR pair (one VOP3 v_fma_f64, bitwise the
// same as fma()): left to itself hipcc materialises every Horner coefficient into VGPRs (two
// v_mov_b32 per step, since v_fmac needs its addend in the destination), which tripled the
// VALU count of each series — the point tables of every k_eval_bal work-group run them
__device__ __forceinline__ double fma_sk(double a, double b, double k) {
  double r;
  asm("v_fma_f64 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(k));
  return r;
}
template <int OFF>
__device__ __forceinline__ double rodrigues_series(double x) {
  // coefficients (-1)^k / (2k + 1 + OFF)!, k = 0 .. 15
  constexpr double c[16] = {
      1.0 / 1.0, -1.0 / 6.0, 1.0 / 120.0, -1.0 / 5040.0, 1.0 / 362880.0, -1.0 / 39916800.0,
      1.0 / 6227020800.0, -1.0 / 1307674368000.0, 1.0 / 355687428096000.0, -1.0 / 121645100408832000.0,
      1.0 / 51090942171709440000.0, -1.0 / 25852016738884976640000.0, 1.0 / 15511210043330985984000000.0,
      -1.0 / 10888869450418352160768000000.0, 1.0 / 8841761993739701954543616000000.0,
      -1.0 / 8222838654177922817725562880000000.0};  // (-1)^k / (2k+1)!
  constexpr double d[16] = {
      1.0 / 2.0, -1.0 / 24.0, 1.0 / 720.0, -1.0 / 40320.0, 1.0 / 3628800.0, -1.0 / 479001600.0,
      1.0 / 87178291200.0, -1.0 / 20922789888000.0, 1.0 / 6402373705728000.0, -1.0 / 2432902008176640000.0,
      1.0 / 1124000727777607680000.0, -1.0 / 620448401733239439360000.0,
      1.0 / 403291461126605635584000000.0, -1.0 / 304888344611713860501504000000.0,
      1.0 / 265252859812191058636308480000000.0, -1.0 / 263130836933693530167218012160000000.0};  // (2k+2)!
  constexpr double e[16] = {
      1.0 / 6.0, -1.0 / 120.0, 1.0 / 5040.0, -1.0 / 362880.0, 1.0 / 39916800.0, -1.0 / 6227020800.0,
      1.0 / 1307674368000.0, -1.0 / 355687428096000.0, 1.0 / 121645100408832000.0,
      -1.0 / 51090942171709440000.0, 1.0 / 25852016738884976640000.0, -1.0 / 15511210043330985984000000.0,
      1.0 / 10888869450418352160768000000.0, -1.0 / 8841761993739701954543616000000.0,
      1.0 / 8222838654177922817725562880000000.0,
      -1.0 / 8683317618811886495518194401280000000.0};  // (2k+3)!
  const double* k = OFF == 0 ? c : OFF == 1 ? d : e;
  double r = k[15];
#pragma unroll
  for (int i = 14; i >= 0; --i) r = fma_sk(r, x, k[i]);
  return r;
}
// R (row-major), t, Rd, Jd of one extrinsic (w, t): the table every pass reads
__device__ __forceinline__ void cam_table(const double* __restrict__ ext6, double (&T)[30]) {
  const double w0 = ext6[0], w1 = ext6[1], w2 = ext6[2];
  double* R = T;
  double* Rd = T + 12;
  double* Jd = T + 21;
  const double th2 = w0 * w0 + w1 * w1 + w2 * w2;
  if (th2 > DBL_EPSILON) {
    // ceres::AngleAxisToRotationMatrix (cos th I + sin th [k]x + (1 - cos th) k k^T, k = w / th),
    // written with sc = sin th / th, cc = (1 - cos th) / th^2 on w itself; row-major. The
    // right Jacobian J_r = I - cc [w]x + bb [w]x^2, bb = (th - sin th) / th^3.
    double sc, cc, bb;
    if (th2 < 9.8696044010893586) {  // |w| < pi
      sc = rodrigues_series<0>(th2);
      cc = rodrigues_series<1>(th2);
      bb = rodrigues_series<2>(th2);
    } else {
      const double th = sqrt(th2);
      double sn, cs;
      sincos(th, &sn, &cs);
      sc = sn / th;
      const double sh = sin(0.5 * th);
      cc = 2.0 * sh * sh / th2;
      bb = (th - sn) / (th2 * th);
    }
    const double cs = 1.0 - cc * th2;
    R[0] = cs + cc * w0 * w0;      R[1] = cc * w0 * w1 - sc * w2; R[2] = sc * w1 + cc * w0 * w2;
    R[3] = sc * w2 + cc * w0 * w1; R[4] = cs + cc * w1 * w1;      R[5] = -sc * w0 + cc * w1 * w2;
    R[6] = -sc * w1 + cc * w0 * w2; R[7] = sc * w0 + cc * w1 * w2; R[8] = cs + cc * w2 * w2;
#pragma unroll
    for (int i = 0; i < 9; ++i) Rd[i] = R[i];
    const double a = cc, b = bb;
    Jd[0] = 1.0 + b * (w0 * w0 - th2); Jd[1] = a * w2 + b * w0 * w1;        Jd[2] = -a * w1 + b * w0 * w2;
    Jd[3] = -a * w2 + b * w1 * w0;     Jd[4] = 1.0 + b * (w1 * w1 - th2); Jd[5] = a * w0 + b * w1 * w2;
    Jd[6] = a * w1 + b * w2 * w0;      Jd[7] = -a * w0 + b * w2 * w1;     Jd[8] = 1.0 + b * (w2 * w2 - th2);
  } else {
    R[0] = 1.0; R[1] = -w2; R[2] = w1;
    R[3] = w2;  R[4] = 1.0; R[5] = -w0;
    R[6] = -w1; R[7] = w0;  R[8] = 1.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) Rd[i] = (i % 4 == 0) ? 1.0 : 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) Jd[i] = (i % 4 == 0) ? 1.0 : 0.0;
  }
  T[9] = ext6[3];
  T[10] = ext6[4];
  T[11] = ext6[5];
}

// ------------------------------------------------------------------------------------
// residual + Jacobian (rows a1-a4)
// ------------------------------------------------------------------------------------
struct Proj {
  double ru, rv;
  double A0[3], A1[3];  // d(ru,rv)/dP
  double rho;           // rho(ru^2 + rv^2) of the raw residual; set under a non-trivial loss only
};

// Robust loss (dab_set_loss), Ceres' definitions over s = ru^2 + rv^2 with a = scale, b = a^2,
// c = 1 / b: rho(s) and rho'(s). Every one has rho'' <= 0, so Ceres' Corrector takes its
// first branch (alpha = 0): the minimiser sees sqrt(rho') r and sqrt(rho') J, and the cost is
// 0.5 sum rho. LOSS is a compile-time parameter of every kernel that evaluates rows: the
// TRIVIAL instantiations contain none of this.
struct LossK {
  double a, b, c;
};
__device__ __forceinline__ LossK loss_of(const DevView& v) { return LossK{v.loss_a, v.loss_b, v.loss_c}; }
template <int LOSS>
__device__ __forceinline__ void loss_eval(const LossK& lk, double s, double& rho, double& rho1) {
  static_assert(LOSS == DAB_LOSS_HUBER || LOSS == DAB_LOSS_SOFT_L1 || LOSS == DAB_LOSS_CAUCHY, "loss");
  if constexpr (LOSS == DAB_LOSS_HUBER) {
    // both branches by select: s = 0 (a / 0) never reaches a sum
    const double r = sqrt(s);
    const bool in = s <= lk.b;
    rho = in ? s : 2.0 * lk.a * r - lk.b;
    rho1 = in ? 1.0 : fmax(DBL_MIN, lk.a / r);
  } else if constexpr (LOSS == DAB_LOSS_SOFT_L1) {
    const double t = sqrt(1.0 + s * lk.c);
    rho = 2.0 * lk.b * (t - 1.0);
    rho1 = fmax(DBL_MIN, 1.0 / t);
  } else {
    const double u = 1.0 + s * lk.c;
    rho = lk.b * log(u);
    rho1 = fmax(DBL_MIN, 1.0 / u);
  }
}

// LOSS != TRIVIAL: o.rho = rho(s) of the raw residual; with want_jac the residual and the rows
// leave scaled by sqrt(rho'(s)) (without it, the candidate's residual stays raw: only rho is used)
template <int LOSS = DAB_LOSS_TRIVIAL>
__device__ __forceinline__ void project(const double P[3], const double* __restrict__ K, double ox,
                                        double oy, Proj& o, bool want_jac, const LossK& lk = LossK{}) {
  const double cx = K[0], cy = K[1], fx = K[2], fy = K[3], k0 = K[4], k1 = K[5];
  // one reciprocal for the perspective divide and its derivative: v_rcp_f64 refined by
  // two Newton steps (within 1 ulp of the two divisions of the functor; 5 instructions
  // instead of the 10 of an IEEE division). P2 = 0 gives a non-finite residual either way.
  double iz = __builtin_amdgcn_rcp(P[2]);
  iz = fma(iz, fma(-P[2], iz, 1.0), iz);
  iz = fma(iz, fma(-P[2], iz, 1.0), iz);
  const double xp = P[0] * iz;
  const double yp = P[1] * iz;
  const double r2 = xp * xp + yp * yp;
  // |k| = 0, 1, 2 are all this expression with unused coefficients zeroed (exact)
  const double d = 1.0 + r2 * (k0 + k1 * r2);
  o.ru = fx * d * xp + cx - ox;
  o.rv = fy * d * yp + cy - oy;
  double rho1 = 1.0;
  if constexpr (LOSS != DAB_LOSS_TRIVIAL) loss_eval<LOSS>(lk, o.ru * o.ru + o.rv * o.rv, o.rho, rho1);
  if (!want_jac) return;
  const double dd = k0 + 2.0 * k1 * r2;
  const double du_dx = fx * (d + 2.0 * xp * xp * dd), du_dy = fx * (2.0 * xp * yp * dd);
  const double dv_dx = fy * (2.0 * xp * yp * dd), dv_dy = fy * (d + 2.0 * yp * yp * dd);
  o.A0[0] = du_dx * iz;
  o.A0[1] = du_dy * iz;
  o.A0[2] = -(du_dx * xp + du_dy * yp) * iz;
  o.A1[0] = dv_dx * iz;
  o.A1[1] = dv_dy * iz;
  o.A1[2] = -(dv_dx * xp + dv_dy * yp) * iz;
  if constexpr (LOSS != DAB_LOSS_TRIVIAL) {
    const double w = sqrt(rho1);
    o.ru *= w;
    o.rv *= w;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      o.A0[i] *= w;
      o.A1[i] *= w;
    }
  }
}

__device__ __forceinline__ void rowmat(const double a[3], const double* __restrict__ M, double o[3]) {
  o[0] = a[0] * M[0] + a[1] * M[3] + a[2] * M[6];
  o[1] = a[0] * M[1] + a[1] * M[4] + a[2] * M[7];
  o[2] = a[0] * M[2] + a[1] * M[5] + a[2] * M[8];
}
__device__ __forceinline__ void matvec_add(const double* __restrict__ M, const double x[3],
                                           const double* __restrict__ t, double o[3]) {
  o[0] = M[0] * x[0] + M[1] * x[1] + M[2] * x[2] + t[0];
  o[1] = M[3] * x[0] + M[4] * x[1] + M[5] * x[2] + t[1];
  o[2] = M[6] * x[0] + M[7] * x[1] + M[8] * x[2] + t[2];
}
// o = -((a x X)^T Jd)
__device__ __forceinline__ void dwrot(const double a[3], const double X[3], const double* __restrict__ Jd,
                                      double o[3]) {
  const double c0 = a[1] * X[2] - a[2] * X[1];
  const double c1 = a[2] * X[0] - a[0] * X[2];
  const double c2 = a[0] * X[1] - a[1] * X[0];
  o[0] = -(c0 * Jd[0] + c1 * Jd[3] + c2 * Jd[6]);
  o[1] = -(c0 * Jd[1] + c1 * Jd[4] + c2 * Jd[7]);
  o[2] = -(c0 * Jd[2] + c1 * Jd[5] + c2 * Jd[8]);
}

template <int NT>
__device__ __forceinline__ void load_tab(const double* __restrict__ camtab, int e, double (&T)[NT]) {
  const double2* p = reinterpret_cast<const double2*>(camtab + (size_t)kCamTab * e);
#pragma unroll
  for (int i = 0; i < NT / 2; ++i) {
    const double2 v = p[i];
    T[2 * i] = v.x;
    T[2 * i + 1] = v.y;
  }
}

// One observation: residual and every Jacobian row, from the camera tables.
struct ObsJac {
  Proj pr;
  double jx0[3], jx1[3];    // d r / d X
  double jw0a[3], jw0b[3];  // d r / d w0   (rows 0, 1)
  double jw1a[3], jw1b[3];  // d r / d w1
  double jt1a[3], jt1b[3];  // d r / d t1   (d r / d t0 = pr.A0 / pr.A1)
};

// Table rows come in with 16-byte vector loads into registers: in BAL-shaped problems
// every lane of a wave reads a different camera, so the number of load instructions
// (not bytes) is what the L2 sees. R,t first (needed for the residual), Rd/Jd only by the
// passes that want camera rows.
template <int OFF, int NT>
__device__ __forceinline__ void load_tab_at(const double* __restrict__ camtab, int e, double (&T)[NT]) {
  const double2* p = reinterpret_cast<const double2*>(camtab + (size_t)kCamTab * e + OFF);
#pragma unroll
  for (int i = 0; i < NT / 2; ++i) {
    const double2 v = p[i];
    T[2 * i] = v.x;
    T[2 * i + 1] = v.y;
  }
}
__device__ __forceinline__ void load_intr(const double* __restrict__ intr, int i, double (&K)[6]) {
  const double2* p = reinterpret_cast<const double2*>(intr + (size_t)kIntr * i);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double2 v = p[k];
    K[2 * k] = v.x;
    K[2 * k + 1] = v.y;
  }
}

// Where a pass reads the per-camera tables from: global memory (L2-resident), or R,t
// (and K when it fits) staged once per work-group in LDS.
struct GlobalTabs {
  const double* __restrict__ camtab;
  const double* __restrict__ intr;
  __device__ __forceinline__ void rt(int e, double (&T)[12]) const { load_tab_at<0, 12>(camtab, e, T); }
  __device__ __forceinline__ void dj(int e, double (&T)[18]) const { load_tab_at<12, 18>(camtab, e, T); }
  __device__ __forceinline__ void k(int i, double (&K)[6]) const { load_intr(intr, i, K); }
};
// One camera and intrinsic for the whole work-group (chunk_uni): the table is computed once
// from the extrinsic (uniform values) and the per-entry index is ignored.
struct UniTabs {
  double T[30];  // R t Rd Jd
  double K[6];
  __device__ __forceinline__ UniTabs(const double* __restrict__ ext, const double* __restrict__ intr, int e,
                                     int i) {
    cam_table(ext + 6 * (size_t)e, T);  // built in place: no table pass needed before this one
    const double* k = intr + (size_t)kIntr * i;
#pragma unroll
    for (int q = 0; q < 6; ++q) K[q] = k[q];
    // the values are wave-uniform: keep them in SGPRs, not 72 VGPRs
#pragma unroll
    for (int q = 0; q < 30; ++q) T[q] = uniform(T[q]);
#pragma unroll
    for (int q = 0; q < 6; ++q) K[q] = uniform(K[q]);
  }
  static __device__ __forceinline__ double uniform(double x) {
    const int lo = __builtin_amdgcn_readfirstlane(__double2loint(x));
    const int hi = __builtin_amdgcn_readfirstlane(__double2hiint(x));
    return __hiloint2double(hi, lo);
  }
  __device__ __forceinline__ void rt(int, double (&o)[12]) const {
#pragma unroll
    for (int q = 0; q < 12; ++q) o[q] = T[q];
  }
  __device__ __forceinline__ void dj(int, double (&o)[18]) const {
#pragma unroll
    for (int q = 0; q < 18; ++q) o[q] = T[12 + q];
  }
  __device__ __forceinline__ void k(int, double (&o)[6]) const {
#pragma unroll
    for (int q = 0; q < 6; ++q) o[q] = K[q];
  }
};

// Every extrinsic's R t Rd Jd and every intrinsic staged in LDS once per block (small
// camera sets: the rig's 79 extrinsics and 16 intrinsics take 20 KB); per-entry table
// reads then come from LDS instead of L2 gathers.
constexpr int kSmallTabs = 128;   // E and NI limit
constexpr int kSmallGrid = 2048;  // grid-stride blocks of the staged-table variants
__host__ __device__ inline bool small_tabs_fit(int E, int NI) { return E <= kSmallTabs && NI <= kSmallTabs; }
__host__ __device__ inline size_t small_tabs_bytes(int E, int NI) { return sizeof(double) * (30 * (size_t)E + 6 * (size_t)NI); }
struct SmallTabs {
  const double* t_s;  // LDS [E][30]
  const double* k_s;  // LDS [NI][6]
  __device__ __forceinline__ void rt(int e, double (&o)[12]) const {
    const double2* p = reinterpret_cast<const double2*>(t_s + 30 * e);
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      const double2 u = p[q];
      o[2 * q] = u.x;
      o[2 * q + 1] = u.y;
    }
  }
  __device__ __forceinline__ void dj(int e, double (&o)[18]) const {
    const double2* p = reinterpret_cast<const double2*>(t_s + 30 * e + 12);
#pragma unroll
    for (int q = 0; q < 9; ++q) {
      const double2 u = p[q];
      o[2 * q] = u.x;
      o[2 * q + 1] = u.y;
    }
  }
  __device__ __forceinline__ void k(int i, double (&o)[6]) const {
    const double2* p = reinterpret_cast<const double2*>(k_s + 6 * i);
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const double2 u = p[q];
      o[2 * q] = u.x;
      o[2 * q + 1] = u.y;
    }
  }
};
// block-cooperative staging into dynamic LDS; returns the table view (barrier inside)
__device__ __forceinline__ SmallTabs stage_small_tabs(double* lds, int E, int NI, const double* __restrict__ camtab,
                                                      const double* __restrict__ intr) {
  double* t_s = lds;
  double* k_s = lds + 30 * (size_t)E;
  for (int i = threadIdx.x; i < 30 * E; i += blockDim.x) t_s[i] = camtab[(size_t)kCamTab * (i / 30) + i % 30];
  for (int i = threadIdx.x; i < 6 * NI; i += blockDim.x) k_s[i] = intr[(size_t)kIntr * (i / 6) + i % 6];
  __syncthreads();
  return SmallTabs{t_s, k_s};
}
template <bool K_IN_LDS, bool KMASK = false>
struct LdsTabs {
  const double* rt_s;  // LDS [E][12]: R t
  const double* k_s;   // LDS [NI][6] when K_IN_LDS
  const double* __restrict__ camtab;
  const double* __restrict__ intr;
  __device__ __forceinline__ void rt(int e, double (&T)[12]) const {
    const double2* p = reinterpret_cast<const double2*>(rt_s + 12 * e);
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const double2 v = p[i];
      T[2 * i] = v.x;
      T[2 * i + 1] = v.y;
    }
  }
  __device__ __forceinline__ void dj(int e, double (&T)[18]) const { load_tab_at<12, 18>(camtab, e, T); }
  __device__ __forceinline__ void k(int i, double (&K)[6]) const {
    if constexpr (K_IN_LDS) {
      const double2* p = reinterpret_cast<const double2*>(k_s + 6 * (KMASK ? (i & 127) : i));
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const double2 v = p[q];
        K[2 * q] = v.x;
        K[2 * q + 1] = v.y;
      }
    } else {
      load_intr(intr, i, K);
    }
  }
};

// Residual and the Jacobian rows of one observation that a pass needs, from the camera
// tables. JP: d r / d X (2x3). SLOT 0: d r / d (w0, t0); SLOT 1: d r / d (w1, t1) of the
// ring camera of an arc∘ring observation; SLOT 2: both (jc0/jc1 = slot 0 rows, jd0/jd1 =
// slot 1 rows); SLOT -1: no camera rows. Q is the point the arc/single rotation acts on:
// X (single) or P2 = R1 X + t1 (arc∘ring).
// MAYCOMP = false: the caller knows no observation is arc∘ring (ext1 < 0 everywhere), so
// the second table is never read and its registers are never allocated.
// obs_rows_l: the same under loss LOSS — residual and rows scaled by sqrt(rho') (project), rho
// = rho(s) of the raw residual (untouched for TRIVIAL, where obs_rows_l IS obs_rows).
template <int LOSS, bool JP, int SLOT, bool MAYCOMP = true, class Tabs>
__device__ __forceinline__ void obs_rows_l(const LossK& lk, double& rho, const int4 id, const double2 xy,
                                           const double X[3], const Tabs& tb, double& ru, double& rv,
                                           double jx0[3], double jx1[3], double jc0[6], double jc1[6],
                                           double jd0[6] = nullptr, double jd1[6] = nullptr) {
  const bool comp = MAYCOMP && id.z >= 0;
  double A[12];  // R0 | t0
  tb.rt(id.y, A);
  double Kr[6];
  tb.k(id.w, Kr);
  double Q[3], B[12];  // B = R1 | t1 (arc∘ring only)
  if (comp) {
    tb.rt(id.z, B);
    matvec_add(B, X, B + 9, Q);
  } else {
    Q[0] = X[0];
    Q[1] = X[1];
    Q[2] = X[2];
  }
  double P[3];
  matvec_add(A, Q, A + 9, P);
  Proj pr;
  project<LOSS>(P, Kr, xy.x, xy.y, pr, true, lk);
  ru = pr.ru;
  rv = pr.rv;
  if constexpr (LOSS != DAB_LOSS_TRIVIAL) rho = pr.rho;
  if constexpr (SLOT == 0 || SLOT == 2) {
    double D[18];  // Rd0 | Jd0
    tb.dj(id.y, D);
    double Da[3], Db[3];
    rowmat(pr.A0, D, Da);
    rowmat(pr.A1, D, Db);
    dwrot(Da, Q, D + 9, jc0);
    dwrot(Db, Q, D + 9, jc1);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      jc0[3 + i] = pr.A0[i];
      jc1[3 + i] = pr.A1[i];
    }
  }
  if constexpr (JP || SLOT >= 1) {
    double B0a[3], B0b[3];
    rowmat(pr.A0, A, B0a);  // A R0
    rowmat(pr.A1, A, B0b);
    if constexpr (SLOT >= 1) {
      double* o0 = SLOT == 1 ? jc0 : jd0;
      double* o1 = SLOT == 1 ? jc1 : jd1;
      if (comp) {
        double D[18];  // Rd1 | Jd1
        tb.dj(id.z, D);
        double Ca[3], Cb[3];
        rowmat(B0a, D, Ca);
        rowmat(B0b, D, Cb);
        dwrot(Ca, X, D + 9, o0);
        dwrot(Cb, X, D + 9, o1);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          o0[3 + i] = B0a[i];
          o1[3 + i] = B0b[i];
        }
      } else {
#pragma unroll
        for (int i = 0; i < 6; ++i) {
          o0[i] = 0.0;
          o1[i] = 0.0;
        }
      }
    }
    if constexpr (JP) {
      if (comp) {
        rowmat(B0a, B, jx0);
        rowmat(B0b, B, jx1);
      } else {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          jx0[i] = B0a[i];
          jx1[i] = B0b[i];
        }
      }
    }
  }
}

template <bool JP, int SLOT, class Tabs, bool MAYCOMP = true>
__device__ __forceinline__ void obs_rows(const int4 id, const double2 xy, const double X[3], const Tabs& tb,
                                         double& ru, double& rv, double jx0[3], double jx1[3], double jc0[6],
                                         double jc1[6], double jd0[6] = nullptr, double jd1[6] = nullptr) {
  double rho;
  obs_rows_l<DAB_LOSS_TRIVIAL, JP, SLOT, MAYCOMP>(LossK{}, rho, id, xy, X, tb, ru, rv, jx0, jx1, jc0, jc1, jd0, jd1);
}

// Every row of one observation (parity API, cross blocks, candidate pass).
template <int LOSS = DAB_LOSS_TRIVIAL, class Tabs>
__device__ __forceinline__ void obs_jacobian_t(const int4 id, const double2 xy, const double X[3], const Tabs& tb,
                                               ObsJac& o, const LossK& lk = LossK{}) {
  double c0[6], c1[6], d0[6], d1[6];
  obs_rows_l<LOSS, true, 2>(lk, o.pr.rho, id, xy, X, tb, o.pr.ru, o.pr.rv, o.jx0, o.jx1, c0, c1, d0, d1);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    o.jw0a[i] = c0[i];
    o.jw0b[i] = c1[i];
    o.pr.A0[i] = c0[3 + i];
    o.pr.A1[i] = c1[3 + i];
    o.jw1a[i] = d0[i];
    o.jw1b[i] = d1[i];
    o.jt1a[i] = d0[3 + i];
    o.jt1b[i] = d1[3 + i];
  }
}
__device__ __forceinline__ void obs_jacobian(const int4 id, const double2 xy, const double X[3],
                                             const double* __restrict__ camtab,
                                             const double* __restrict__ intr, ObsJac& o) {
  obs_jacobian_t(id, xy, X, GlobalTabs{camtab, intr}, o);
}

// entry k (< 27) of the camera's [U upper-packed | g_c] from the point-frame sums s
// (same packing): U_rr = J^T U~_rr J, U_rt = J^T U~_rt, U_tt = U~_tt, g_r = J^T g~_r
__device__ __forceinline__ int upk6(int a, int b) {  // packed index of (a, b), a <= b
  return a * 6 - a * (a - 1) / 2 + (b - a);
}
__device__ __forceinline__ double cam_frame_entry(const double* s, const double* J, int k) {
  if (k >= 21) {
    const int i = k - 21;
    if (i >= 3) return s[k];
    return J[i] * s[21] + J[3 + i] * s[22] + J[6 + i] * s[23];
  }
  int a = 0, r = k;
  while (r >= 6 - a) {
    r -= 6 - a;
    ++a;
  }
  const int b = a + r;
  if (a >= 3) return s[k];
  if (b >= 3) return J[a] * s[upk6(0, b)] + J[3 + a] * s[upk6(1, b)] + J[6 + a] * s[upk6(2, b)];
  double t = 0.0;
#pragma unroll
  for (int p = 0; p < 3; ++p) {
    double u = 0.0;
#pragma unroll
    for (int q = 0; q < 3; ++q) u += s[upk6(min(p, q), max(p, q))] * J[3 * q + b];
    t += J[3 * p + a] * u;
  }
  return t;
}

// camera-space point of an observation, as obs_rows_l forms it
template <class Tabs>
__device__ __forceinline__ void obs_cam_point(const int4 id, const double X[3], const Tabs& tb, double (&P)[3]) {
  double A[12];
  tb.rt(id.y, A);
  double Q[3];
  if (id.z >= 0) {
    double B[12];
    tb.rt(id.z, B);
    matvec_add(B, X, B + 9, Q);
  } else {
    Q[0] = X[0];
    Q[1] = X[1];
    Q[2] = X[2];
  }
  matvec_add(A, Q, A + 9, P);
}
// d r / d (cx, cy, f0, f1, k0, k1) of one observation (rows z0 = d ru, z1 = d rv) with project's
// own expressions for xp, yp, r2, d; under a loss scaled by sqrt(rho') of the raw residual as
// project scales the other rows. cols: bit a set = column a is kept (else zero); nf1: the
// single focal length drives both rows (column 2).
template <int LOSS>
__device__ __forceinline__ void intr_rows(const double P[3], const double* __restrict__ K, double ox, double oy,
                                          const LossK& lk, int cols, bool nf1, double (&z0)[6], double (&z1)[6]) {
  const double cx = K[0], cy = K[1], fx = K[2], fy = K[3], k0 = K[4], k1 = K[5];
  double iz = __builtin_amdgcn_rcp(P[2]);
  iz = fma(iz, fma(-P[2], iz, 1.0), iz);
  iz = fma(iz, fma(-P[2], iz, 1.0), iz);
  const double xp = P[0] * iz;
  const double yp = P[1] * iz;
  const double r2 = xp * xp + yp * yp;
  const double d = 1.0 + r2 * (k0 + k1 * r2);
  double w = 1.0;
  if constexpr (LOSS != DAB_LOSS_TRIVIAL) {
    const double ru = fx * d * xp + cx - ox;
    const double rv = fy * d * yp + cy - oy;
    double rho, rho1;
    loss_eval<LOSS>(lk, ru * ru + rv * rv, rho, rho1);
    w = sqrt(rho1);
  }
  z0[0] = w;
  z1[0] = 0.0;
  z0[1] = 0.0;
  z1[1] = w;
  z0[2] = w * (d * xp);
  z1[2] = nf1 ? w * (d * yp) : 0.0;
  z0[3] = 0.0;
  z1[3] = nf1 ? 0.0 : w * (d * yp);
  z0[4] = w * (fx * r2 * xp);
  z1[4] = w * (fy * r2 * yp);
  z0[5] = w * (fx * r2 * r2 * xp);
  z1[5] = w * (fy * r2 * r2 * yp);
#pragma unroll
  for (int a = 0; a < 6; ++a)
    if (!((cols >> a) & 1)) {
      z0[a] = 0.0;
      z1[a] = 0.0;
    }
}

}  // namespace dab
