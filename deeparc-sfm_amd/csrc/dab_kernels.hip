// dab_kernels.hip — gfx950 kernels of the BA hot path.
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
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cstdlib>
#include <type_traits>

#include "dab_kernels.h"
#include "dab_wave.h"

namespace dab {

#ifdef DAB_TRACE
// timing build only (scripts/trace_build.sh): per-wave s_memrealtime stamps (100 MHz), kept
// in LDS while the wave runs (a global store per stamp would sit in the wave's vmcnt and
// delay the hop stamps below) and copied out by stamp 3, which every exit path takes
__device__ unsigned long long g_trace[256 * 16 * 8];
__device__ unsigned g_hwid[256 * 16];  // HW_REG_HW_ID of every wave (its SIMD, CU, SE)
__shared__ unsigned long long g_trace_lds[16 * 8];
#define DAB_TRACE_INIT()                                                                   \
  do {                                                                                     \
    if ((threadIdx.x & 63) < 8) g_trace_lds[(threadIdx.x >> 6) * 8 + (threadIdx.x & 63)] = 0ull; \
    if ((threadIdx.x & 63) == 0 && blockIdx.x < 256)                                       \
      g_hwid[blockIdx.x * 16 + (threadIdx.x >> 6)] = __builtin_amdgcn_s_getreg((31 << 11) | 4); \
  } while (0)
#define DAB_STAMP_ANY(k)                                                                   \
  do {                                                                                     \
    const unsigned long long t_ = __builtin_amdgcn_s_memrealtime();                         \
    if ((threadIdx.x & 63) == 0) g_trace_lds[(threadIdx.x >> 6) * 8 + (k)] = t_;             \
    if ((k) == 3 && (threadIdx.x & 63) < 8 && blockIdx.x < 256)                            \
      g_trace[(blockIdx.x * 16 + (threadIdx.x >> 6)) * 8 + (threadIdx.x & 63)] =            \
          g_trace_lds[(threadIdx.x >> 6) * 8 + (threadIdx.x & 63)];                        \
  } while (0)
#define DAB_STAMP(k) DAB_STAMP_ANY(k)
// a stamp once every load in flight has returned (prologue hops; perturbs the schedule a little)
#define DAB_STAMP_HOP(k)                                        \
  do {                                                          \
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); \
    DAB_STAMP_ANY(k);                                           \
  } while (0)
#else
#define DAB_TRACE_INIT() \
  do {                   \
  } while (0)
#define DAB_STAMP_HOP(k) \
  do {                   \
  } while (0)
#define DAB_STAMP_ANY(k) \
  do {                   \
  } while (0)
#define DAB_STAMP(k) \
  do {               \
  } while (0)
#endif

int grid_for(int n, int block, int cap) {
  int g = (n + block - 1) / block;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return g;
}

// ------------------------------------------------------------------------------------
// reductions
// ------------------------------------------------------------------------------------
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

__global__ void k_seg_final(int nseg, int K, const int* __restrict__ seg_chunk,
                            const double* __restrict__ partial, double* __restrict__ out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nseg * K) return;
  const int seg = t / K, k = t - seg * K;
  double v = 0.0;
  for (int c = seg_chunk[seg]; c < seg_chunk[seg + 1]; ++c) v += partial[(size_t)c * K + k];
  out[t] = v;
}

// one block of 256 threads: strided per-thread sums in fixed order, then a fixed tree
__global__ __launch_bounds__(256) void k_final_sum(int grid, int K, const double* __restrict__ partial,
                                                   double* __restrict__ out, unsigned max_mask) {
  __shared__ double sh[256];
  const int t = threadIdx.x;
  for (int k = 0; k < K; ++k) {
    const bool is_max = (max_mask >> k) & 1u;
    double v = 0.0;
    for (int c = t; c < grid; c += 256) {
      const double x = partial[(size_t)c * K + k];
      v = is_max ? fmax(v, x) : v + x;
    }
    sh[t] = v;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
      if (t < off) sh[t] = is_max ? fmax(sh[t], sh[t + off]) : sh[t] + sh[t + off];
      __syncthreads();
    }
    if (t == 0) out[k] = sh[0];
    __syncthreads();
  }
}

// One 1024-thread block; each thread's (at most a few) elements have all their loads in
// flight together (the 256-thread loop form waited on ~24 dependent load pairs per thread:
// 18.7 us at C3, twice per LM iteration). Sums: wave DPP sums, then the 16 waves in order;
// the max is order-free.
__global__ __launch_bounds__(1024) void k_cam_norms(int E, const int* __restrict__ ext_col,
                                                    const double* __restrict__ ext,
                                                    const double* __restrict__ ext_c,
                                                    const double* __restrict__ ug, double* __restrict__ out) {
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

void launch_cam_norms(hipStream_t s, int E, const int* ext_col, const double* ext, const double* ext_c,
                      const double* ug, double* out) {
  k_cam_norms<<<1, 1024, 0, s>>>(E, ext_col, ext, ext_c, ug, out);
}
// segments with many chunks: one 256-thread block per segment, thread (k, stripe) sums the
// stripe's chunks of component k, the stripes are added in order
__global__ __launch_bounds__(256) void k_seg_final_block(int K, const int* __restrict__ seg_chunk,
                                                          const double* __restrict__ partial,
                                                          double* __restrict__ out) {
  __shared__ double sh[256];
  const int seg = blockIdx.x;
  const int stripes = 256 / K;
  const int k = threadIdx.x % K, stripe = threadIdx.x / K;
  double v = 0.0;
  if (stripe < stripes)
    for (int c = seg_chunk[seg] + stripe; c < seg_chunk[seg + 1]; c += stripes) v += partial[(size_t)c * K + k];
  sh[threadIdx.x] = v;
  __syncthreads();
  if (threadIdx.x < K) {
    double t = sh[threadIdx.x];
    for (int q = 1; q < stripes; ++q) t += sh[q * K + threadIdx.x];
    out[(size_t)seg * K + threadIdx.x] = t;
  }
}

void launch_seg_final(hipStream_t s, int nseg, int K, const int* seg_chunk, const double* partial,
                      double* out, int max_chunks) {
  if (nseg <= 0) return;
  if (max_chunks > 8) {
    k_seg_final_block<<<nseg, 256, 0, s>>>(K, seg_chunk, partial, out);
    return;
  }
  const int n = nseg * K;
  k_seg_final<<<grid_for(n, 256, 1 << 20), 256, 0, s>>>(nseg, K, seg_chunk, partial, out);
}
void launch_final_sum(hipStream_t s, int grid, int K, const double* partial, double* out,
                      unsigned max_mask) {
  k_final_sum<<<1, 256, 0, s>>>(grid, K, partial, out, max_mask);
}

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

__global__ void k_cam_tables(int E, const double* __restrict__ ext, double* __restrict__ tab) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  double T[30];
  cam_table(ext + 6 * (size_t)e, T);
  double* o = tab + (size_t)kCamTab * e;
#pragma unroll
  for (int i = 0; i < 30; ++i) o[i] = T[i];
  o[30] = 0.0;
  o[31] = 0.0;
}

void launch_cam_tables(hipStream_t s, int E, const double* ext, double* camtab) {
  if (E <= 0) return;
  k_cam_tables<<<grid_for(E, 64, 1 << 20), 64, 0, s>>>(E, ext, camtab);
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

// Point side of the evaluation pass (rows a1-a4 + the point half of a7), matrix-free:
// residual and d r / d X per observation, reduced straight into V = Jp^T Jp (6) and
// g_p = Jp^T r (3). Nothing per observation is written: every later pass re-evaluates
// the rows it needs from the inputs (32 B per observation; the Jacobian is 144-240 B).
// One SELL-64 slice: lane l owns point 64 sl + l (its X loaded once), wave w of the WPS
// waves takes the slice's observation rows k = w, w + WPS, ... (coalesced 64-slot rows),
// and the per-wave sums are combined in LDS (sh[WPS-1][9][64]) in a fixed order: no
// cross-lane scan. Every wave of the work-group calls this the same number of times
// (sl >= nslice: no work, barriers only).
template <int WPS, int VAR, int LOSS = DAB_LOSS_TRIVIAL, class Tabs>
__device__ __forceinline__ void eval_slice(const DevView& v, const double* __restrict__ points, const Tabs& tabs,
                                           double* __restrict__ V, double* __restrict__ g, int sl, int w,
                                           double (*sh)[9][64], double (&acc)[2]) {
  const int lane = threadIdx.x & 63;
  const size_t NPs = (size_t)v.NP;
  const bool live = sl < v.nslice;
  const int p = 64 * sl + lane;
  const LossK lk = loss_of(v);
  double c[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) c[k] = 0.0;
  if (live) {
    const int off = v.slice_off[sl], len = (v.slice_off[sl + 1] - off) >> 6;
    double X[3] = {0.0, 0.0, 0.0};
    if (p < v.NP) {
      X[0] = points[3 * (size_t)p];
      X[1] = points[3 * (size_t)p + 1];
      X[2] = points[3 * (size_t)p + 2];
    }
    // rows are software-pipelined: the next row's inputs are in flight while this
    // row computes (each wave walks only len / WPS rows, so latency dominates)
    int4 id_n = make_int4(-1, 0, -1, 0);
    double2 xy_n = make_double2(0.0, 0.0);
    if (w < len) {
      id_n = v.obs_idx[off + 64 * w + lane];
      xy_n = v.obs_xy[off + 64 * w + lane];
    }
    for (int k = w; k < len; k += WPS) {
      int4 id = id_n;
      const double2 xy = xy_n;
      if (k + WPS < len) {
        id_n = v.obs_idx[off + 64 * (k + WPS) + lane];
        xy_n = v.obs_xy[off + 64 * (k + WPS) + lane];
      }
      if (id.x < 0) continue;  // padding slot
      double ru, rv, jx0[3], jx1[3], rho = 0.0;
      if constexpr (VAR == 1) {  // ablation: loads only
        ru = xy.x + id.y;
        rv = xy.y + id.w;
#pragma unroll
        for (int q = 0; q < 3; ++q) jx0[q] = jx1[q] = X[q];
      } else {
        if constexpr (VAR == 2) id.y = id.w = 0;  // ablation: one camera (uniform table loads)
        obs_rows_l<LOSS, true, -1>(lk, rho, id, xy, X, tabs, ru, rv, jx0, jx1, nullptr, nullptr);
      }
      // accumulate as two fused multiply-adds per entry (row 0, then row 1)
      c[0] = fma(jx1[0], jx1[0], fma(jx0[0], jx0[0], c[0]));
      c[1] = fma(jx1[0], jx1[1], fma(jx0[0], jx0[1], c[1]));
      c[2] = fma(jx1[0], jx1[2], fma(jx0[0], jx0[2], c[2]));
      c[3] = fma(jx1[1], jx1[1], fma(jx0[1], jx0[1], c[3]));
      c[4] = fma(jx1[1], jx1[2], fma(jx0[1], jx0[2], c[4]));
      c[5] = fma(jx1[2], jx1[2], fma(jx0[2], jx0[2], c[5]));
      c[6] = fma(jx1[0], rv, fma(jx0[0], ru, c[6]));
      c[7] = fma(jx1[1], rv, fma(jx0[1], ru, c[7]));
      c[8] = fma(jx1[2], rv, fma(jx0[2], ru, c[8]));
      if constexpr (LOSS == DAB_LOSS_TRIVIAL) acc[0] = fma(rv, rv, fma(ru, ru, acc[0]));
      else acc[0] += rho;  // the cost is 0.5 sum rho(s), not 0.5 |scaled r|^2
      acc[1] += (isfinite(ru) && isfinite(rv)) ? 0.0 : 1.0;
    }
  }
  if constexpr (WPS > 1) {
    if (w > 0) {
#pragma unroll
      for (int k = 0; k < 9; ++k) sh[w - 1][k][lane] = c[k];
    }
    __syncthreads();
  }
  if (live && w == 0 && p < v.NP) {
    if constexpr (WPS > 1) {
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        double t = c[k];
#pragma unroll
        for (int q = 0; q < WPS - 1; ++q) t += sh[q][k][lane];
        c[k] = t;
      }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) V[k * NPs + p] = c[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) g[k * NPs + p] = c[6 + k];
  }
  if constexpr (WPS > 1) __syncthreads();
}

// cost partials of a work-group of NW waves: wave sums, then a fixed-order sum
template <int NW>
__device__ __forceinline__ void store_cost_partial(double (&acc)[2], double* __restrict__ partial) {
  __shared__ double shp[NW][2];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const double t = wave_sum_lane63(acc[i]);
    if (lane == 63) shp[w][i] = t;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    double t = shp[0][threadIdx.x];
#pragma unroll
    for (int q = 1; q < NW; ++q) t += shp[q][threadIdx.x];
    partial[2 * (size_t)blockIdx.x + threadIdx.x] = t;
  }
}

// As store_cost_partial, and the last work-group to arrive sums all partials (fixed
// order) into cost[2]. The partials are stored write-through (agent-scope atomic stores)
// and drained before the arrival count, and read back with agent-scope atomic loads: no
// release/acquire fences (the hand-off recipe of the CDNA4 guide, Guideline 16).
template <int NW>
__device__ __forceinline__ void store_cost_partial_last(double (&acc)[2], double* __restrict__ partial,
                                                        unsigned* __restrict__ arrivals, double* __restrict__ cost) {
  __shared__ double shp[NW][2];
  __shared__ int last;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const double t = wave_sum_lane63(acc[i]);
    if (lane == 63) shp[w][i] = t;
  }
  __syncthreads();
  if (threadIdx.x < 64) {
    if (threadIdx.x < 2) {
      double t = shp[0][threadIdx.x];
#pragma unroll
      for (int q = 1; q < NW; ++q) t += shp[q][threadIdx.x];
      __hip_atomic_store(reinterpret_cast<unsigned long long*>(partial) + 2 * (size_t)blockIdx.x + threadIdx.x,
                         (unsigned long long)__double_as_longlong(t), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (threadIdx.x == 0)
      last = __hip_atomic_fetch_add(arrivals, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1;
  }
  __syncthreads();
  if (!last) return;
  __shared__ double red[2][NW];
  const unsigned long long* pp = reinterpret_cast<const unsigned long long*>(partial);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    double v = 0.0;
    for (int c = threadIdx.x; c < (int)gridDim.x; c += blockDim.x)
      v += __longlong_as_double((long long)__hip_atomic_load(pp + 2 * (size_t)c + i, __ATOMIC_RELAXED,
                                                             __HIP_MEMORY_SCOPE_AGENT));
    const double t = wave_sum_lane63(v);
    if (lane == 63) red[i][w] = t;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    double t = red[threadIdx.x][0];
#pragma unroll
    for (int q = 1; q < NW; ++q) t += red[threadIdx.x][q];
    cost[threadIdx.x] = t;
  }
  if (threadIdx.x == 0) __hip_atomic_store(arrivals, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// tables from global memory: one block per slice, grid-strided
template <int WPS, int VAR = 0, int LOSS = DAB_LOSS_TRIVIAL>
__global__ __launch_bounds__(64 * WPS) void k_eval_points(DevView v, const double* __restrict__ points,
                                                          const double* __restrict__ camtab,
                                                          double* __restrict__ V, double* __restrict__ g,
                                                          double* __restrict__ partial) {
  __shared__ double sh[WPS > 1 ? WPS - 1 : 1][9][64];
  const GlobalTabs tabs{camtab, v.intr};
  double acc[2] = {0.0, 0.0};
  const int rounds = (v.nslice + gridDim.x - 1) / gridDim.x;
  for (int r = 0; r < rounds; ++r)
    eval_slice<WPS, VAR, LOSS>(v, points, tabs, V, g, r * gridDim.x + blockIdx.x, threadIdx.x >> 6, sh, acc);
  store_cost_partial<WPS>(acc, partial);
}

// Tables staged in LDS (camera count <= kLdsCams): R,t of every extrinsic (and K of every
// intrinsic when there are at most KI of them) are copied once per work-group, so the
// per-lane table reads of BAL-shaped data (every lane a different camera) become
// ds_read_b128 instead of 64-line L2 gathers. Persistent: one 1024-thread work-group per
// CU, 16 / WPS slices in flight (WPS waves each, rows split, LDS-combined).
constexpr int kLdsCams = 1024;
template <int KI, int WPS, bool KMASK = false, int LOSS = DAB_LOSS_TRIVIAL>  // KMASK: ablation (wrong K, all from LDS)
__global__ __launch_bounds__(1024) void k_eval_points_lds(DevView v, const double* __restrict__ points,
                                                          const double* __restrict__ ext,
                                                          const double* __restrict__ camtab,
                                                          double* __restrict__ V, double* __restrict__ g,
                                                          double* __restrict__ partial,
                                                          unsigned* __restrict__ arrivals,
                                                          double* __restrict__ cost) {
  constexpr int G = 16 / WPS;  // slices in flight per work-group
  __shared__ double rt_s[kLdsCams * 12];
  __shared__ double k_s[KI > 0 ? KI * 6 : 2];
  __shared__ double sh[G][WPS > 1 ? WPS - 1 : 1][9][64];
  // R,t of every extrinsic, computed here from the parameters (no table pass in front)
  for (int e = threadIdx.x; e < v.E; e += blockDim.x) {
    double T[30];
    cam_table(ext + 6 * (size_t)e, T);
#pragma unroll
    for (int q = 0; q < 12; ++q) rt_s[12 * e + q] = T[q];
  }
  if constexpr (KI > 0) {
    for (int i = threadIdx.x; i < (KMASK ? min(v.NI, KI) : v.NI) * 3; i += blockDim.x) {
      const int n = i / 3, q = i - 3 * (i / 3);
      reinterpret_cast<double2*>(k_s)[i] = reinterpret_cast<const double2*>(v.intr + (size_t)kIntr * n)[q];
    }
  }
  __syncthreads();
  const LdsTabs<(KI > 0), KMASK> tabs{rt_s, k_s, camtab, v.intr};
  const int wave = threadIdx.x >> 6, grp = wave / WPS, w = wave % WPS;
  double acc[2] = {0.0, 0.0};
  // slices dealt round robin over the work-groups (slot q of work-group b takes slice
  // q * grid + b): every CU gets a share even when the slices are few (C3: 1,563 slices
  // for 256 CUs), and the long slices (sorted first) spread over all of them
  const int per_wg = (v.nslice + gridDim.x - 1) / gridDim.x;
  const int rounds = (per_wg + G - 1) / G;
  for (int r = 0; r < rounds; ++r)
    eval_slice<WPS, 0, LOSS>(v, points, tabs, V, g, (r * G + grp) * gridDim.x + blockIdx.x, w, sh[grp], acc);
  store_cost_partial_last<16>(acc, partial, arrivals, cost);
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

template <int NW>
__device__ __forceinline__ void cost_fx_add(double (&acc)[2], unsigned long long* __restrict__ fx) {
  __shared__ double shp[NW][2];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const double t = wave_sum_lane63(acc[i]);
    if (lane == 63) shp[w][i] = t;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double p = shp[0][0], b = shp[0][1];
#pragma unroll
    for (int q = 1; q < NW; ++q) {
      p += shp[q][0];
      b += shp[q][1];
    }
    cost_fx_commit(p, b, fx + kFxStride * (blockIdx.x % kFxCopies));
  }
}

// Deep-prefetch variant. The SELL rows of a slice are independent loads, but the kernel
// above keeps only one row per wave in flight, and the work-group's first loads wait
// for the table build. Here every wave holds a queue of D rows (idx + xy, 8 VGPRs per
// row) and issues its first D rows and its points before building the tables, so HBM
// latency overlaps the prologue and ~D x more bytes are in flight per CU. R,t and (when
// NI <= kLdsCams) every intrinsic sit in LDS; the two-wave combine goes through a small
// buffer in three phases of three components, so all three fit in 160 KiB.
template <int D>
struct RowQueue {
  int4 id[D];
  double2 xy[D];
};
template <int WPS, int D>
__device__ __forceinline__ void rowq_fill(const DevView& v, int off, int len, int w, int lane, RowQueue<D>& q) {
#pragma unroll
  for (int d = 0; d < D; ++d) {
    const int k = w + d * WPS;
    if (k < len) {
      q.id[d] = v.obs_idx[off + 64 * k + lane];
      q.xy[d] = v.obs_xy[off + 64 * k + lane];
    } else {
      q.id[d] = make_int4(-1, 0, -1, 0);
      q.xy[d] = make_double2(0.0, 0.0);
    }
  }
}
// VAR (timing ablations, wrong results unless noted): bit 0 no trig in the table build,
// bit 1 loads only (no row math), bit 2 no table staging at all, bit 3 plain partials (no
// cost total), bit 4 no V/g stores, bit 5 no cross-wave combine, bit 6 last-arriver cost
// sum into cost[] instead of the fixed-point atomics (correct results)
template <bool KL, int WPS, int D, int VAR = 0, bool COMP = true, int LOSS = DAB_LOSS_TRIVIAL>
__global__ __launch_bounds__(1024) void k_eval_points_pf(DevView v, const double* __restrict__ points,
                                                         const double* __restrict__ ext,
                                                         double* __restrict__ V, double* __restrict__ g,
                                                         double* __restrict__ partial,
                                                         unsigned* __restrict__ arrivals,
                                                         double* __restrict__ cost,
                                                         unsigned long long* __restrict__ costfx,
                                                         unsigned long long* __restrict__ fx_next) {
  constexpr int G = 16 / WPS;  // slices in flight per work-group
  if (blockIdx.x == 0 && fx_next)
    for (int i = threadIdx.x; i < kFxWords; i += blockDim.x) fx_next[i] = 0ull;
  constexpr int PH = WPS <= 2 ? 3 : 1;  // components per combine phase
  __shared__ double rt_s[kLdsCams * 12];
  __shared__ double k_s[KL ? kLdsCams * 6 : 2];
  __shared__ double sh[WPS > 1 ? G : 1][WPS > 1 ? WPS - 1 : 1][PH][64];
  // wave-uniform indices in SGPRs: slice bounds and row loops become scalar branches
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int grp = wave / WPS, w = wave % WPS;
  const size_t NPs = (size_t)v.NP;
  const int per_wg = (v.nslice + gridDim.x - 1) / gridDim.x;
  const int rounds = (per_wg + G - 1) / G;
  RowQueue<D> q;
  double X[3] = {0.0, 0.0, 0.0};
  int sl = grp * gridDim.x + blockIdx.x;  // round 0 (slot q of the work-group: slice q * grid + b)
  int off = 0, len = 0;
  // round 0's first rows and points go out before the table build
  if (sl < v.nslice) {
    off = v.slice_off[sl];
    len = (v.slice_off[sl + 1] - off) >> 6;
    const int p = 64 * sl + lane;
    if (p < v.NP) {
      X[0] = points[3 * (size_t)p];
      X[1] = points[3 * (size_t)p + 1];
      X[2] = points[3 * (size_t)p + 2];
    }
  }
  rowq_fill<WPS, D>(v, off, len, w, lane, q);
  // table staging: every load of this thread's share (its extrinsic: 3 x 16 B; up to three
  // 16-B intrinsic pieces) is issued before any of them is used, so the prologue costs
  // one L2/HBM round trip, not one per loop turn (E, NI <= kLdsCams = blockDim)
  if constexpr (!(VAR & 4)) {
    const int e = threadIdx.x;
    double2 xw[3];
    if (e < v.E) {
#pragma unroll
      for (int i = 0; i < 3; ++i) xw[i] = reinterpret_cast<const double2*>(ext + 6 * (size_t)e)[i];
    }
    double2 kq[3];
    if constexpr (KL) {
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int i = threadIdx.x + j * 1024;
        if (i < v.NI * 3) kq[j] = reinterpret_cast<const double2*>(v.intr + (size_t)kIntr * (i / 3))[i % 3];
      }
    }
    if (e < v.E) {
      const double x6[6] = {xw[0].x, xw[0].y, xw[1].x, xw[1].y, xw[2].x, xw[2].y};
      double T[30];
      if constexpr (VAR & 1) {
#pragma unroll
        for (int i = 0; i < 12; ++i) T[i] = (i % 4 == 0 ? 1.0 : 0.0) + (i >= 9 ? x6[i - 6] : 0.0);
      } else {
        cam_table(x6, T);
      }
#pragma unroll
      for (int i = 0; i < 6; ++i) reinterpret_cast<double2*>(rt_s + 12 * e)[i] = make_double2(T[2 * i], T[2 * i + 1]);
    }
    if constexpr (KL) {
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int i = threadIdx.x + j * 1024;
        if (i < v.NI * 3) reinterpret_cast<double2*>(k_s)[i] = kq[j];
      }
    }
  }
  __syncthreads();
  const LdsTabs<KL> tabs{rt_s, k_s, nullptr, v.intr};
  const LossK lk = loss_of(v);
  double acc[2] = {0.0, 0.0};
  for (int r = 0; r < rounds; ++r) {
    if (r > 0) {
      sl = (r * G + grp) * gridDim.x + blockIdx.x;
      off = len = 0;
      X[0] = X[1] = X[2] = 0.0;
      if (sl < v.nslice) {
        off = v.slice_off[sl];
        len = (v.slice_off[sl + 1] - off) >> 6;
        const int p = 64 * sl + lane;
        if (p < v.NP) {
          X[0] = points[3 * (size_t)p];
          X[1] = points[3 * (size_t)p + 1];
          X[2] = points[3 * (size_t)p + 2];
        }
      }
      rowq_fill<WPS, D>(v, off, len, w, lane, q);
    }
    double c[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) c[k] = 0.0;
    // the queue is walked in place (row k + d WPS sits in slot d of the current turn,
    // and the slot is refilled with the row D turns later), so no register holding a
    // load in flight is ever copied and each wait covers only the oldest row
#pragma unroll 1
    for (int k0 = w; k0 < len; k0 += D * WPS) {
#pragma unroll
      for (int d = 0; d < D; ++d) {
        const int k = k0 + d * WPS;
        if (k >= len) break;
        const int4 id = q.id[d];
        const double2 xy = q.xy[d];
        const int kn = k + D * WPS;
        if (kn < len) {
          q.id[d] = v.obs_idx[off + 64 * kn + lane];
          q.xy[d] = v.obs_xy[off + 64 * kn + lane];
        }
        // branch-free: padding slots (point -1; ext0 = intr = 0, ext1 = -1) are evaluated
        // and dropped by selects, so the row has no exec-mask branch around it
        const bool live = id.x >= 0;
        double ru, rv, jx0[3], jx1[3], rho = 0.0;
        if constexpr (VAR & 2) {
          ru = xy.x + id.y;
          rv = xy.y + id.w;
#pragma unroll
          for (int q = 0; q < 3; ++q) jx0[q] = jx1[q] = X[q];
        } else {
          obs_rows_l<LOSS, true, -1, COMP>(lk, rho, id, xy, X, tabs, ru, rv, jx0, jx1, nullptr, nullptr);
        }
        if (!live) ru = rv = jx0[0] = jx0[1] = jx0[2] = jx1[0] = jx1[1] = jx1[2] = 0.0;
        if constexpr (LOSS != DAB_LOSS_TRIVIAL) rho = live ? rho : 0.0;
        c[0] = fma(jx1[0], jx1[0], fma(jx0[0], jx0[0], c[0]));
        c[1] = fma(jx1[0], jx1[1], fma(jx0[0], jx0[1], c[1]));
        c[2] = fma(jx1[0], jx1[2], fma(jx0[0], jx0[2], c[2]));
        c[3] = fma(jx1[1], jx1[1], fma(jx0[1], jx0[1], c[3]));
        c[4] = fma(jx1[1], jx1[2], fma(jx0[1], jx0[2], c[4]));
        c[5] = fma(jx1[2], jx1[2], fma(jx0[2], jx0[2], c[5]));
        c[6] = fma(jx1[0], rv, fma(jx0[0], ru, c[6]));
        c[7] = fma(jx1[1], rv, fma(jx0[1], ru, c[7]));
        c[8] = fma(jx1[2], rv, fma(jx0[2], ru, c[8]));
        if constexpr (LOSS == DAB_LOSS_TRIVIAL) acc[0] = fma(rv, rv, fma(ru, ru, acc[0]));
        else acc[0] += rho;
        acc[1] += (isfinite(ru) && isfinite(rv)) ? 0.0 : 1.0;
      }
    }
    // waves 1.. of the group hand their sums to wave 0 (fixed order), PH components at a time
    if constexpr (WPS > 1 && !(VAR & 32)) {
#pragma unroll
      for (int ph = 0; ph < 9; ph += PH) {
        if (w > 0) {
#pragma unroll
          for (int k = 0; k < PH; ++k) sh[grp][w - 1][k][lane] = c[ph + k];
        }
        __syncthreads();
        if (w == 0) {
#pragma unroll
          for (int k = 0; k < PH; ++k) {
            double t = c[ph + k];
#pragma unroll
            for (int u = 0; u < WPS - 1; ++u) t += sh[grp][u][k][lane];
            c[ph + k] = t;
          }
        }
        __syncthreads();
      }
    }
    const int p = 64 * sl + lane;
    if (!(VAR & 16) && w == 0 && sl < v.nslice && p < v.NP) {
#pragma unroll
      for (int k = 0; k < 6; ++k) V[k * NPs + p] = c[k];
#pragma unroll
      for (int k = 0; k < 3; ++k) g[k * NPs + p] = c[6 + k];
    }
  }
  if constexpr (VAR & 8) store_cost_partial<16>(acc, partial);
  else if constexpr (VAR & 64) store_cost_partial_last<16>(acc, partial, arrivals, cost);
  else cost_fx_add<16>(acc, costfx);
}

template <int WPS, int D, int VAR = 0, int LOSS = DAB_LOSS_TRIVIAL>
static void launch_pf(hipStream_t s, const DevView& v, const double* points, const double* ext, double* V, double* g,
                      double* partial, unsigned* arrivals, double* cost, unsigned long long* costfx,
                      unsigned long long* fx_next, int grid) {
  // single-extrinsic problems: no second table, so the row queue can be 2 deeper
  if (!v.any_comp && v.NI <= kLdsCams)
    k_eval_points_pf<true, WPS, D + 2, VAR, false, LOSS>
        <<<grid, 1024, 0, s>>>(v, points, ext, V, g, partial, arrivals, cost, costfx, fx_next);
  else if (v.NI <= kLdsCams)
    k_eval_points_pf<true, WPS, D, VAR, true, LOSS><<<grid, 1024, 0, s>>>(v, points, ext, V, g, partial, arrivals, cost, costfx, fx_next);
  else
    k_eval_points_pf<false, WPS, D, VAR, true, LOSS><<<grid, 1024, 0, s>>>(v, points, ext, V, g, partial, arrivals, cost, costfx, fx_next);
}

// LDS variants (all <= 160 KiB): wps 0 = 4 waves/slice, K staged when NI <= 128;
// wps -1 = 1 wave/slice with every intrinsic staged (NI <= 1024); wps -2 = 2 waves/slice
template <int LOSS>
static void launch_eval_points_t(hipStream_t s, const DevView& v, const double* points, const double* ext,
                        const double* camtab, double* V, double* g, double* partial, unsigned* arrivals,
                        double* cost, unsigned long long* costfx, unsigned long long* fx_next, int grid,
                        int wps) {
  if (wps == 0 || wps == -2) {  // LDS tables built in-kernel; grid = persistent work-groups
    if (wps == 0) {
      if (v.NI <= 128) k_eval_points_lds<128, 4, false, LOSS><<<grid, 1024, 0, s>>>(v, points, ext, camtab, V, g, partial, arrivals, cost);
      else k_eval_points_lds<0, 4, false, LOSS><<<grid, 1024, 0, s>>>(v, points, ext, camtab, V, g, partial, arrivals, cost);
    } else {
      if (v.NI <= 128) k_eval_points_lds<128, 2, false, LOSS><<<grid, 1024, 0, s>>>(v, points, ext, camtab, V, g, partial, arrivals, cost);
      else k_eval_points_lds<0, 2, false, LOSS><<<grid, 1024, 0, s>>>(v, points, ext, camtab, V, g, partial, arrivals, cost);
    }
    return;
  }
  if (wps <= -100) {  // deep-prefetch variants: -(100 + 10 WPS + D + 1000 VAR)
    switch (-wps - 100) {
      case 12: launch_pf<1, 2, 0, LOSS>(s, v, points, ext, V, g, partial, arrivals, cost, costfx, fx_next, grid); break;
      case 13: launch_pf<1, 3, 0, LOSS>(s, v, points, ext, V, g, partial, arrivals, cost, costfx, fx_next, grid); break;
      case 23: launch_pf<2, 3, 0, LOSS>(s, v, points, ext, V, g, partial, arrivals, cost, costfx, fx_next, grid); break;
      case 64012: launch_pf<1, 2, 64, LOSS>(s, v, points, ext, V, g, partial, arrivals, cost, costfx, fx_next, grid); break;
      case 64022: launch_pf<2, 2, 64, LOSS>(s, v, points, ext, V, g, partial, arrivals, cost, costfx, fx_next, grid); break;
#ifdef DAB_ABLATIONS  // timing ablations (wrong results)
      case 2012: launch_pf<1, 2, 2>(s, v, points, ext, V, g, partial, arrivals, cost, costfx, fx_next, grid); break;
      case 4012: launch_pf<1, 2, 4>(s, v, points, ext, V, g, partial, arrivals, cost, costfx, fx_next, grid); break;
      case 1012: launch_pf<1, 2, 1>(s, v, points, ext, V, g, partial, arrivals, cost, costfx, fx_next, grid); break;
#endif
      default: launch_pf<2, 2, 0, LOSS>(s, v, points, ext, V, g, partial, arrivals, cost, costfx, fx_next, grid); break;
    }
    return;
  }
#ifdef DAB_ABLATIONS  // timing ablations (wrong results)
  if (wps == -5) {  // intrinsic index masked to the 128 staged in LDS
    k_eval_points_lds<128, 2, true><<<grid, 1024, 0, s>>>(v, points, ext, camtab, V, g, partial, arrivals, cost);
    return;
  }
  if (wps == 41 || wps == 42) {
    if (wps == 41) k_eval_points<4, 1><<<grid, 256, 0, s>>>(v, points, camtab, V, g, partial);
    else k_eval_points<4, 2><<<grid, 256, 0, s>>>(v, points, camtab, V, g, partial);
    launch_final_sum(s, grid, 2, partial, cost);
    return;
  }
#endif
  if (wps == 16) {
    k_eval_points<16, 0, LOSS><<<grid, 1024, 0, s>>>(v, points, camtab, V, g, partial);
  } else if (wps == 8) {
    k_eval_points<8, 0, LOSS><<<grid, 512, 0, s>>>(v, points, camtab, V, g, partial);
  } else {
    k_eval_points<4, 0, LOSS><<<grid, 256, 0, s>>>(v, points, camtab, V, g, partial);
  }
  launch_final_sum(s, grid, 2, partial, cost);
}
void launch_eval_points(hipStream_t s, const DevView& v, const double* points, const double* ext,
                        const double* camtab, double* V, double* g, double* partial, unsigned* arrivals,
                        double* cost, unsigned long long* costfx, unsigned long long* fx_next, int grid,
                        int wps) {
  DAB_LOSS_SWITCH(v.loss, launch_eval_points_t<LOSS>(s, v, points, ext, camtab, V, g, partial, arrivals, cost, costfx,
                                                     fx_next, grid, wps));
}
bool eval_points_needs_camtab(int wps) { return wps > 0; }

bool eval_points_lds_fits(int E) { return E <= kLdsCams; }

// parity API: every Jacobian column as planes Jfull[2*col+row][N]
__global__ __launch_bounds__(256) void k_jacobian_full(DevView v, const double* __restrict__ points,
                                                       const double* __restrict__ camtab,
                                                       double2* __restrict__ r, double* __restrict__ J) {
  const int N = v.N;
  const size_t Ns = (size_t)N;
  for (int s = blockIdx.x * blockDim.x + threadIdx.x; s < N; s += gridDim.x * blockDim.x) {
    const int4 id = v.obs_idx[s];
    if (id.x < 0) continue;  // padding slot
    const double X[3] = {points[3 * (size_t)id.x], points[3 * (size_t)id.x + 1], points[3 * (size_t)id.x + 2]};
    ObsJac o;
    obs_jacobian(id, v.obs_xy[s], X, camtab, v.intr, o);
    r[s] = make_double2(o.pr.ru, o.pr.rv);
    double* Jo = J + s;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      Jo[(2 * c) * Ns] = o.jx0[c];
      Jo[(2 * c + 1) * Ns] = o.jx1[c];
      Jo[(2 * (3 + c)) * Ns] = o.jw0a[c];
      Jo[(2 * (3 + c) + 1) * Ns] = o.jw0b[c];
      Jo[(2 * (6 + c)) * Ns] = o.pr.A0[c];
      Jo[(2 * (6 + c) + 1) * Ns] = o.pr.A1[c];
      Jo[(2 * (9 + c)) * Ns] = o.jw1a[c];
      Jo[(2 * (9 + c) + 1) * Ns] = o.jw1b[c];
      Jo[(2 * (12 + c)) * Ns] = o.jt1a[c];
      Jo[(2 * (12 + c) + 1) * Ns] = o.jt1b[c];
    }
  }
}

void launch_jacobian_full(hipStream_t s, const DevView& v, const double* points, const double* camtab,
                          double* r, double* Jfull) {
  if (v.N <= 0) return;
  k_jacobian_full<<<grid_for(v.N, 256, 1 << 20), 256, 0, s>>>(v, points, camtab,
                                                              reinterpret_cast<double2*>(r), Jfull);
}

// residual at a parameter state
__device__ __forceinline__ void residual_at(const DevView& v, const double* __restrict__ points,
                                            const double* __restrict__ camtab, int s, double& ru,
                                            double& rv) {
  const int4 id = v.obs_idx[s];
  const double2 xy = v.obs_xy[s];
  const double X[3] = {points[3 * (size_t)id.x], points[3 * (size_t)id.x + 1], points[3 * (size_t)id.x + 2]};
  const double* K = v.intr + (size_t)kIntr * id.w;
  double T0[12];
  load_tab<12>(camtab, id.y, T0);
  double P[3];
  if (id.z >= 0) {
    double T1[12], P2[3];
    load_tab<12>(camtab, id.z, T1);
    matvec_add(T1, X, T1 + 9, P2);
    matvec_add(T0, P2, T0 + 9, P);
  } else {
    matvec_add(T0, X, T0 + 9, P);
  }
  Proj pr;
  project(P, K, xy.x, xy.y, pr, false);
  ru = pr.ru;
  rv = pr.rv;
}

__global__ __launch_bounds__(256) void k_residual(DevView v, const double* __restrict__ points,
                                                  const double* __restrict__ camtab,
                                                  double2* __restrict__ rout,
                                                  double* __restrict__ partial) {
  double acc[2] = {0.0, 0.0};
  for (int s = blockIdx.x * blockDim.x + threadIdx.x; s < v.N; s += gridDim.x * blockDim.x) {
    if (v.obs_idx[s].x < 0) continue;  // padding slot
    double ru, rv;
    residual_at(v, points, camtab, s, ru, rv);
    if (rout) rout[s] = make_double2(ru, rv);
    acc[0] += ru * ru + rv * rv;
    acc[1] += (isfinite(ru) && isfinite(rv)) ? 0.0 : 1.0;
  }
  block_reduce_store<2>(acc, partial + 2 * (size_t)blockIdx.x);
}

void launch_residual(hipStream_t s, const DevView& v, const double* points, const double* camtab,
                     double* r_out, double* partial, int grid) {
  k_residual<<<grid, 256, 0, s>>>(v, points, camtab, reinterpret_cast<double2*>(r_out), partial);
}

// filterPoint3d (DeepArcManager.cc:332-424) masks, one SELL slice per 64-lane block:
// lane = point, its slots walked in order. keep(slot) = !(mse < eb); a point lives when
// one of its slots is kept and !(|X - c|^2 > radius/2); a dead point drops its slots.
__global__ __launch_bounds__(64) void k_filter(DevView v, const double* __restrict__ points,
                                               const double* __restrict__ camtab, double eb, double c0,
                                               double c1, double c2, double half_r,
                                               unsigned char* __restrict__ slot_keep,
                                               unsigned char* __restrict__ pt_keep) {
  const int sl = blockIdx.x, lane = threadIdx.x;
  const int p = 64 * sl + lane;
  const int off = v.slice_off[sl], len = (v.slice_off[sl + 1] - off) >> 6;
  bool alive = false;
  for (int k = 0; k < len; ++k) {
    const int s = off + 64 * k + lane;
    unsigned char keep = 0;
    if (v.obs_idx[s].x >= 0) {
      double ru, rv;
      residual_at(v, points, camtab, s, ru, rv);
      const double mse = (ru * ru + rv * rv) / 2.0;
      keep = (mse < eb) ? 0 : 1;
    }
    slot_keep[s] = keep;
    alive = alive || keep;
  }
  if (p >= v.NP) return;
  double d2 = 0.0;
  const double c[3] = {c0, c1, c2};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double d = points[3 * (size_t)p + i] - c[i];
    d2 += d * d;
  }
  alive = alive && !(d2 > half_r);
  pt_keep[p] = alive ? 1 : 0;
  if (!alive)
    for (int k = 0; k < len; ++k) slot_keep[off + 64 * k + lane] = 0;
}

void launch_filter(hipStream_t s, const DevView& v, const double* points, const double* camtab, double eb,
                   const double c[3], double radius, unsigned char* slot_keep, unsigned char* pt_keep) {
  if (v.nslice <= 0) return;
  k_filter<<<v.nslice, 64, 0, s>>>(v, points, camtab, eb, c[0], c[1], c[2], radius / 2, slot_keep, pt_keep);
}

// ------------------------------------------------------------------------------------
// camera-side J^T J / J^T r reductions, matrix-free (row a7)
// ------------------------------------------------------------------------------------
// One block per chunk of camera-major entry positions (one camera per chunk): the
// entry's observation is re-evaluated from its camera-major input copy (cm_idx, cm_xy,
// 32 B, contiguous) and its camera rows reduced into U (21 upper) | g_c (6).
// entries i0, i0 + stride, ... < e of one chunk (a block: i0 = b + threadIdx.x, stride =
// blockDim.x; one wave of the fused pass: i0 = b + lane, stride = 64)
// MakeTabs: a callable returning the table view, called after the first entry's loads
// are issued (the fused pass builds the camera table in SGPRs while they are in flight).
template <int LOSS = DAB_LOSS_TRIVIAL, class MakeTabs>
__device__ __forceinline__ void eval_cams_chunk_lazy(const DevView& v, int i0, int e, int stride,
                                                     const double* __restrict__ points, MakeTabs make_tabs,
                                                     double (&acc)[27]) {
  // software-pipelined: the next entry's inputs (and its point) load while this one computes
  int i = i0;
  int4 id_n = make_int4(0, 0, -1, 0);
  double2 xy_n = make_double2(0.0, 0.0);
  double X_n[3] = {0.0, 0.0, 0.0};
  if (i < e) {
    id_n = v.cm_idx[i];
    xy_n = v.cm_xy[i];
    X_n[0] = points[3 * (size_t)id_n.x];
    X_n[1] = points[3 * (size_t)id_n.x + 1];
    X_n[2] = points[3 * (size_t)id_n.x + 2];
  }
  const auto tabs = make_tabs();
  const LossK lk = loss_of(v);
  for (; i < e; i += stride) {
    int4 id = id_n;
    const double2 xy = xy_n;
    const double X[3] = {X_n[0], X_n[1], X_n[2]};
    const int in = i + stride;
    if (in < e) {
      id_n = v.cm_idx[in];
      xy_n = v.cm_xy[in];
      X_n[0] = points[3 * (size_t)id_n.x];
      X_n[1] = points[3 * (size_t)id_n.x + 1];
      X_n[2] = points[3 * (size_t)id_n.x + 2];
    }
    const bool slot1 = (id.w & kSlotBit) != 0;
    id.w &= ~kSlotBit;
    double ru, rv, ja[6], jb[6], rho;
    if (slot1) obs_rows_l<LOSS, false, 1>(lk, rho, id, xy, X, tabs, ru, rv, nullptr, nullptr, ja, jb);
    else obs_rows_l<LOSS, false, 0>(lk, rho, id, xy, X, tabs, ru, rv, nullptr, nullptr, ja, jb);
    int k = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int bb = a; bb < 6; ++bb) {
        acc[k] = fma(jb[a], jb[bb], fma(ja[a], ja[bb], acc[k]));
        ++k;
      }
#pragma unroll
    for (int a = 0; a < 6; ++a) acc[21 + a] = fma(jb[a], rv, fma(ja[a], ru, acc[21 + a]));
  }
}

template <int LOSS = DAB_LOSS_TRIVIAL, class Tabs>
__device__ __forceinline__ void eval_cams_chunk(const DevView& v, int i0, int e, int stride,
                                                const double* __restrict__ points, const Tabs& tabs,
                                                double (&acc)[27]) {
  eval_cams_chunk_lazy<LOSS>(v, i0, e, stride, points, [&]() -> const Tabs& { return tabs; }, acc);
}

// Uniform chunk, single-extrinsic observations (the fused pass's camera waves): entries
// i0, i0 + stride, ... < e with a three-slot software pipeline in static registers: while
// entry i computes, the point of entry i + stride is gathered (its index arrived one step
// earlier) and the index and pixel of entry i + 2 stride are loaded. The simple one-ahead
// pipeline waits for the next index right before every gather, i.e. one HBM latency per
// entry; here a wait only ever covers loads issued a full step earlier. Only the point
// index is read (cm_pt, 4 B, not the 16-B cm_idx record): the table is the chunk's.
template <int NS = 3, int LOSS = DAB_LOSS_TRIVIAL, class MakeTabs>
__device__ __forceinline__ void eval_cams_uni_pipe(const DevView& v, int i0, int e, int stride,
                                                   const double* __restrict__ points, MakeTabs make_tabs,
                                                   double (&acc)[27]) {
  // NS register slots: the index and pixel of entry i + (NS-1) stride are loaded and the
  // point of entry i + (NS-2) stride is gathered while entry i computes
  static_assert(NS >= 3, "at least three slots");
  const int* __restrict__ cm_pt = v.cm_pt;
  int pt[NS];
  double2 xy[NS];
  double X[NS][3];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    pt[s] = -1;
    xy[s] = make_double2(0.0, 0.0);
    X[s][0] = X[s][1] = X[s][2] = 0.0;
  }
#pragma unroll
  for (int s = 0; s < NS - 1; ++s)
    if (i0 + s * stride < e) {
      pt[s] = cm_pt[i0 + s * stride];
      xy[s] = v.cm_xy[i0 + s * stride];
    }
#pragma unroll
  for (int s = 0; s < NS - 2; ++s)
    if (pt[s] >= 0) {
#pragma unroll
      for (int q = 0; q < 3; ++q) X[s][q] = points[3 * (size_t)pt[s] + q];
    }
  const auto tabs = make_tabs();
  const LossK lk = loss_of(v);
  DAB_STAMP_ANY(1);
  for (int i = i0; i < e; i += NS * stride) {
#pragma unroll
    for (int u = 0; u < NS; ++u) {
      const int ii = i + u * stride;
      if (ii >= e) break;
      const int sg = (u + NS - 2) % NS, sl = (u + NS - 1) % NS;
      if (pt[sg] >= 0 && ii + (NS - 2) * stride < e) {
#pragma unroll
        for (int q = 0; q < 3; ++q) X[sg][q] = points[3 * (size_t)pt[sg] + q];
      }
      if (ii + (NS - 1) * stride < e) {
        pt[sl] = cm_pt[ii + (NS - 1) * stride];
        xy[sl] = v.cm_xy[ii + (NS - 1) * stride];
      }
      double ru, rv, ja[6], jb[6], rho;
      obs_rows_l<LOSS, false, 0, false>(lk, rho, make_int4(pt[u], 0, -1, 0), xy[u], X[u], tabs, ru, rv, nullptr,
                                        nullptr, ja, jb);
      int k = 0;
#pragma unroll
      for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int bb = a; bb < 6; ++bb) {
          acc[k] = fma(jb[a], jb[bb], fma(ja[a], ja[bb], acc[k]));
          ++k;
        }
#pragma unroll
      for (int a = 0; a < 6; ++a) acc[21 + a] = fma(jb[a], rv, fma(ja[a], ru, acc[21 + a]));
    }
  }
}



// Camera blocks accumulated in the point frame (the fused pass's camera waves). With
// Y = R X and J_l = R J_r (the left Jacobian), the rotation part of a row a (= dr/dP) is
//   -((a R) x X)^T J_r = (Y x a)^T J_l          (R (u x v) = R u x R v),
// so every row is w = [Y x a | a] times the per-camera constant blockdiag(J_l, I): the
// loop accumulates the 6 x 6 block and the 6-vector in w's basis (no J_r product per row:
// 118 fp64 instructions per entry instead of 154) and cam_frame_entry applies J_l once
// per camera, after the sums. The small-angle tables (R = I + [w]x, Rd = J_r = I) take
// Z = X in place of Y and J_l = I: the same rows as obs_rows, exactly.
struct UniFrame {
  double T[12];  // R | t
  double K[6];
  bool small;
  // from a frame shared in LDS (k_eval_bal: R t K J_l small, kBalFrame doubles), every
  // lane reading the same address (broadcast), then held in SGPRs
  struct FromShared {};
  __device__ __forceinline__ UniFrame(FromShared, const double* fr) {
#pragma unroll
    for (int q = 0; q < 12; ++q) T[q] = UniTabs::uniform(fr[q]);
#pragma unroll
    for (int q = 0; q < 6; ++q) K[q] = UniTabs::uniform(fr[12 + q]);
    small = UniTabs::uniform(fr[27]) != 0.0;
  }
};

template <int LOSS = DAB_LOSS_TRIVIAL>
__device__ __forceinline__ void frame_rows_acc(const double2 xy, const double (&X)[3], const UniFrame& f,
                                               double (&acc)[27], const LossK& lk = LossK{}) {
  const double* R = f.T;
  double Y[3], P[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    Y[r] = R[3 * r] * X[0] + R[3 * r + 1] * X[1] + R[3 * r + 2] * X[2];
    P[r] = Y[r] + f.T[9 + r];
  }
  // a wave-uniform select (two loop copies, one per case, would spill)
  double Z[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) Z[r] = f.small ? X[r] : Y[r];
  Proj pr;
  project<LOSS>(P, f.K, xy.x, xy.y, pr, true, lk);  // rows linear in A, r: scaled here, J_l after the sums
  // one row at a time (the row's 6 values are all that is live beside the sums); the
  // per-element order is the two-row fma(b, b, fma(a, a, acc)) of obs_rows' callers
#pragma unroll
  for (int row = 0; row < 2; ++row) {
    const double* A = row == 0 ? pr.A0 : pr.A1;
    const double r = row == 0 ? pr.ru : pr.rv;
    double j[6];
    j[0] = Z[1] * A[2] - Z[2] * A[1];
    j[1] = Z[2] * A[0] - Z[0] * A[2];
    j[2] = Z[0] * A[1] - Z[1] * A[0];
#pragma unroll
    for (int i = 0; i < 3; ++i) j[3 + i] = A[i];
    int k = 0;
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int bb = a; bb < 6; ++bb) {
        acc[k] = fma(j[a], j[bb], acc[k]);
        ++k;
      }
#pragma unroll
    for (int a = 0; a < 6; ++a) acc[21 + a] = fma(j[a], r, acc[21 + a]);
  }
}

// The fused pass's camera loop, gathering the points itself (no camera-major copy to refresh
// when the points move). Three register slots per ring; per 64-entry step the point index is
// loaded four steps ahead and the point (with the pixel) gathered two steps ahead, so the
// index -> gather -> compute chain has two steps of arithmetic to hide each hop. Every load is
// unconditional (clamped to the last entry; the step count is wave-uniform), so the waits the
// compiler places count exactly: the gather of step st + 2 waits only for its index, the
// compute of step st only for its point. The camera's frame comes from the caller
// (get_frame(), called once the first indices and gathers are in flight: k_eval_bal's frames
// shared in LDS).
template <int LOSS = DAB_LOSS_TRIVIAL, class GetFrame>
__device__ __forceinline__ void eval_cams_gather_f(const int* __restrict__ cm_pt, const double2* __restrict__ cmxy,
                                                   const double* __restrict__ points, int i0, int e,
                                                   double (&acc)[27], GetFrame get_frame,
                                                   const LossK& lk = LossK{}) {
  constexpr int DG = 2, DI = 4, R = 3;
  const int lo = i0 - (int)(threadIdx.x & 63);
  const int n = (e - lo + 63) >> 6;  // steps of 64 entries
  int pid[R];
  double2 xy[R];
  double X[R][3];
  auto load_idx = [&](int slot, int step) { pid[slot] = cm_pt[min(i0 + 64 * step, e - 1)]; };
  auto gather = [&](int islot, int slot, int step) {
    const int p = pid[islot];
    xy[slot] = cmxy[min(i0 + 64 * step, e - 1)];
#pragma unroll
    for (int q = 0; q < 3; ++q) X[slot][q] = points[3 * (size_t)p + q];
  };
  DAB_STAMP_HOP(4);  // the chunk bounds are here
  if (n > 0) {
#pragma unroll
    for (int st = 0; st < DG; ++st) load_idx(st % R, st);
    DAB_STAMP_HOP(5);  // the first indices are here
#pragma unroll
    for (int st = 0; st < DG; ++st) gather(st % R, st % R, st);
#pragma unroll
    for (int st = DG; st < DI; ++st) load_idx(st % R, st);
  }
  DAB_STAMP_HOP(6);  // the first points are here
  const UniFrame f = get_frame();
  for (int st0 = 0; st0 < n; st0 += R) {
#pragma unroll
    for (int u = 0; u < R; ++u) {
      const int st = st0 + u;
      gather((st + DG) % R, (st + DG) % R, st + DG);
      load_idx((st + DI) % R, st + DI);
      if (i0 + 64 * st < e) frame_rows_acc<LOSS>(xy[u], X[u], f, acc, lk);
    }
  }
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

// General entries (int4 index records, the rig's camera-major and pair-major copies): the
// same three-slot register pipeline as eval_cams_uni_pipe — while entry i computes, the
// point of entry i + stride is gathered and the record of entry i + 2 stride loaded —
// around a per-entry body(id, xy, X).
template <class Body>
__device__ __forceinline__ void pipe_entries(const int4* __restrict__ idx, const double2* __restrict__ xyv, int i0,
                                             int e, int stride, const double* __restrict__ points, Body body) {
  int4 id[3];
  double2 xy[3];
  double X[3][3];
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    id[s] = make_int4(-1, 0, -1, 0);
    xy[s] = make_double2(0.0, 0.0);
    X[s][0] = X[s][1] = X[s][2] = 0.0;
  }
#pragma unroll
  for (int s = 0; s < 2; ++s)
    if (i0 + s * stride < e) {
      id[s] = idx[i0 + s * stride];
      xy[s] = xyv[i0 + s * stride];
    }
  if (id[0].x >= 0) {
#pragma unroll
    for (int q = 0; q < 3; ++q) X[0][q] = points[3 * (size_t)id[0].x + q];
  }
  for (int i = i0; i < e; i += 3 * stride) {
#pragma unroll
    for (int u = 0; u < 3; ++u) {
      const int ii = i + u * stride;
      if (ii >= e) break;
      const int sg = (u + 1) % 3, sl = (u + 2) % 3;
      if (id[sg].x >= 0 && ii + stride < e) {
#pragma unroll
        for (int q = 0; q < 3; ++q) X[sg][q] = points[3 * (size_t)id[sg].x + q];
      }
      if (ii + 2 * stride < e) {
        id[sl] = idx[ii + 2 * stride];
        xy[sl] = xyv[ii + 2 * stride];
      }
      body(id[u], xy[u], X[u]);
    }
  }
}

// J_l (row-major) and the small-angle flag of extrinsic e from the global tables
__device__ __forceinline__ void ext_frame(const double* __restrict__ camtab, int e, double* jl, int k, bool& small) {
  const double* T = camtab + (size_t)kCamTab * e;
  small = T[12] == 1.0 && T[13] == 0.0 && T[14] == 0.0 && T[15] == 0.0 && T[16] == 1.0 && T[17] == 0.0 &&
          T[18] == 0.0 && T[19] == 0.0 && T[20] == 1.0;
  if (k < 9) {
    const int r = k / 3, c = k - 3 * r;
    jl[k] = T[12 + 3 * r] * T[21 + c] + T[12 + 3 * r + 1] * T[24 + c] + T[12 + 3 * r + 2] * T[27 + c];
  }
}

// pipe_entries with NS register slots: the record of entry i + (NS-1) stride is loaded and
// the point of entry i + (NS-2) stride gathered while entry i computes (kernels with
// registers to spare and few waves per SIMD, e.g. k_eval_pair)
template <int NS, class Body>
__device__ __forceinline__ void pipe_entries_ns(const int4* __restrict__ idx, const double2* __restrict__ xyv,
                                                int i0, int e, int stride, const double* __restrict__ points,
                                                Body body) {
  static_assert(NS >= 3, "at least three slots");
  int4 id[NS];
  double2 xy[NS];
  double X[NS][3];
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    id[s] = make_int4(-1, 0, -1, 0);
    xy[s] = make_double2(0.0, 0.0);
    X[s][0] = X[s][1] = X[s][2] = 0.0;
  }
#pragma unroll
  for (int s = 0; s < NS - 1; ++s)
    if (i0 + s * stride < e) {
      id[s] = idx[i0 + s * stride];
      xy[s] = xyv[i0 + s * stride];
    }
#pragma unroll
  for (int s = 0; s < NS - 2; ++s)
    if (id[s].x >= 0) {
#pragma unroll
      for (int q = 0; q < 3; ++q) X[s][q] = points[3 * (size_t)id[s].x + q];
    }
  for (int i = i0; i < e; i += NS * stride) {
#pragma unroll
    for (int u = 0; u < NS; ++u) {
      const int ii = i + u * stride;
      if (ii >= e) break;
      const int sg = (u + NS - 2) % NS, sl = (u + NS - 1) % NS;
      if (id[sg].x >= 0 && ii + (NS - 2) * stride < e) {
#pragma unroll
        for (int q = 0; q < 3; ++q) X[sg][q] = points[3 * (size_t)id[sg].x + q];
      }
      if (ii + (NS - 1) * stride < e) {
        id[sl] = idx[ii + (NS - 1) * stride];
        xy[sl] = xyv[ii + (NS - 1) * stride];
      }
      body(id[u], xy[u], X[u]);
    }
  }
}

// pipe_entries_ns with a uniform trip count: every lane of the block runs ceil((e - b) /
// stride) iterations, a lane past the end on the clamped last entry with valid = false (its
// body must add nothing). Every load is unconditional, so the memory counters the compiler
// tracks stay exact across the unrolled slots and a body waits only for its own slot's
// loads. With the guarded loads of pipe_entries_ns the compiler could not count what was
// outstanding on every path and waited for all of it (vmcnt(0)) before each body: the
// prefetch of the next slots never overlapped the arithmetic.
// NS register slots: the record of entry k + NS - 1 is loaded, then the point of entry
// k + GD gathered (its record loaded NS - 1 - GD iterations earlier), then entry k computed;
// with GD <= NS - 3 each load has at least two bodies of arithmetic to arrive in.
template <int NS, int GD, class Body>
__device__ __forceinline__ void pipe_entries_uni(const int4* __restrict__ idx, const double2* __restrict__ xyv,
                                                 int b, int e, int lane, int stride,
                                                 const double* __restrict__ points, Body body) {
  static_assert(NS >= 3 && GD >= 1 && GD <= NS - 2, "slot distances");
  constexpr int RD = NS - 1;
  const int niter = (e - b + stride - 1) / stride;
  const int last = e - 1;
  int4 id[NS];
  double2 xy[NS];
  double X[NS][3];
#pragma unroll
  for (int s = 0; s < RD; ++s) {
    const int i = min(b + lane + s * stride, last);
    id[s] = idx[i];
    xy[s] = xyv[i];
  }
#pragma unroll
  for (int s = 0; s < GD; ++s)
#pragma unroll
    for (int q = 0; q < 3; ++q) X[s][q] = points[3 * (size_t)max(id[s].x, 0) + q];
  for (int k = 0; k < niter; k += NS) {
#pragma unroll
    for (int u = 0; u < NS; ++u) {
      const int kk = k + u;
      const int sl = (u + RD) % NS, sg = (u + GD) % NS;
      {
        const int i = min(b + lane + (kk + RD) * stride, last);
        id[sl] = idx[i];
        xy[sl] = xyv[i];
      }
#pragma unroll
      for (int q = 0; q < 3; ++q) X[sg][q] = points[3 * (size_t)max(id[sg].x, 0) + q];
      if (kk < niter) body(id[u], xy[u], X[u], b + lane + kk * stride <= last);
    }
  }
}

// UNI: the chunks of `list` are uniform (chunk_uni), tables read once per block
template <bool UNI, int LOSS = DAB_LOSS_TRIVIAL>
__global__ __launch_bounds__(256) void k_eval_cams(DevView v, const int* __restrict__ chunk_beg,
                                                   const int* __restrict__ list,
                                                   const double* __restrict__ points,
                                                   const double* __restrict__ ext,
                                                   const double* __restrict__ camtab,
                                                   double* __restrict__ partial) {
  const int c = list ? list[blockIdx.x] : blockIdx.x;
  const int b = chunk_beg[c], e = chunk_beg[c + 1];
  double acc[27];
#pragma unroll
  for (int i = 0; i < 27; ++i) acc[i] = 0.0;
  if constexpr (UNI) {
    const int2 u = v.chunk_uni[c];
    eval_cams_uni_pipe<3, LOSS>(v, b + threadIdx.x, e, blockDim.x, points,
                                [&]() { return UniTabs(ext, v.intr, u.x, u.y); }, acc);
  } else if (small_tabs_fit(v.E, v.NI)) {
    extern __shared__ double tabs_lds[];
    eval_cams_chunk<LOSS>(v, b + threadIdx.x, e, blockDim.x, points,
                          stage_small_tabs(tabs_lds, v.E, v.NI, camtab, v.intr), acc);
  } else {
    eval_cams_chunk<LOSS>(v, b + threadIdx.x, e, blockDim.x, points, GlobalTabs{camtab, v.intr}, acc);
  }
  // per-wave transposed sums (wave_sums_transposed), then the waves in order
  __shared__ double wsum[kRedBlock / 64][27];
  wave_sums_transposed<27>(acc, wsum[threadIdx.x >> 6]);
  __syncthreads();
  if (threadIdx.x < 27) {
    double t = wsum[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kRedBlock / 64; ++w) t += wsum[w][threadIdx.x];
    partial[27 * (size_t)c + threadIdx.x] = t;
  }
}

void launch_eval_cams(hipStream_t s, const DevView& v, const ChunkLists& cl, const int* chunk_beg,
                      const double* points, const double* ext, const double* camtab, double* partial) {
  if (cl.nuni > 0)
    DAB_LOSS_SWITCH(v.loss, k_eval_cams<true, LOSS><<<cl.nuni, 256, 0, s>>>(
                                v, chunk_beg, cl.nuni == cl.nchunk ? nullptr : cl.uni, points, ext, camtab, partial));
  if (cl.ngen > 0) {
    const size_t lds = small_tabs_fit(v.E, v.NI) ? small_tabs_bytes(v.E, v.NI) : 0;
    DAB_LOSS_SWITCH(v.loss, k_eval_cams<false, LOSS><<<cl.ngen, 256, lds, s>>>(
                                v, chunk_beg, cl.ngen == cl.nchunk ? nullptr : cl.gen, points, ext, camtab, partial));
  }
}

// ------------------------------------------------------------------------------------
// k_eval_bal: the fused evaluation pass (BAL-shaped problems), both traversal orders in ONE
// launch, camera-side and point-side waves side by side on every CU
// ------------------------------------------------------------------------------------
// Why fused: the camera side is fp64-VALU heavy and the point side latency bound, but as two
// kernels they cannot overlap: a 1024-thread work-group at 128 VGPRs fills a CU's register
// file. Here waves 0..kBalPW-1 of each work-group run the point side (SELL slices, lane =
// point, a 3-deep row queue of packed 4-B records, R,t and K in LDS) and the other waves the
// camera side (wpc waves per free camera, each a part of its uniform chunk, the frame in
// SGPRs, blocks accumulated in the point frame), so one side's arithmetic fills the other's
// memory stalls. Every reduction keeps a fixed order: a camera's parts are combined (row sums
// in LDS) by whichever of its waves arrives last, in part order; the point waves' cost
// partials are summed by the last point wave in wave order and added as fixed-point integers
// (cost_fx_commit). V, g are bitwise those of the two-kernel pass; U, g_c are regrouped sums
// (equal to rounding); every run is bitwise the same.
//  * the camera waves' frames (R, t, K, J_l of the work-group's own cameras, at most 8) are
//    built by one lane per camera of the first camera wave and shared through LDS; each
//    camera wave waits for them only after its first index and point gathers are in flight
//    (eval_cams_gather_f), so there is no per-wave frame trigonometry;
//  * the point waves alone build R,t of every extrinsic into LDS (both of a thread's
//    extrinsics loaded before either table is built) and meet at an LDS-counter barrier of
//    their own before their rows; the camera waves never wait for the point tables.
// Round 5 (`profiles/r05_*`): this kernel replaced k_eval_fused (round 4; every camera wave
// built its own frame, the point tables in a load -> table loop), whose two trigonometry
// phases were a third of its VALU stream (6.61 M VALU per C3 launch, `r05_eval_fused_mix.txt`).
// C3 launch 25.3 -> 22.4 us, C2 9.9 -> 9.2 us on the same boxes (`scripts/eval_ab.py`).
// Ablations (`DAB_EVAL_SIDE`, timing only, wrong results): the point tables were 4.4 us of the
// critical path with the loop (r05l), 1.6 us with the loads issued first (r05m).
// Measured and dropped (same boxes): the camera waves on the older hardware waves 0-7
// (26.0 against 22.4 us); the larger camera parts on the SIMDs with the lighter point waves
// (22.4-23.8 against 22.3 us); R,t built ONCE per XCD inside the launch — 64-extrinsic chunks
// claimed from a per-XCD counter, published into the XCD's L2, consumed with sc1 loads after
// a done count (`scripts/experiments/eval_bal_xcd_tables.patch`; correct, 32 against 23.5 us:
// the hand-off's device-scope round trips put the tables at 10 us).
// Requirements (fused_eval_fits): every observation single-extrinsic, one uniform chunk per
// free camera, E, NI <= kLdsCams, NC <= (camera waves / 2) x grid.
constexpr int kBalPW = 8;              // point waves per work-group
constexpr int kBalCW = 16 - kBalPW;    // camera waves
constexpr int kBalFrame = 28;          // doubles per shared camera frame: R t K J_l small
// first part of a two-part camera chunk, in 1/1024: the older waves (part 0) get more, since
// the SIMDs' oldest-first issue starves the younger ones (round 3's per-wave timeline: 688 for
// k_eval_fused; re-swept for k_eval_bal in round 5, scripts/runs/r05aq.sh: 840 at 21.8 us against
// 22.0-22.3 us for 600-780 and 900-960, interleaved repetitions on one box)
constexpr int kCamSplit = 840;
bool fused_eval_fits(const DevView& v, int nchunk, int ngen, int ncross, int grid) {
  return !v.any_comp && ncross == 0 && ngen == 0 && nchunk == v.NC && v.NC > 0 && v.E <= kLdsCams &&
         v.NI <= kLdsCams && v.NC <= (kBalCW / 2) * grid;
}
// waves per camera: as many as still give every camera a slot in one round (small camera
// sets split each chunk finer: C2's 99 cameras take 8 waves each, C3's 999 take 2)
static int fused_wpc(int NC, int grid) {
  int w = kBalCW;
  while (w > 2 && (long long)NC * w > (long long)kBalCW * grid) w >>= 1;
  return w;
}
// point waves per slice: more when the slices are few (every slice in one round), if the
// per-part sums fit in rt_s beside the tables
static int fused_wps(int nslice, int E, int grid) {
  int w = kBalPW;
  const int used = (12 * E + 1) & ~1, cap = kLdsCams * 12;
  while (w > 1 && ((long long)nslice * w > (long long)kBalPW * grid || used + kBalPW * 9 * 64 > cap)) w >>= 1;
  return w;
}
// spin on a work-group word until it reaches `want`, bounded by an iteration count (~2^20
// sleeps, a fraction of a second; then the error words get `code` and the wave goes on, its
// results void: the pass fails closed). err: the handle's sticky word (dab_sync); errfx: the
// pass's cost set (word kFxErr), all-reduced with the cost so that every rank fails together
__device__ __forceinline__ void lds_wait_ge(const unsigned* w, unsigned want, unsigned* err,
                                            unsigned long long* errfx, unsigned code) {
  for (unsigned n = 0; __hip_atomic_load(w, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < want; ++n) {
    __builtin_amdgcn_s_sleep(1);
    if (n > (1u << 20)) {
      __hip_atomic_fetch_or(err, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_or(errfx + kFxErr, (unsigned long long)code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return;
    }
  }
}
// WPC_, WPS_ > 0: the waves per camera and per slice as compile-time constants (C3: 2, 1;
// C2: 8, 8), 0: the run-time wpc_rt, wps_rt. Round 6: the constants fold the part cuts'
// divisions, the part-combine and slice-part loops and the slot arithmetic — C2 9.29 ->
// 8.44 us per launch, C3 unchanged, bitwise the same sums (profiles/r06zk_*)
template <int WPC_, int WPS_, int LOSS = DAB_LOSS_TRIVIAL>
__global__ __launch_bounds__(1024) void k_eval_bal(DevView v, const int* __restrict__ chunk_beg,
                                                   const double* __restrict__ points, const double* __restrict__ ext,
                                                   const double* __restrict__ camtab, double* __restrict__ V,
                                                   double* __restrict__ g, double* __restrict__ ug,
                                                   unsigned long long* __restrict__ costfx,
                                                   unsigned long long* __restrict__ fx_next, unsigned* __restrict__ err,
                                                   int wpc_rt, int wps_rt, int side) {
  const int wpc = WPC_ > 0 ? WPC_ : wpc_rt, wps = WPS_ > 0 ? WPS_ : wps_rt;
  const LossK lk = loss_of(v);
  __shared__ double rt_s[kLdsCams * 12];
  __shared__ double k_s[kLdsCams * 6];
  __shared__ double csum[kBalCW][27];            // camera waves' sums: [slot * wpc + part]
  __shared__ double cfr[kBalCW / 2][kBalFrame];  // the work-group's camera frames, by slot
  __shared__ double shp[kBalPW][2];
  __shared__ unsigned ccount[kBalCW + kBalPW], tbar, kbar, pdone;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  DAB_TRACE_INIT();
  DAB_STAMP(0);
  // camera slot -> camera: slot s of work-group b takes camera s G + (G - 1 - b), so that the
  // work-groups short of a camera are the ones with an extra point slice (slices are dealt
  // from work-group 0 up), and a small camera set leaves the point side's work-groups alone
  auto cam_of = [&](int slot) { return slot * (int)gridDim.x + ((int)gridDim.x - 1 - (int)blockIdx.x); };
  const int nsl = kBalCW / wpc;
  if (threadIdx.x < kBalCW + kBalPW) ccount[threadIdx.x] = 0u;
  if (threadIdx.x == 0) tbar = kbar = pdone = 0u;
  if (blockIdx.x == 0 && fx_next)
    for (int i = threadIdx.x; i < kFxWords; i += blockDim.x) fx_next[i] = 0ull;
  __syncthreads();
  DAB_STAMP(7);  // past the work-group's first barrier
  // the frames of the work-group's cameras, one lane per camera slot (wave kBalPW), shared
  // through LDS; the camera waves wait only for these
  auto build_frames = [&]() {
    const int c = cam_of(lane);
    if (lane < nsl && c < v.NC) {
      // the (ext, intr) of the camera's chunk: computed when the map is affine (the usual
      // BAL numbering), which takes one dependent load off the frames' start
      const int2 u = v.uni_affine ? make_int2(c + v.uni_ox, c + v.uni_oi) : v.chunk_uni[c];
      double k6[6];  // the intrinsic leaves with the extrinsic (one round trip for both)
#pragma unroll
      for (int q = 0; q < 6; ++q) k6[q] = v.intr[(size_t)kIntr * u.y + q];
      double F[30];
      if (camtab) {
#pragma unroll
        for (int q = 0; q < 30; ++q) F[q] = camtab[(size_t)kCamTab * u.x + q];
      } else {
        double x6[6];
#pragma unroll
        for (int q = 0; q < 6; ++q) x6[q] = ext[6 * (size_t)u.x + q];
        cam_table(x6, F);
      }
      double* o = cfr[lane];
#pragma unroll
      for (int q = 0; q < 12; ++q) o[q] = F[q];
#pragma unroll
      for (int q = 0; q < 6; ++q) o[12 + q] = k6[q];
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int cc = 0; cc < 3; ++cc)
          o[18 + 3 * r + cc] = F[12 + 3 * r] * F[21 + cc] + F[12 + 3 * r + 1] * F[24 + cc] + F[12 + 3 * r + 2] * F[27 + cc];
      // cam_table's branch (its small-angle Rd is exactly I, R never is otherwise)
      o[27] = (F[12] == 1.0 && F[13] == 0.0 && F[14] == 0.0 && F[15] == 0.0 && F[16] == 1.0 && F[17] == 0.0 &&
               F[18] == 0.0 && F[19] == 0.0 && F[20] == 1.0 && F[21] == 1.0 && F[25] == 1.0 && F[29] == 1.0)
                  ? 1.0
                  : 0.0;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (lane == 0) __hip_atomic_store(&tbar, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
  };

  // what this launch runs (the split schedule's point-side launch builds no camera frames, its
  // camera-side launch no point tables and no intrinsic DMA); the timing ablations 3..6 exist
  // only in -DDAB_ABLATIONS builds
  const bool test_timeout = (side & kSideTestTimeout) != 0;
  side &= ~kSideTestTimeout;
#ifdef DAB_ABLATIONS
  const bool abl_tables_only = side == 3, abl_no_tabs = side == 4 || side == 5, abl_no_frames = side == 4 || side == 6;
#else
  constexpr bool abl_tables_only = false, abl_no_tabs = false, abl_no_frames = false;
#endif
  if (wave >= kBalPW) {
    // ---------------- camera side ----------------
    if (side == kSidePoints || abl_tables_only) {
      DAB_STAMP(3);
      return;
    }
    const int cw = wave - kBalPW, part = cw / nsl, slot = cw - part * nsl;
    const int c = cam_of(slot);  // one round (fused_eval_fits / fused_wpc)
    if (cw == 0 && !abl_no_frames) build_frames();
    if (c >= v.NC) {
      DAB_STAMP(3);
      return;
    }
    const int b = chunk_beg[c], e = chunk_beg[c + 1];
    auto cut = [&](int q) -> int {
      if (wpc == 2 && q == 1) return b + (int)(((long long)(e - b) * kCamSplit) >> 10);
      return b + (int)(((long long)(e - b) * q) / wpc);
    };
    const int lo = cut(part), hi = cut(part + 1);
    double acc[27];
#pragma unroll
    for (int i = 0; i < 27; ++i) acc[i] = 0.0;
    const double* fr = cfr[slot];
    eval_cams_gather_f<LOSS>(v.cm_pt, v.cm_xy, points, lo + lane, hi, acc, [&]() {
      // the frames, built while the first gathers fly (kSideTestTimeout, a test: a frame flag
      // that never comes — the wait must run out and fail the pass closed)
      if (!abl_no_frames) lds_wait_ge(&tbar, test_timeout ? 2u : 1u, err, costfx, 1u);
      const UniFrame f(UniFrame::FromShared{}, fr);
      DAB_STAMP(1);
      return f;
    }, lk);
    DAB_STAMP(2);
    wave_sums_transposed<27>(acc, csum[slot * wpc + part]);
    unsigned old = 0;
    if (lane == 0) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      old = __hip_atomic_fetch_add(&ccount[slot], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    old = __builtin_amdgcn_readfirstlane(old);
    if (old != (unsigned)wpc - 1) {  // another part is still running: the last one writes the row
      DAB_STAMP(3);
      return;
    }
    double* cs = csum[slot * wpc];
    if (lane < 27) {
      double t = cs[lane];
      for (int q = 1; q < wpc; ++q) t += csum[slot * wpc + q][lane];
      cs[lane] = t;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (lane < 27) ug[27 * (size_t)c + lane] = cam_frame_entry(cs, fr + 18, lane);
    DAB_STAMP(3);
    return;
  }

  // ---------------- point side ----------------
  if (side == kSideCams) {  // the split schedule's camera-side launch: nothing for the point waves
    DAB_STAMP(3);
    return;
  }
  // a work-group with no slice in any round (slot 0 of round 0 holds its lowest slice, b):
  // no tables, no rows, nothing to add (small problems: C2's camera work-groups, whose camera
  // waves then have the CU's issue and memory path to themselves)
  if ((int)blockIdx.x >= v.nslice) {
    DAB_STAMP(3);
    return;
  }
  const size_t NPs = (size_t)v.NP;
  const int pw = wave, pslots = kBalPW / wps, slot = pw / wps, part = pw - slot * wps;
  const int rounds = abl_tables_only ? 0 : (v.nslice + pslots * gridDim.x - 1) / (pslots * gridDim.x);
  constexpr int D = 3;
  int qe[D];      // packed records (ext | intr << 16, -1 = padding)
  double2 qxy[D];
  double X[3] = {0.0, 0.0, 0.0};
  int sl = slot * gridDim.x + blockIdx.x, off = 0, len = 0;
  // every load of a round's set-up is unconditional (clamped to valid addresses; a lane
  // past the points or a wave past the slices computes nothing from what it read), so the
  // row queue's waits count exactly
  auto setup_round = [&]() {
    const bool has = sl < v.nslice;
    const int slc = min(sl, v.nslice - 1);
    const int o0 = v.slice_off[slc], o1 = v.slice_off[slc + 1];
    off = has ? o0 : 0;
    len = has ? (o1 - o0) >> 6 : 0;
    const int p = min(64 * slc + lane, v.NP - 1);
    X[0] = points[3 * (size_t)p];
    X[1] = points[3 * (size_t)p + 1];
    X[2] = points[3 * (size_t)p + 2];
#pragma unroll
    for (int d = 0; d < D; ++d) {
      const int kk = max(0, min(part + d * wps, len - 1));
      qe[d] = v.obs_e[off + 64 * kk + lane];
      qxy[d] = v.obs_xy[off + 64 * kk + lane];
    }
  };
  // this thread's extrinsics (E <= kLdsCams = 2 x 512: at most two) leave first, so that one
  // load latency covers both tables (a loop of load -> table, twice, paid it twice: 4.4 us of
  // a C3 launch went to the point tables, r05l)
  constexpr int kTabPer = (kLdsCams + kBalPW * 64 - 1) / (kBalPW * 64);
  double xr[kTabPer][12];  // camtab: R,t as they are; else the 6 parameters
  const bool tabs_now = !abl_no_tabs;
  if (tabs_now) {
#pragma unroll
    for (int j = 0; j < kTabPer; ++j) {
      const int e = min(pw * 64 + lane + j * kBalPW * 64, v.E - 1);
      if (camtab) {
#pragma unroll
        for (int q = 0; q < 12; ++q) xr[j][q] = camtab[(size_t)kCamTab * e + q];
      } else {
#pragma unroll
        for (int q = 0; q < 6; ++q) xr[j][q] = ext[6 * (size_t)e + q];
      }
    }
  }
  // K of every intrinsic by LDS-DMA (no registers), each CU of an XCD starting at its own
  // 1/32 of the array, before the first rows' loads
  {
    const unsigned xrot = blockIdx.x >> 3;
    const int npiece = 3 * v.NI, nch = (npiece + 63) >> 6;
    const int rot = (int)((xrot * (unsigned)nch) >> 5);
    for (int j = pw; j < nch; j += kBalPW) {
      int jr = j + rot;
      if (jr >= nch) jr -= nch;
      const int i = min(jr * 64 + lane, npiece - 1);
      __builtin_amdgcn_global_load_lds(v.intr + (size_t)kIntr * (i / 3) + 2 * (i % 3), k_s + 2 * (size_t)(jr * 64), 16,
                                       0, 0);
    }
  }
  if (rounds > 0) setup_round();
  // R, t of every extrinsic (R,t only: the rest of cam_table folds away)
  if (tabs_now) {
#pragma unroll
    for (int j = 0; j < kTabPer; ++j) {
      const int e = pw * 64 + lane + j * kBalPW * 64;
      if (e >= v.E) break;
      double T[30];
      if (camtab) {
#pragma unroll
        for (int q = 0; q < 12; ++q) T[q] = xr[j][q];
      } else {
        cam_table(xr[j], T);
      }
#pragma unroll
      for (int i = 0; i < 6; ++i) reinterpret_cast<double2*>(rt_s + 12 * e)[i] = make_double2(T[2 * i], T[2 * i + 1]);
    }
  }
  DAB_STAMP_ANY(5);  // this wave's tables are built
  // barrier of the point waves only (LDS counter): own LDS writes and the K LDS-DMA retired
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  if (lane == 0) __hip_atomic_fetch_add(&kbar, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
  lds_wait_ge(&kbar, (unsigned)kBalPW, err, costfx, 1u);
  DAB_STAMP(1);
  if (abl_tables_only) return;
  const LdsTabs<true, false> tabs{rt_s, k_s, nullptr, v.intr};
  double acc[2] = {0.0, 0.0};
  for (int r = 0; r < rounds; ++r) {
    if (r > 0) {
      sl = (r * pslots + slot) * gridDim.x + blockIdx.x;
      setup_round();
    }
    double c[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) c[k] = 0.0;
#pragma unroll 1
    for (int k0 = part; k0 < len; k0 += D * wps) {
#pragma unroll
      for (int d = 0; d < D; ++d) {
        const int k = k0 + d * wps;
        const int pk = qe[d], pe = pk >= 0 ? pk : 0;
        const int4 id = make_int4(pk >= 0 ? 0 : -1, pe & 0xffff, -1, pe >> 16);
        const double2 xy = qxy[d];
        const int kn = min(k + D * wps, len - 1);
        qe[d] = v.obs_e[off + 64 * kn + lane];
        qxy[d] = v.obs_xy[off + 64 * kn + lane];
        if (k >= len) continue;  // wave-uniform; no load below
        const bool live = id.x >= 0;
        double ru, rv, jx0[3], jx1[3], rho = 0.0;
        obs_rows_l<LOSS, true, -1, false>(lk, rho, id, xy, X, tabs, ru, rv, jx0, jx1, nullptr, nullptr);
        if (!live) ru = rv = jx0[0] = jx0[1] = jx0[2] = jx1[0] = jx1[1] = jx1[2] = 0.0;
        if constexpr (LOSS != DAB_LOSS_TRIVIAL) rho = live ? rho : 0.0;
        c[0] = fma(jx1[0], jx1[0], fma(jx0[0], jx0[0], c[0]));
        c[1] = fma(jx1[0], jx1[1], fma(jx0[0], jx0[1], c[1]));
        c[2] = fma(jx1[0], jx1[2], fma(jx0[0], jx0[2], c[2]));
        c[3] = fma(jx1[1], jx1[1], fma(jx0[1], jx0[1], c[3]));
        c[4] = fma(jx1[1], jx1[2], fma(jx0[1], jx0[2], c[4]));
        c[5] = fma(jx1[2], jx1[2], fma(jx0[2], jx0[2], c[5]));
        c[6] = fma(jx1[0], rv, fma(jx0[0], ru, c[6]));
        c[7] = fma(jx1[1], rv, fma(jx0[1], ru, c[7]));
        c[8] = fma(jx1[2], rv, fma(jx0[2], ru, c[8]));
        // a non-finite residual makes the lane's r^2 sum non-finite, which the
        // fixed-point add below flags: no per-row finiteness test
        if constexpr (LOSS == DAB_LOSS_TRIVIAL) acc[0] = fma(rv, rv, fma(ru, ru, acc[0]));
        else acc[0] += rho;
      }
    }
    const int p = 64 * sl + lane;
    if (wps > 1) {
      // (one round by construction) parts -> LDS after the tables (fused_wps keeps
      // 12 E + kBalPW * 9 * 64 doubles inside rt_s); the last part sums them in order
      double* cbuf = rt_s + ((12 * v.E + 1) & ~1);
#pragma unroll
      for (int k = 0; k < 9; ++k) cbuf[(pw * 9 + k) * 64 + lane] = c[k];
      unsigned old = 0;
      if (lane == 0) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        old = __hip_atomic_fetch_add(&ccount[kBalCW + slot], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
      old = __builtin_amdgcn_readfirstlane(old);
      if (old != (unsigned)wps - 1) continue;
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        double t = cbuf[((slot * wps) * 9 + k) * 64 + lane];
        for (int q2 = 1; q2 < wps; ++q2) t += cbuf[((slot * wps + q2) * 9 + k) * 64 + lane];
        c[k] = t;
      }
    }
    if (sl < v.nslice && p < v.NP) {
#pragma unroll
      for (int k = 0; k < 6; ++k) V[k * NPs + p] = c[k];
#pragma unroll
      for (int k = 0; k < 3; ++k) g[k * NPs + p] = c[6 + k];
    }
  }
  DAB_STAMP(2);
  // cost: wave sums, summed in wave order by the last point wave, added in fixed point
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const double t = wave_sum_lane63(acc[i]);
    if (lane == 63) shp[pw][i] = t;
  }
  unsigned old = 0;
  if (lane == 63) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    old = __hip_atomic_fetch_add(&pdone, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  old = __builtin_amdgcn_readlane(old, 63);
  DAB_STAMP(3);
  if (old != (unsigned)kBalPW - 1 || lane != 0) return;
  double pc = shp[0][0], bc = shp[0][1];
#pragma unroll
  for (int w = 1; w < kBalPW; ++w) {
    pc += shp[w][0];
    bc += shp[w][1];
  }
  cost_fx_commit(pc, bc, costfx + kFxStride * (blockIdx.x % kFxCopies));
}

void launch_eval_bal(hipStream_t s, const DevView& v, const int* chunk_beg, const double* points, const double* ext,
                     const double* camtab, double* V, double* g, double* ug, unsigned long long* costfx,
                     unsigned long long* fx_next, unsigned* err, int grid, int side) {
  const int wpc = fused_wpc(v.NC, grid), wps = fused_wps(v.nslice, v.E, grid);
  DAB_LOSS_SWITCH(v.loss, {
    if (wpc == 2 && wps == 1)
      k_eval_bal<2, 1, LOSS><<<grid, 1024, 0, s>>>(v, chunk_beg, points, ext, camtab, V, g, ug, costfx, fx_next, err, wpc, wps, side);
    else if (wpc == 8 && wps == 8)
      k_eval_bal<8, 8, LOSS><<<grid, 1024, 0, s>>>(v, chunk_beg, points, ext, camtab, V, g, ug, costfx, fx_next, err, wpc, wps, side);
    else
      k_eval_bal<0, 0, LOSS><<<grid, 1024, 0, s>>>(v, chunk_beg, points, ext, camtab, V, g, ug, costfx, fx_next, err, wpc, wps, side);
  });
}

template <int LOSS>
__global__ __launch_bounds__(256) void k_eval_cross(DevView v, const int* __restrict__ chunk_beg,
                                                    const int4* __restrict__ x_idx,
                                                    const double2* __restrict__ x_xy,
                                                    const double* __restrict__ points,
                                                    const double* __restrict__ camtab,
                                                    double* __restrict__ partial) {
  const int c = blockIdx.x;
  const int b = chunk_beg[c], e = chunk_beg[c + 1];
  double acc[36];
#pragma unroll
  for (int i = 0; i < 36; ++i) acc[i] = 0.0;
  extern __shared__ double tabs_lds[];
  const bool small = small_tabs_fit(v.E, v.NI);
  const LossK lk = loss_of(v);
  SmallTabs st{nullptr, nullptr};
  if (small) st = stage_small_tabs(tabs_lds, v.E, v.NI, camtab, v.intr);
  // both slots' camera rows (no d r / d X), Jc0^T Jc1 accumulated
  auto body = [&](const int4 id, const double2 xy, const double (&X)[3], const auto& tabs) {
    double ru, rv, ja[6], jb[6], da[6], db[6], rho;
    obs_rows_l<LOSS, false, 2>(lk, rho, id, xy, X, tabs, ru, rv, nullptr, nullptr, ja, jb, da, db);
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
      for (int bb = 0; bb < 6; ++bb) acc[6 * a + bb] += ja[a] * da[bb] + jb[a] * db[bb];
  };
  if (small && b < e) {
    // rotated frame: rows [Z_a x A_k | A_k] and [Z_r x A_k R_a | A_k R_a] of the chunk's
    // (arc, ring) pair, the sums taken to B_a^T M B_r afterwards (only R, t, K per entry)
    __shared__ double jl[2][9];
    __shared__ double wsx[kRedBlock / 64][36];
    const int4 id0 = x_idx[b];
    bool sa, sr;
    ext_frame(camtab, id0.y, jl[0], threadIdx.x, sa);
    ext_frame(camtab, id0.z, jl[1], threadIdx.x, sr);
    pipe_entries(x_idx, x_xy, b + threadIdx.x, e, blockDim.x, points,
                 [&](const int4 id, const double2 xy, const double (&X)[3]) {
                   double Ta[12], Tb[12], Kr[6];
                   st.rt(id.y, Ta);
                   st.rt(id.z, Tb);
                   st.k(id.w, Kr);
                   double Q[3], P[3], Z0[3], Z1[3];
                   matvec_add(Tb, X, Tb + 9, Q);
                   matvec_add(Ta, Q, Ta + 9, P);
#pragma unroll
                   for (int k = 0; k < 3; ++k) {
                     Z0[k] = sa ? Q[k] : P[k] - Ta[9 + k];
                     Z1[k] = sr ? X[k] : Q[k] - Tb[9 + k];
                   }
                   Proj pr;
                   project<LOSS>(P, Kr, xy.x, xy.y, pr, true, lk);  // w0 and w1 each carry sqrt(rho')
#pragma unroll
                   for (int row = 0; row < 2; ++row) {
                     const double* A = row == 0 ? pr.A0 : pr.A1;
                     double at[3], w0[6], w1[6];
                     rowmat(A, Ta, at);
                     w0[0] = Z0[1] * A[2] - Z0[2] * A[1];
                     w0[1] = Z0[2] * A[0] - Z0[0] * A[2];
                     w0[2] = Z0[0] * A[1] - Z0[1] * A[0];
                     w1[0] = Z1[1] * at[2] - Z1[2] * at[1];
                     w1[1] = Z1[2] * at[0] - Z1[0] * at[2];
                     w1[2] = Z1[0] * at[1] - Z1[1] * at[0];
#pragma unroll
                     for (int k = 0; k < 3; ++k) {
                       w0[3 + k] = A[k];
                       w1[3 + k] = at[k];
                     }
#pragma unroll
                     for (int a = 0; a < 6; ++a)
#pragma unroll
                       for (int bb = 0; bb < 6; ++bb) acc[6 * a + bb] = fma(w0[a], w1[bb], acc[6 * a + bb]);
                   }
                 });
    {
      double h0[18], h1[18];
#pragma unroll
      for (int k = 0; k < 18; ++k) {
        h0[k] = acc[k];
        h1[k] = acc[18 + k];
      }
      wave_sums_transposed<18>(h0, wsx[threadIdx.x >> 6]);
      wave_sums_transposed<18>(h1, wsx[threadIdx.x >> 6] + 18);
    }
    __syncthreads();
    if (threadIdx.x < 36) {
      double t = wsx[0][threadIdx.x];
#pragma unroll
      for (int w = 1; w < kRedBlock / 64; ++w) t += wsx[w][threadIdx.x];
      wsx[0][threadIdx.x] = t;
    }
    __syncthreads();
    if (threadIdx.x < 36) {  // (B_a^T M B_r)_ij, B = blockdiag(J_l, I)
      const int i = threadIdx.x / 6, j = threadIdx.x - 6 * (threadIdx.x / 6);
      const double* M = wsx[0];
      double x = 0.0;
      if (i < 3 && j < 3) {
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
          for (int q = 0; q < 3; ++q) x += jl[0][3 * p + i] * M[6 * p + q] * jl[1][3 * q + j];
      } else if (i < 3) {
#pragma unroll
        for (int p = 0; p < 3; ++p) x += jl[0][3 * p + i] * M[6 * p + j];
      } else if (j < 3) {
#pragma unroll
        for (int q = 0; q < 3; ++q) x += M[6 * i + q] * jl[1][3 * q + j];
      } else {
        x = M[6 * i + j];
      }
      partial[36 * (size_t)c + threadIdx.x] = x;
    }
    return;
  }
  if (small)
    pipe_entries(x_idx, x_xy, b + threadIdx.x, e, blockDim.x, points,
                 [&](const int4 id, const double2 xy, const double (&X)[3]) { body(id, xy, X, st); });
  else
    pipe_entries(x_idx, x_xy, b + threadIdx.x, e, blockDim.x, points,
                 [&](const int4 id, const double2 xy, const double (&X)[3]) {
                   body(id, xy, X, GlobalTabs{camtab, v.intr});
                 });
  block_reduce_store<36>(acc, partial + 36 * (size_t)c);
}

// The rig's composed observations in ONE pair-major pass (both cameras free): per chunk of
// one (arc, ring) pair, the arc's and the ring's camera blocks (27 each) and the cross
// block (36) from a single projection per observation, in the rotated frame (rows
// [Z_a x A_k | A_k], [Z_r x A_k R_a | A_k R_a]; each camera's J_l applied after the
// sums). It replaces, for these observations, both camera-major entries and the separate
// cross pass: one 56-B input per observation instead of three. k_cam_final adds the
// camera halves to the camera-major partials of the remaining entries.
template <int PNS, int PGD, bool UT = false, int LOSS = DAB_LOSS_TRIVIAL>
__global__ __launch_bounds__(256) void k_eval_pair(DevView v, const int* __restrict__ chunk_beg,
                                                   const int4* __restrict__ x_idx,
                                                   const double2* __restrict__ x_xy,
                                                   const double* __restrict__ points,
                                                   const double* __restrict__ camtab, double* __restrict__ xpart,
                                                   double* __restrict__ cpart) {
  const int c = blockIdx.x;
  const int b = chunk_beg[c], e = chunk_beg[c + 1];
  extern __shared__ double tabs_lds[];
  SmallTabs st{nullptr, nullptr};
  if constexpr (!UT) st = stage_small_tabs(tabs_lds, v.E, v.NI, camtab, v.intr);  // barrier inside
  __shared__ double jl[2][9];
  __shared__ double ws[kRedBlock / 64][90];
  if (b >= e) {
    if (threadIdx.x < 36) xpart[36 * (size_t)c + threadIdx.x] = 0.0;
    if (threadIdx.x < 54) cpart[54 * (size_t)c + threadIdx.x] = 0.0;
    return;
  }
  const int4 id0 = x_idx[b];
  const LossK lk = loss_of(v);
  bool sa, sr;
  ext_frame(camtab, id0.y, jl[0], threadIdx.x, sa);
  ext_frame(camtab, id0.z, jl[1], threadIdx.x, sr);
  double Tau[12], Tbu[12], Ku[6];  // UT: the chunk's one arc, ring and intrinsic
  if constexpr (UT) {
    const GlobalTabs g{camtab, v.intr};
    g.rt(id0.y, Tau);
    g.rt(id0.z, Tbu);
    g.k(id0.w, Ku);
  }
  // [0, 27) arc U | g, [27, 54) ring U | g, [54, 90) cross (arc row-major)
  double acc[90];
#pragma unroll
  for (int i = 0; i < 90; ++i) acc[i] = 0.0;
  pipe_entries_uni<PNS, PGD>(x_idx, x_xy, b, e, threadIdx.x, blockDim.x, points,
               [&](const int4 id, const double2 xy, const double (&X)[3], const bool valid) {
                 double Ta[12], Tb[12], Kr[6];
                 if constexpr (UT) {
#pragma unroll
                   for (int k = 0; k < 12; ++k) {
                     Ta[k] = Tau[k];
                     Tb[k] = Tbu[k];
                   }
#pragma unroll
                   for (int k = 0; k < 6; ++k) Kr[k] = Ku[k];
                 } else {
                   st.rt(id.y, Ta);
                   st.rt(id.z, Tb);
                   st.k(id.w, Kr);
                 }
                 double Q[3], P[3], Z0[3], Z1[3];
                 matvec_add(Tb, X, Tb + 9, Q);
                 matvec_add(Ta, Q, Ta + 9, P);
#pragma unroll
                 for (int k = 0; k < 3; ++k) {
                   Z0[k] = sa ? Q[k] : P[k] - Ta[9 + k];
                   Z1[k] = sr ? X[k] : Q[k] - Tb[9 + k];
                 }
                 Proj pr;
                 // w0, w1 and r are linear in (A, r) of the observation: scaled before the sums
                 project<LOSS>(P, Kr, xy.x, xy.y, pr, true, lk);
                 if (!valid) {  // a lane past the chunk's end: zero rows add exactly nothing
                   pr.ru = pr.rv = 0.0;
#pragma unroll
                   for (int k = 0; k < 3; ++k) pr.A0[k] = pr.A1[k] = 0.0;
                 }
#pragma unroll
                 for (int row = 0; row < 2; ++row) {
                   const double* A = row == 0 ? pr.A0 : pr.A1;
                   const double r = row == 0 ? pr.ru : pr.rv;
                   double at[3], w0[6], w1[6];
                   rowmat(A, Ta, at);
                   w0[0] = Z0[1] * A[2] - Z0[2] * A[1];
                   w0[1] = Z0[2] * A[0] - Z0[0] * A[2];
                   w0[2] = Z0[0] * A[1] - Z0[1] * A[0];
                   w1[0] = Z1[1] * at[2] - Z1[2] * at[1];
                   w1[1] = Z1[2] * at[0] - Z1[0] * at[2];
                   w1[2] = Z1[0] * at[1] - Z1[1] * at[0];
#pragma unroll
                   for (int k = 0; k < 3; ++k) {
                     w0[3 + k] = A[k];
                     w1[3 + k] = at[k];
                   }
                   int k = 0;
#pragma unroll
                   for (int a = 0; a < 6; ++a)
#pragma unroll
                     for (int bb = a; bb < 6; ++bb) {
                       acc[k] = fma(w0[a], w0[bb], acc[k]);
                       acc[27 + k] = fma(w1[a], w1[bb], acc[27 + k]);
                       ++k;
                     }
#pragma unroll
                   for (int a = 0; a < 6; ++a) {
                     acc[21 + a] = fma(w0[a], r, acc[21 + a]);
                     acc[48 + a] = fma(w1[a], r, acc[48 + a]);
                   }
#pragma unroll
                   for (int a = 0; a < 6; ++a)
#pragma unroll
                     for (int bb = 0; bb < 6; ++bb) acc[54 + 6 * a + bb] = fma(w0[a], w1[bb], acc[54 + 6 * a + bb]);
                 }
               });
  {
    double h0[30], h1[30], h2[30];
#pragma unroll
    for (int k = 0; k < 30; ++k) {
      h0[k] = acc[k];
      h1[k] = acc[30 + k];
      h2[k] = acc[60 + k];
    }
    wave_sums_transposed<30>(h0, ws[threadIdx.x >> 6]);
    wave_sums_transposed<30>(h1, ws[threadIdx.x >> 6] + 30);
    wave_sums_transposed<30>(h2, ws[threadIdx.x >> 6] + 60);
  }
  __syncthreads();
  if (threadIdx.x < 90) {
    double t = ws[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kRedBlock / 64; ++w) t += ws[w][threadIdx.x];
    ws[0][threadIdx.x] = t;  // each thread rewrites only what it read
  }
  __syncthreads();
  const double* M = ws[0];
  if (threadIdx.x < 27) {
    cpart[54 * (size_t)c + threadIdx.x] = cam_frame_entry(M, jl[0], threadIdx.x);
  } else if (threadIdx.x < 54) {
    cpart[54 * (size_t)c + threadIdx.x] = cam_frame_entry(M + 27, jl[1], threadIdx.x - 27);
  } else if (threadIdx.x < 90) {  // (B_a^T X B_r)_ij, B = blockdiag(J_l, I)
    const int q = threadIdx.x - 54, i = q / 6, j = q - 6 * (q / 6);
    const double* X = M + 54;
    double x = 0.0;
    if (i < 3 && j < 3) {
#pragma unroll
      for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int r = 0; r < 3; ++r) x += jl[0][3 * p + i] * X[6 * p + r] * jl[1][3 * r + j];
    } else if (i < 3) {
#pragma unroll
      for (int p = 0; p < 3; ++p) x += jl[0][3 * p + i] * X[6 * p + j];
    } else if (j < 3) {
#pragma unroll
      for (int r = 0; r < 3; ++r) x += X[6 * i + r] * jl[1][3 * r + j];
    } else {
      x = X[6 * i + j];
    }
    xpart[36 * (size_t)c + q] = x;
  }
}

bool pair_eval_fits(int E, int NI) { return small_tabs_fit(E, NI); }
void launch_eval_pair(hipStream_t s, const DevView& v, int nchunk, const int* chunk_beg, const int4* x_idx,
                      const double2* x_xy, const double* points, const double* camtab, double* xpart,
                      double* cpart, bool uni_intr) {
  if (nchunk <= 0) return;
  // four register slots, the point gathered one entry ahead: 256 VGPRs and no AGPRs, two
  // waves per SIMD (deeper slots spilled into AGPRs and measured slower: 6 slots 249 us,
  // 5 slots 212 against 198 at C5 before the chunk cut below). With one intrinsic per pair
  // the chunk's arc, ring and intrinsic tables are uniform values (no LDS tables): 198
  // against 244 us.
  DAB_LOSS_SWITCH(v.loss, {
    if (uni_intr)
      k_eval_pair<4, 1, true, LOSS><<<nchunk, 256, 0, s>>>(v, chunk_beg, x_idx, x_xy, points, camtab, xpart, cpart);
    else
      k_eval_pair<4, 1, false, LOSS><<<nchunk, 256, small_tabs_bytes(v.E, v.NI), s>>>(v, chunk_beg, x_idx, x_xy,
                                                                                      points, camtab, xpart, cpart);
  });
}

// ug[c] = its camera-major chunk partials (seg_chunk) + its halves of the pair chunks
// (xcam_list codes 2 q + half, increasing q): one block per camera, 37 stripes of 27
// threads over the terms, the stripes summed in order (fixed order, as k_seg_final_block)
__global__ __launch_bounds__(1024) void k_cam_final(const int* __restrict__ seg_chunk,
                                                   const double* __restrict__ partial,
                                                   const int* __restrict__ xcam_ptr,
                                                   const int* __restrict__ xcam_list,
                                                   const double* __restrict__ cpart, double* __restrict__ ug) {
  constexpr int kS = 1024 / 27;
  __shared__ double sh[kS * 27];
  const int c = blockIdx.x, k = threadIdx.x % 27, stripe = threadIdx.x / 27;
  if (stripe < kS) {
    double t = 0.0;
    const int n1 = seg_chunk[c + 1] - seg_chunk[c], n2 = xcam_ptr[c + 1] - xcam_ptr[c];
    for (int j = stripe; j < n1 + n2; j += kS) {
      if (j < n1) {
        t += partial[27 * (size_t)(seg_chunk[c] + j) + k];
      } else {
        const int code = xcam_list[xcam_ptr[c] + j - n1];
        t += cpart[54 * (size_t)(code >> 1) + 27 * (code & 1) + k];
      }
    }
    sh[stripe * 27 + k] = t;
  }
  __syncthreads();
  if (threadIdx.x < 27) {
    double t = sh[threadIdx.x];
#pragma unroll
    for (int q = 1; q < kS; ++q) t += sh[q * 27 + threadIdx.x];
    ug[27 * (size_t)c + threadIdx.x] = t;
  }
}
void launch_cam_final(hipStream_t s, int NC, const int* seg_chunk, const double* partial, const int* xcam_ptr,
                      const int* xcam_list, const double* cpart, double* ug) {
  if (NC <= 0) return;
  k_cam_final<<<NC, 1024, 0, s>>>(seg_chunk, partial, xcam_ptr, xcam_list, cpart, ug);
}
// the general camera-major kernel over an arbitrary chunk set (no uniform-chunk lists)
void launch_eval_cams_gen(hipStream_t s, const DevView& v, int nchunk, const int* chunk_beg, const double* points,
                          const double* ext, const double* camtab, double* partial) {
  if (nchunk <= 0) return;
  const size_t lds = small_tabs_fit(v.E, v.NI) ? small_tabs_bytes(v.E, v.NI) : 0;
  DAB_LOSS_SWITCH(v.loss, k_eval_cams<false, LOSS><<<nchunk, 256, lds, s>>>(v, chunk_beg, nullptr, points, ext, camtab,
                                                                           partial));
}

void launch_eval_cross(hipStream_t s, const DevView& v, int nchunk, const int* chunk_beg, const int4* x_idx,
                       const double2* x_xy, const double* points, const double* camtab, double* partial) {
  if (nchunk <= 0) return;
  const size_t lds = small_tabs_fit(v.E, v.NI) ? small_tabs_bytes(v.E, v.NI) : 0;
  DAB_LOSS_SWITCH(v.loss,
                  k_eval_cross<LOSS><<<nchunk, 256, lds, s>>>(v, chunk_beg, x_idx, x_xy, points, camtab, partial));
}

// ------------------------------------------------------------------------------------
// LM step: point elimination (Schur complement) and back-substitution
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_point_factor(DevView v, const double* __restrict__ V,
                                                      const double* __restrict__ g,
                                                      const double* __restrict__ sp, StepScalars sc,
                                                      double* __restrict__ L, double* __restrict__ q,
                                                      int* __restrict__ fail) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= v.NP) return;
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
  // PU = diag(s) L^-T: L^-1 = [[a, 0, 0], [b, c, 0], [d, e, f]]
  const double ia = 1.0 / l00, ic = 1.0 / l11, iff = 1.0 / l22;
  const double ib = -l10 * ia * ic;
  const double ie = -l21 * ic * iff;
  const double id = -(l20 * ia + l21 * ib) * iff;
  double* pu = L + 6 * (size_t)p;  // (00, 01, 02, 11, 12, 22) of diag(s) L^-T
  pu[0] = s0 * ia;
  pu[1] = s0 * ib;
  pu[2] = s0 * id;
  pu[3] = s1 * ic;
  pu[4] = s1 * ie;
  pu[5] = s2 * iff;
  reinterpret_cast<double2*>(q)[2 * (size_t)p] = make_double2(q0, q1);
  reinterpret_cast<double2*>(q)[2 * (size_t)p + 1] = make_double2(q2, 0.0);
}

void launch_point_factor(hipStream_t s, const DevView& v, const double* V, const double* g,
                         const double* scale_p, StepScalars sc, double* L, double* q, int* fail) {
  if (v.NP <= 0) return;
  k_point_factor<<<grid_for(v.NP, 256, 1 << 20), 256, 0, s>>>(v, V, g, scale_p, sc, L, q, fail);
}

// Y = (s_c ∘ Jc^T Jp) PU_p. Two passes re-evaluate the rows so that both layouts are
// written with coalesced stores: camera-major (thread per position) and by observation
// slot (thread per SELL slot, both extrinsic slots of the observation).
__device__ __forceinline__ void make_y(const double (&ja)[6], const double (&jb)[6], const double (&jx0)[3],
                                       const double (&jx1)[3], const double* __restrict__ sc,
                                       const double* __restrict__ pu, double (&y)[18]) {
  const double u00 = pu[0], u01 = pu[1], u02 = pu[2], u11 = pu[3], u12 = pu[4], u22 = pu[5];
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    const double sa = sc[a];
    const double w0 = ja[a] * jx0[0] + jb[a] * jx1[0];
    const double w1 = ja[a] * jx0[1] + jb[a] * jx1[1];
    const double w2 = ja[a] * jx0[2] + jb[a] * jx1[2];
    y[3 * a] = sa * (w0 * u00);
    y[3 * a + 1] = sa * (w0 * u01 + w1 * u11);
    y[3 * a + 2] = sa * (w0 * u02 + w1 * u12 + w2 * u22);
  }
}

// SMALL: the camera tables are staged in LDS (small_tabs_fit) and the grid strides
template <class YT, bool SMALL, bool REC = false, int LOSS = DAB_LOSS_TRIVIAL>  // REC: [NE][18] records instead of planes
__global__ __launch_bounds__(256) void k_entry_y(DevView v, const double* __restrict__ points,
                                                 const double* __restrict__ camtab,
                                                 const double* __restrict__ scc,
                                                 const double* __restrict__ PU, YT* __restrict__ Ycm) {
  extern __shared__ double tabs_lds[];
  SmallTabs st{nullptr, nullptr};
  if constexpr (SMALL) st = stage_small_tabs(tabs_lds, v.E, v.NI, camtab, v.intr);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < v.NE; i += gridDim.x * blockDim.x) {
    int4 id = v.cm_idx[i];
    const bool slot1 = (id.w & kSlotBit) != 0;
    id.w &= ~kSlotBit;
    const int c = v.ext_col[slot1 ? id.z : id.y];
    const double2 xy = v.cm_xy[i];
    const double X[3] = {points[3 * (size_t)id.x], points[3 * (size_t)id.x + 1], points[3 * (size_t)id.x + 2]};
    // under a loss both factors of Jc^T Jp carry sqrt(rho'): Y is that of the scaled rows
    const LossK lk = loss_of(v);
    double ru, rv, jx0[3], jx1[3], ja[6], jb[6], rho;
    if constexpr (SMALL) {
      if (slot1) obs_rows_l<LOSS, true, 1>(lk, rho, id, xy, X, st, ru, rv, jx0, jx1, ja, jb);
      else obs_rows_l<LOSS, true, 0>(lk, rho, id, xy, X, st, ru, rv, jx0, jx1, ja, jb);
    } else {
      if (slot1) obs_rows_l<LOSS, true, 1>(lk, rho, id, xy, X, GlobalTabs{camtab, v.intr}, ru, rv, jx0, jx1, ja, jb);
      else obs_rows_l<LOSS, true, 0>(lk, rho, id, xy, X, GlobalTabs{camtab, v.intr}, ru, rv, jx0, jx1, ja, jb);
    }
    double y[18];
    make_y(ja, jb, jx0, jx1, scc + 6 * c, PU + 6 * (size_t)id.x, y);
    if constexpr (REC) {
      double2* dst = reinterpret_cast<double2*>(Ycm + (size_t)kYRec * i);
#pragma unroll
      for (int k = 0; k < 9; ++k) dst[k] = make_double2(y[2 * k], y[2 * k + 1]);
    } else {
      store_yplane(Ycm, (size_t)v.NE, (size_t)i, y);
    }
  }
}

template <class YT, bool SMALL, int LOSS = DAB_LOSS_TRIVIAL>
__global__ __launch_bounds__(256) void k_entry_y_slots(DevView v, const double* __restrict__ points,
                                                       const double* __restrict__ camtab,
                                                       const double* __restrict__ scc,
                                                       const double* __restrict__ PU, YT* __restrict__ Ypm) {
  extern __shared__ double tabs_lds[];
  SmallTabs st{nullptr, nullptr};
  if constexpr (SMALL) st = stage_small_tabs(tabs_lds, v.E, v.NI, camtab, v.intr);
  const size_t NS = (size_t)v.N;
  for (int s = blockIdx.x * blockDim.x + threadIdx.x; s < v.N; s += gridDim.x * blockDim.x) {
    const int4 id = v.obs_idx[s];
    if (id.x < 0) continue;  // padding slot
    const int c0 = v.ext_col[id.y], c1 = id.z >= 0 ? v.ext_col[id.z] : -1;
    if (c0 < 0 && c1 < 0) continue;
    const double X[3] = {points[3 * (size_t)id.x], points[3 * (size_t)id.x + 1], points[3 * (size_t)id.x + 2]};
    const LossK lk = loss_of(v);
    double ru, rv, jx0[3], jx1[3], ja[6], jb[6], da[6], db[6], rho;
    if constexpr (SMALL) obs_rows_l<LOSS, true, 2>(lk, rho, id, v.obs_xy[s], X, st, ru, rv, jx0, jx1, ja, jb, da, db);
    else
      obs_rows_l<LOSS, true, 2>(lk, rho, id, v.obs_xy[s], X, GlobalTabs{camtab, v.intr}, ru, rv, jx0, jx1, ja, jb, da,
                                db);
    const double* pu = PU + 6 * (size_t)id.x;
    double y[18];
    if (c0 >= 0) {
      make_y(ja, jb, jx0, jx1, scc + 6 * c0, pu, y);
      store_yplane(Ypm, NS, (size_t)s, y);
    }
    if (c1 >= 0) {
      make_y(da, db, jx0, jx1, scc + 6 * c1, pu, y);
      store_yplane(Ypm + 18 * NS, NS, (size_t)s, y);
    }
  }
}

template <class YT, int LOSS>
static void launch_entry_y_t(hipStream_t s, const DevView& v, const double* points, const double* camtab,
                             const double* scale_c, const double* PU, YT* cm, YT* pm) {
  const int g = grid_for(v.NE, 256, 1 << 20), gs = grid_for(v.N, 256, 1 << 20);
  if (small_tabs_fit(v.E, v.NI)) {
    const size_t lds = small_tabs_bytes(v.E, v.NI);
    if (cm) k_entry_y<YT, true, false, LOSS><<<std::min(g, kSmallGrid), 256, lds, s>>>(v, points, camtab, scale_c, PU, cm);
    if (pm) k_entry_y_slots<YT, true, LOSS><<<std::min(gs, kSmallGrid), 256, lds, s>>>(v, points, camtab, scale_c, PU, pm);
  } else {
    if (cm) k_entry_y<YT, false, false, LOSS><<<g, 256, 0, s>>>(v, points, camtab, scale_c, PU, cm);
    if (pm) k_entry_y_slots<YT, false, LOSS><<<gs, 256, 0, s>>>(v, points, camtab, scale_c, PU, pm);
  }
}

void launch_entry_y(hipStream_t s, const DevView& v, const double* points, const double* camtab,
                    const double* scale_c, const double* PU, YBufs Y, bool with_pm, double* rec) {
  if (v.NE <= 0) return;
  if (rec && !Y.f32) {  // records for the explicit S blocks; the slot planes as usual
    const int g = grid_for(v.NE, 256, 1 << 20);
    DAB_LOSS_SWITCH(v.loss, {
      if (small_tabs_fit(v.E, v.NI))
        k_entry_y<double, true, true, LOSS><<<std::min(g, kSmallGrid), 256, small_tabs_bytes(v.E, v.NI), s>>>(
            v, points, camtab, scale_c, PU, rec);
      else
        k_entry_y<double, false, true, LOSS><<<g, 256, 0, s>>>(v, points, camtab, scale_c, PU, rec);
      if (with_pm) launch_entry_y_t<double, LOSS>(s, v, points, camtab, scale_c, PU, nullptr, (double*)Y.pm);
    });
    return;
  }
  // fp32 records (pcg_fp32) exist for the TRIVIAL loss only: dab_solve refuses the combination
  if (Y.f32)
    launch_entry_y_t<float, DAB_LOSS_TRIVIAL>(s, v, points, camtab, scale_c, PU, (float*)Y.cm,
                                              with_pm ? (float*)Y.pm : nullptr);
  else
    DAB_LOSS_SWITCH(v.loss, launch_entry_y_t<double, LOSS>(s, v, points, camtab, scale_c, PU, (double*)Y.cm,
                                                           with_pm ? (double*)Y.pm : nullptr));
}

// one wave per S block; lane (a,b) < 36 accumulates -sum Y_row[a,:] . Y_col[b,:]
// Y planes -> one contiguous 144-B record per entry: the S-block pairs gather whole
// records (2 lines) instead of one 8-B element from each of 18 planes (18 lines)
__global__ __launch_bounds__(256) void k_y_records(int NE, const double* __restrict__ Y, double* __restrict__ Yr) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (size_t)kYRec * NE) return;
  const size_t i = t / kYRec, j = t - kYRec * (t / kYRec);
  Yr[t] = Y[j * (size_t)NE + i];
}

// one wave per S block, three pairs per step: lane l < 54 is (group l / 18, row a, column
// pair (c, c + 3)) and sums the terms of the pairs i = group, group + 3, ...; the three
// groups are added in group order at the end (fixed order, deterministic). The old form
// used 36 lanes on one pair per step. Round 6: each group's 18 lanes load the pair's two
// records once, one element each (coalesced 144-B records), into the wave's LDS, and every
// lane takes its row / columns from there — the rows were loaded by every lane that needed
// them before (9 loads per lane per pair, 4.5x the records' bytes through the L1/TA);
// the same products and sums: bitwise the same blocks.
__global__ __launch_bounds__(256) void k_s_blocks(int nblk, const int* __restrict__ blk_pair_beg,
                                                  const int2* __restrict__ pairs,
                                                  const double* __restrict__ Yr,
                                                  double* __restrict__ packed, double* __restrict__ S, int lds,
                                                  const int2* __restrict__ blk_cam) {
  constexpr int U = 4;                     // pairs per group per step
  __shared__ double ys[4][3][U][2 * kYRec];  // [wave][group][pair][x record | y record]
  const int blk = blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (blk >= nblk) return;  // wave-uniform
  const int grp = lane < 54 ? lane / 18 : 3, k = lane - 18 * (lane / 18);
  const int a = k / 3, c = k - 3 * (k / 3);
  double* L = &ys[threadIdx.x >> 6][grp < 3 ? grp : 0][0][0];
  double acc0 = 0.0, acc1 = 0.0;
  auto term = [&](int u, double& t0, double& t1) {
    const double* x = L + 2 * kYRec * u + 3 * a;
    const double* y = L + 2 * kYRec * u + kYRec + 3 * c;
    const double x0 = x[0], x1 = x[1], x2 = x[2];
    t0 = x0 * y[0] + x1 * y[1] + x2 * y[2];
    t1 = x0 * y[9] + x1 * y[10] + x2 * y[11];
  };
  auto sync = []() {  // the group's LDS stores visible to its lanes / its reads done
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  };
  const int e = blk_pair_beg[blk + 1];
  int i = blk_pair_beg[blk] + grp;
  if (grp < 3) {
    // four of the group's pairs in flight per step (twelve per wave)
    for (; i + 9 < e; i += 12) {
      double xv[U], yv[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int2 pr = pairs[i + 3 * u];
        xv[u] = Yr[(size_t)kYRec * pr.x + k];
        yv[u] = Yr[(size_t)kYRec * pr.y + k];
      }
      sync();
#pragma unroll
      for (int u = 0; u < U; ++u) {
        L[2 * kYRec * u + k] = xv[u];
        L[2 * kYRec * u + kYRec + k] = yv[u];
      }
      sync();
      double t0[U], t1[U];
#pragma unroll
      for (int u = 0; u < U; ++u) term(u, t0[u], t1[u]);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        acc0 += t0[u];
        acc1 += t1[u];
      }
    }
    for (; i < e; i += 3) {
      const int2 pr = pairs[i];
      const double xv = Yr[(size_t)kYRec * pr.x + k], yv = Yr[(size_t)kYRec * pr.y + k];
      sync();
      L[k] = xv;
      L[kYRec + k] = yv;
      sync();
      double t0, t1;
      term(0, t0, t1);
      acc0 += t0;
      acc1 += t1;
    }
  }
  // groups 0 + 1 + 2 in order, in the lanes of group 0
  const double g1a = __shfl(acc0, lane + 18), g1b = __shfl(acc1, lane + 18);
  const double g2a = __shfl(acc0, lane + 36), g2b = __shfl(acc1, lane + 36);
  if (lane < 18) {
    double* o = packed + 36 * (size_t)blk + 6 * a;
    if (S) {
      const int2 rc = blk_cam[blk];  // (row cam, col cam), row >= col
      o = S + (size_t)(6 * rc.x + a) * lds + 6 * rc.y;
    }
    o[c] = -((acc0 + g1a) + g2a);
    o[c + 3] = -((acc1 + g1b) + g2b);
  }
}
// the lower blocks of S without any pair (absent from blk_cam): zeros
__global__ void k_s_zero_blocks(int nzero, const int2* __restrict__ blk_zero, double* __restrict__ S, int lds) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nzero * 36) return;
  const int blk = t / 36, ab = t - 36 * blk, a = ab / 6, b = ab - 6 * (ab / 6);
  const int2 rc = blk_zero[blk];
  S[(size_t)(6 * rc.x + a) * lds + 6 * rc.y + b] = 0.0;
}

void launch_s_blocks(hipStream_t s, int nblk, const int* blk_pair_beg, const int2* pairs,
                     const double* Y, int NE, double* packed, double* Yr, double* S, int lds, const int2* blk_cam,
                     int nzero, const int2* blk_zero) {
  if (S && nzero > 0)
    k_s_zero_blocks<<<grid_for(nzero * 36, 256, 1 << 20), 256, 0, s>>>(nzero, blk_zero, S, lds);
  if (nblk <= 0) return;
  if (Y) k_y_records<<<(unsigned)(((size_t)kYRec * NE + 255) / 256), 256, 0, s>>>(NE, Y, Yr);
  k_s_blocks<<<(nblk + 3) / 4, 256, 0, s>>>(nblk, blk_pair_beg, pairs, Yr, packed, S, lds, blk_cam);
}

template <bool REC>
__global__ __launch_bounds__(256) void k_cam_rhs_partial(DevView v, const int* __restrict__ chunk_beg,
                                                         const double* __restrict__ Y,
                                                         const double* __restrict__ q,
                                                         double* __restrict__ partial) {
  const int c = blockIdx.x;
  const int b = chunk_beg[c], e = chunk_beg[c + 1];
  double acc[6] = {0, 0, 0, 0, 0, 0};
  for (int i = b + threadIdx.x; i < e; i += blockDim.x) {
    const int p = v.cm_pt[i];
    const double2 qa = reinterpret_cast<const double2*>(q)[2 * (size_t)p];
    const double q2 = q[4 * (size_t)p + 2];
    double y[18];
    if constexpr (REC) {
      const double2* src = reinterpret_cast<const double2*>(Y + (size_t)kYRec * i);
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        const double2 u = src[k];
        y[2 * k] = u.x;
        y[2 * k + 1] = u.y;
      }
    } else {
      load_yplane(Y, (size_t)v.NE, (size_t)i, y);
    }
#pragma unroll
    for (int a = 0; a < 6; ++a) acc[a] -= y[3 * a] * qa.x + y[3 * a + 1] * qa.y + y[3 * a + 2] * q2;
  }
  block_reduce_store<6>(acc, partial + 6 * (size_t)c);
}

void launch_cam_rhs_partial(hipStream_t s, const DevView& v, int nchunk, const int* chunk_beg,
                            const double* Y, const double* q, double* partial, bool rec) {
  if (nchunk <= 0) return;
  if (rec) k_cam_rhs_partial<true><<<nchunk, 256, 0, s>>>(v, chunk_beg, Y, q, partial);
  else k_cam_rhs_partial<false><<<nchunk, 256, 0, s>>>(v, chunk_beg, Y, q, partial);
}

// --- dense reduced camera system ------------------------------------------------------
__global__ void k_s_scatter(int nblk, const int2* __restrict__ blk_cam, const double* __restrict__ packed,
                            double* __restrict__ S, int lds) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nblk * 36) return;
  const int blk = t / 36, ab = t - 36 * blk, a = ab / 6, b = ab - 6 * (ab / 6);
  const int2 rc = blk_cam[blk];  // (row cam, col cam), row >= col
  S[(size_t)(6 * rc.x + a) * lds + 6 * rc.y + b] = packed[t];
}
__global__ void k_s_diag(int NC, const double* __restrict__ ug, const double* __restrict__ scc,
                         StepScalars sc, const double* __restrict__ ybc, double* __restrict__ S, int lds) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= NC * 36) return;
  const int c = t / 36, ab = t - 36 * c, a = ab / 6, b = ab - 6 * (ab / 6);
  if (b > a) return;  // lower triangle of the diagonal block
  const int q = b * 6 - (b * (b - 1)) / 2 + (a - b);  // upper-packed index of (b, a)
  const double sa = scc[6 * c + a], sb = scc[6 * c + b];
  double u = sa * ug[27 * (size_t)c + q] * sb;
  if (a == b) {
    const double d = fmin(fmax(u, sc.min_diag), sc.max_diag);
    const double D = sqrt(d / sc.radius);
    u += D * D;
  }
  const size_t n = (size_t)6 * NC;
  S[(size_t)(6 * c + a) * lds + 6 * c + b] += u;
  if (b == 0) S[n * lds + 6 * c + a] = sa * ug[27 * (size_t)c + 21 + a] + ybc[6 * c + a];
}
__global__ void k_s_cross(int ncross, const int2* __restrict__ cross_cam, const double* __restrict__ X,
                          const double* __restrict__ scc, double* __restrict__ S, int lds) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ncross * 36) return;
  const int k = t / 36, ab = t - 36 * k, a = ab / 6, b = ab - 6 * (ab / 6);
  const int2 cc = cross_cam[k];  // (c0 = arc, c1 = ring): X = Jc0^T Jc1
  const double v = scc[6 * cc.x + a] * X[36 * (size_t)k + ab] * scc[6 * cc.y + b];
  if (cc.x > cc.y) S[(size_t)(6 * cc.x + a) * lds + 6 * cc.y + b] += v;
  else S[(size_t)(6 * cc.y + b) * lds + 6 * cc.x + a] += v;
}

void launch_s_add_u(hipStream_t s, int NC, const double* ug, int ncross, const int2* cross_cam, const double* Ucross,
                    const double* scale_c, StepScalars sc, const double* ybc, double* S, int lds) {
  if (NC > 0) k_s_diag<<<grid_for(NC * 36, 256, 1 << 20), 256, 0, s>>>(NC, ug, scale_c, sc, ybc, S, lds);
  if (ncross > 0)
    k_s_cross<<<grid_for(ncross * 36, 256, 1 << 20), 256, 0, s>>>(ncross, cross_cam, Ucross, scale_c, S, lds);
}
void launch_s_unpack(hipStream_t s, int NC, int nblk, const int2* blk_cam, const double* packed,
                     const double* ug, int ncross, const int2* cross_cam, const double* Ucross,
                     const double* scale_c, StepScalars sc, const double* ybc, double* S, int lds) {
  const size_t n = (size_t)6 * NC;
  (void)hipMemsetAsync(S, 0, sizeof(double) * (n + 1) * lds, s);
  if (nblk > 0) k_s_scatter<<<grid_for(nblk * 36, 256, 1 << 20), 256, 0, s>>>(nblk, blk_cam, packed, S, lds);
  launch_s_add_u(s, NC, ug, ncross, cross_cam, Ucross, scale_c, sc, ybc, S, lds);
}

// --- explicit reduced camera system for small camera sets: register-owned block tiles ---
// DENSE_SCHUR's S = U~ + D^2 - sum_p Y_p Y_p^T without pair tables. A record is one distinct
// (point, free camera) pair, Y_{p,c} = sum over the point's entries on camera c of
// s_c o (J_c^T J_p) PU_p (6x3). k_schur_y re-evaluates every record once per LM step into
// HBM and adds the rhs sum_p Y_{p,c} q_p in fixed point. k_schur_tiles: the lower block
// triangle of S (blocks (c, d <= c)) is cut into tiles of row ranges (<= 1024 blocks); in a
// work-group every thread OWNS two blocks of the tile and keeps their 72 sums in registers
// (the pair of a heavy and a light block by sampled hit counts, so the lanes of a wave have
// similar work). The records are ordered (batch, camera, point), so a tile whose last row
// camera is c needs only a prefix of each batch; batches arrive by LDS-DMA (global_load_lds,
// no registers) into ONE buffer of the whole LDS (round 6; SchurTiles::single): a batch then
// holds up to 64 points instead of ~34 at C5, so a lane's hit count per batch is Poisson with
// twice the mean and the wave's busiest lane (which every lane waits for) wastes less:
// k_schur_tiles 3.50 -> 3.19 ms at C5 although each batch's DMA is now waited for
// (profiles/r06z6_*). The two-buffer form (batch b + 1 in flight while batch b is summed)
// stays as DAB_TILE_SINGLE=0. Per batch, a per-camera mask of the batch's points and per-camera record offsets
// (the batch header, DMA'd with it) give the records of a (point, camera) pair by a popcount.
// Each thread walks the points that see both of its cameras in batch order. No atomics:
// each block's sum has one fixed order (groups' partials then added in group order), so the
// result is bitwise reproducible.
constexpr size_t kTileBufBytes = kTileLdsMax / 2;  // one LDS buffer: header area + records
__host__ __device__ inline int tile_hdr_bytes(int NC) { return (int)(((size_t)8 * NC + (size_t)4 * (NC + 1) + 15) / 16 * 16); }
int schur_tile_hdr_bytes(int NC) { return tile_hdr_bytes(NC); }
__host__ __device__ inline size_t tile_hdr_area(int NC) { return ((size_t)tile_hdr_bytes(NC) + 1023) / 1024 * 1024; }
int schur_tile_batch_cap(int NC, bool single) {
  // records land in whole 1-KB DMA chunks (a chunk's tail lanes repeat its last piece)
  const size_t area = ((single ? kTileLdsMax : kTileBufBytes) - tile_hdr_area(NC)) / 1024 * 1024;
  return (int)(area / (18 * sizeof(double)));
}

// k_schur_y: thread per record; tables staged in LDS; rhs partials of the work-group in LDS
// (fixed point, 2^(60 - kx[R] - kq) units), then one global integer atomic per rhs row.
template <int LOSS>
__global__ __launch_bounds__(256, 3) void k_schur_y(DevView v, const double* __restrict__ points,
                                                 const double* __restrict__ camtab, const double* __restrict__ PU,
                                                 const double* __restrict__ q, const double* __restrict__ scc,
                                                 SchurTiles a, double* __restrict__ yrec,
                                                 unsigned long long* __restrict__ rhs_out) {
  extern __shared__ __align__(16) double ylds[];
  const SmallTabs st = stage_small_tabs(ylds, v.E, v.NI, camtab, v.intr);
  unsigned long long* rhs = reinterpret_cast<unsigned long long*>(ylds + 30 * (size_t)v.E + 6 * (size_t)v.NI);
  for (int i = threadIdx.x; i < 6 * v.NC; i += blockDim.x) rhs[i] = 0ull;
  __syncthreads();
  // a wave's 64 consecutive records leave through LDS: each lane builds its record, then the
  // wave stores the 9 KB as lane-contiguous 16-B pieces (whole lines, instead of 64 lines
  // touched 16 B at a time by every store)
  const int lane = threadIdx.x & 63;
  // half a wave's records at a time (32 x 144 B per wave): the smaller stage lets three
  // work-groups share a CU (three waves per SIMD)
  double* stage = reinterpret_cast<double*>(rhs + 6 * (size_t)v.NC) + (size_t)(threadIdx.x >> 6) * 32 * 18;
  for (int rb = blockIdx.x * blockDim.x + (threadIdx.x & ~63); rb < a.nrec; rb += gridDim.x * blockDim.x) {
    const int r = rb + lane;
    const int nvalid = min(64, a.nrec - rb);
    double rq[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};  // this record's rhs terms (Y q per row)
    double yo[18];  // this record's Y (staged below)
    int rcam = -1;
    if (r < a.nrec) {
    const int4 ri = a.rec_info[r];  // (first sorted entry, count, point, camera)
    const int pt = ri.z, cam = ri.w;
    const double X[3] = {points[3 * (size_t)pt], points[3 * (size_t)pt + 1], points[3 * (size_t)pt + 2]};
    // W = sum over the record's entries of J_c^T J_p (6 x 3); Y = s_c o (W PU) once after
    double w[18];
#pragma unroll
    for (int k = 0; k < 18; ++k) w[k] = 0.0;
    const int4 ro = a.rec_obs[r];
    for (int e = ri.x; e < ri.x + ri.y; ++e) {
      // the first entry's observation comes with the record; further ones (a point seen by
      // one camera twice: the rig's arc through several rings) are gathered
      int os;
      int4 id;
      if (e == ri.x) {
        os = ro.x;
        id = make_int4(pt, ro.y, ro.z, ro.w);
      } else {
        os = a.sch_ent[e].x;
        id = v.obs_idx[os >> 1];
      }
      double2 xy0 = make_double2(0.0, 0.0);  // the residual is not used ...
      // ... except by a loss: its weight needs the entry's pixel (16 B more per entry)
      if constexpr (LOSS != DAB_LOSS_TRIVIAL) xy0 = v.obs_xy[os >> 1];
      const LossK lk = loss_of(v);
      double ru, rv, jx0[3], jx1[3], ja[6], jb[6], rho;  // the rows of the record's camera slot only
      if (os & 1) obs_rows_l<LOSS, true, 1>(lk, rho, id, xy0, X, st, ru, rv, jx0, jx1, ja, jb);
      else obs_rows_l<LOSS, true, 0>(lk, rho, id, xy0, X, st, ru, rv, jx0, jx1, ja, jb);
#pragma unroll
      for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int k = 0; k < 3; ++k) w[3 * r + k] = fma(jb[r], jx1[k], fma(ja[r], jx0[k], w[3 * r + k]));
    }
    double (&y)[18] = w;  // Y = s_c o (W PU) in place, row by row (W's registers are reused)
    {
      const double* pu = PU + 6 * (size_t)pt;
      const double u00 = pu[0], u01 = pu[1], u02 = pu[2], u11 = pu[3], u12 = pu[4], u22 = pu[5];
#pragma unroll
      for (int r = 0; r < 6; ++r) {
        const double sa = scc[6 * cam + r];
        const double w0 = w[3 * r], w1 = w[3 * r + 1], w2 = w[3 * r + 2];
        y[3 * r] = sa * (w0 * u00);
        y[3 * r + 1] = sa * (w0 * u01 + w1 * u11);
        y[3 * r + 2] = sa * (w0 * u02 + w1 * u12 + w2 * u22);
      }
    }
#pragma unroll
    for (int k = 0; k < 18; ++k) yo[k] = y[k];
    const double q0 = q[4 * (size_t)pt], q1 = q[4 * (size_t)pt + 1], q2 = q[4 * (size_t)pt + 2];
#pragma unroll
    for (int k = 0; k < 6; ++k) rq[k] = y[3 * k] * q0 + y[3 * k + 1] * q1 + y[3 * k + 2] * q2;
    rcam = cam;
    }
    if (rcam >= 0) {  // rhs in fixed point (integer adds: the order does not matter)
#pragma unroll
      for (int k = 0; k < 6; ++k)
        __hip_atomic_fetch_add(rhs + 6 * rcam + k,
                               (unsigned long long)__double2ll_rn(ldexp(rq[k], 60 - a.kx[6 * rcam + k] - a.kq)),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
#pragma unroll
    for (int h2 = 0; h2 < 2; ++h2) {
      const int nv = min(32, nvalid - 32 * h2);
      if (nv <= 0) break;
      if ((lane >> 5) == h2 && rcam >= 0) {
        double2* o = reinterpret_cast<double2*>(stage + 18 * (lane & 31));
#pragma unroll
        for (int k = 0; k < 9; ++k) o[k] = make_double2(yo[2 * k], yo[2 * k + 1]);
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      double2* dst = reinterpret_cast<double2*>(yrec + 18 * ((size_t)rb + 32 * h2));
      const double2* src = reinterpret_cast<const double2*>(stage);
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        const int piece = 64 * j + lane;
        if (piece < 9 * nv) dst[piece] = src[piece];
      }
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 6 * v.NC; i += blockDim.x)
    if (rhs[i]) __hip_atomic_fetch_add(rhs_out + i, rhs[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// one owned block's sums over the batch's points that see both of its cameras (batch order)
__device__ __forceinline__ void tile_block_hits(const double* __restrict__ ly, const unsigned long long* __restrict__ mask,
                                                const int* __restrict__ off, int c, int d, double (&acc)[36]) {
  const unsigned long long mc = mask[c], md = mask[d];
  const int oc = off[c], od = off[d];
  unsigned long long m = mc & md;
  while (m) {
    const int pl = __builtin_ctzll(m);
    m &= m - 1;
    const unsigned long long below = (1ull << pl) - 1ull;
    const double2* pi = reinterpret_cast<const double2*>(ly + 18 * (oc + __builtin_popcountll(mc & below)));
    const double2* pj = reinterpret_cast<const double2*>(ly + 18 * (od + __builtin_popcountll(md & below)));
    double yi[18], yj[18];
#pragma unroll
    for (int u = 0; u < 9; ++u) {
      const double2 zi = pi[u], zj = pj[u];
      yi[2 * u] = zi.x;
      yi[2 * u + 1] = zi.y;
      yj[2 * u] = zj.x;
      yj[2 * u + 1] = zj.y;
    }
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int s2 = 0; s2 < 6; ++s2)
        acc[6 * r + s2] =
            fma(yi[3 * r + 2], yj[3 * s2 + 2], fma(yi[3 * r + 1], yj[3 * s2 + 1], fma(yi[3 * r], yj[3 * s2], acc[6 * r + s2])));
  }
}
__device__ __forceinline__ int tri_row(int bl) {  // c with c (c+1)/2 <= bl < (c+1)(c+2)/2
  int c = (int)((sqrtf(8.0f * bl + 1.0f) - 1.0f) * 0.5f);
  while (tri_n(c + 1) <= bl) ++c;
  while (tri_n(c) > bl) --c;
  return c;
}

// LDS-DMA of batch b into buffer dst: the header, then the records of cameras 0..clast
// (a prefix of the batch). 16-B pieces, 64 lane-linear pieces (1 KB) per wave instruction,
// chunks dealt to the waves round robin; a partial chunk's tail lanes repeat its last piece.
__device__ __forceinline__ void tile_dma_batch(const SchurTiles& a, const double* __restrict__ yrec, int NC, int clast,
                                               int b, unsigned char* dst) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  constexpr int kWaves = kTileThreads / 64;
  const unsigned char* h = a.hdr + (size_t)b * a.hdr_bytes;
  // the prefix length first: an ordinary load's use waits for every load in flight
  const int nrec = reinterpret_cast<const int*>(h + 8 * (size_t)NC)[clast + 1];
  const int hp = a.hdr_bytes / 16;  // header pieces
  for (int j = wave; j * 64 < hp; j += kWaves)
    __builtin_amdgcn_global_load_lds(h + 16 * (size_t)min(j * 64 + lane, hp - 1), dst + 1024 * (size_t)j, 16, 0, 0);
  const int np = 9 * nrec;  // record pieces
  const unsigned char* src = reinterpret_cast<const unsigned char*>(yrec + 18 * (size_t)a.batch_rec[b]);
  unsigned char* rdst = dst + tile_hdr_area(NC);
  for (int j = wave; j * 64 < np; j += kWaves)
    __builtin_amdgcn_global_load_lds(src + 16 * (size_t)min(j * 64 + lane, np - 1), rdst + 1024 * (size_t)j, 16, 0, 0);
}

__global__ __launch_bounds__(kTileThreads) void k_schur_tiles(const double* __restrict__ yrec, SchurTiles a, int NC) {
  extern __shared__ __align__(16) unsigned char tile_lds[];
  // XCD-aware placement: the tiles of one group of points run on one XCD (blocks b and b + 8
  // share one), so the group's records come from HBM once and from that L2 for the others
  // work-group -> (tile t, part j of its group g): the nsub work-groups of one group of
  // batches (every tile, a heavy tile in several parts) run on one XCD
  int u, g;
  if (a.ngroup % 8 == 0) {
    const int x = blockIdx.x & 7, y = blockIdx.x >> 3;
    u = y % a.nsub;
    g = (y / a.nsub) * 8 + x;
  } else {
    u = blockIdx.x % a.nsub;
    g = blockIdx.x / a.nsub;
  }
  int t = 0;
  while (a.tile_subbeg[t + 1] <= u) ++t;
  const int ns = a.tile_sub[t];
  const int slot = g * ns + (u - a.tile_subbeg[t]), nslot = a.ngroup * ns;
  const int clast = a.tile_clast[t];
  const int blA = a.tile_slot[(size_t)t * 2 * kTileThreads + threadIdx.x];
  const int blB = a.tile_slot[(size_t)t * 2 * kTileThreads + kTileThreads + threadIdx.x];
  int cA = 0, dA = 0, cB = 0, dB = 0;
  if (blA >= 0) {
    cA = tri_row(blA);
    dA = blA - (int)tri_n(cA);
  }
  if (blB >= 0) {
    cB = tri_row(blB);
    dB = blB - (int)tri_n(cB);
  }
  double accA[36], accB[36];
#pragma unroll
  for (int k = 0; k < 36; ++k) accA[k] = accB[k] = 0.0;
  const int b0 = (int)((long long)a.nbatch * slot / nslot), b1 = (int)((long long)a.nbatch * (slot + 1) / nslot);
  const bool single = a.single != 0;
  if (b0 < b1 && !single) tile_dma_batch(a, yrec, NC, clast, b0, tile_lds);
  __syncthreads();  // drains the DMA (vmcnt) and publishes buffer 0
  for (int b = b0; b < b1; ++b) {
    unsigned char* cur = single ? tile_lds : tile_lds + kTileBufBytes * ((b - b0) & 1);
    if (single) {  // one buffer: the batch lands, then it is summed
      tile_dma_batch(a, yrec, NC, clast, b, tile_lds);
      __syncthreads();
    } else if (b + 1 < b1) {
      // the next batch streams into the other buffer while this one is summed (the sums
      // below touch only LDS and registers, so nothing waits for the DMA before the barrier)
      tile_dma_batch(a, yrec, NC, clast, b + 1, tile_lds + kTileBufBytes * ((b + 1 - b0) & 1));
    }
    const unsigned long long* mask = reinterpret_cast<const unsigned long long*>(cur);
    const int* off = reinterpret_cast<const int*>(cur + 8 * (size_t)NC);
    const double* ly = reinterpret_cast<const double*>(cur + tile_hdr_area(NC));
    if (blA >= 0) tile_block_hits(ly, mask, off, cA, dA, accA);
    if (blB >= 0) tile_block_hits(ly, mask, off, cB, dB, accB);
    __syncthreads();  // batch b consumed, batch b + 1 landed
  }
  double* out = a.partial + (size_t)slot * a.stride;
  if (blA >= 0) {
    double2* o = reinterpret_cast<double2*>(out + 36 * (size_t)blA);
#pragma unroll
    for (int k = 0; k < 18; ++k) o[k] = make_double2(accA[2 * k], accA[2 * k + 1]);
  }
  if (blB >= 0) {
    double2* o = reinterpret_cast<double2*>(out + 36 * (size_t)blB);
#pragma unroll
    for (int k = 0; k < 18; ++k) o[k] = make_double2(accB[2 * k], accB[2 * k + 1]);
  }
}

// Row exponents of the fixed-point rhs: 2^kx[R] >= sqrt(s_R^2 U_RR) (U from ug, all-reduced)
__global__ void k_schur_scale(int NC, const double* __restrict__ ug, const double* __restrict__ scc,
                              int* __restrict__ kx) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 6 * NC) return;
  const int c = i / 6, a = i - 6 * c;
  const double s = scc[i];
  const double u = s * s * ug[27 * (size_t)c + a * 6 - (a * (a - 1)) / 2];
  int k = 0;
  if (u > 0.0 && isfinite(u)) {
    int e;
    (void)frexp(u, &e);  // u < 2^e, so sqrt(u) < 2^ceil(e/2)
    k = (e + 1) >> 1;
  }
  kx[i] = k;
}

// p[0] + p[stride] + ... + p[(n - 1) stride], added in that order; the loads leave eight at
// a time (a loop of dependent load -> add pairs ran at ~0.8 TB/s)
__device__ __forceinline__ double sum_partials_in_order(const double* __restrict__ p, size_t stride, int n) {
  double s = 0.0;
  int g = 0;
  for (; g + 8 <= n; g += 8) {
    double v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = p[(size_t)(g + u) * stride];
#pragma unroll
    for (int u = 0; u < 8; ++u) s += v[u];
  }
  for (; g < n; ++g) s += p[(size_t)g * stride];
  return s;
}

// the tiles' partials: element i of block i / 36 summed over that block's slots in order
__global__ void k_schur_sum_tiles(const int* __restrict__ blk_nslot, size_t stride, size_t count,
                                  const double* __restrict__ partial, double* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const int ns = blk_nslot[i / 36];
  out[i] = sum_partials_in_order(partial + i, stride, ns);
}
void launch_schur_sum_tiles(hipStream_t s, const SchurTiles& a, double* out) {
  const size_t count = (size_t)a.nelem;
  if (count > 0)
    k_schur_sum_tiles<<<(unsigned)((count + 255) / 256), 256, 0, s>>>(a.blk_nslot, a.stride, count, a.partial, out);
}

// sum over the groups' partials in group order (fixed: bitwise reproducible)
__global__ void k_schur_sum(int ngroup, size_t stride, size_t count, const double* __restrict__ partial,
                            double* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  out[i] = sum_partials_in_order(partial + i, stride, ngroup);
}

// dense S lower (rows 0..n-1) = -(Schur part), ybc = -(fixed-point rhs part); the U part, D^2
// and the rhs row follow (launch_s_add_u)
__global__ void k_schur_unpack(int NC, const double* __restrict__ sblk, const unsigned long long* __restrict__ rfx,
                               const int* __restrict__ kx, int kq, double* __restrict__ S, int lds,
                               double* __restrict__ ybc) {
  const int n = 6 * NC;
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t nlow = (size_t)tri_n(n);
  if (t < nlow) {
    int R = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while (tri_n(R + 1) <= (long long)t) ++R;
    while (tri_n(R) > (long long)t) --R;
    const int C = (int)(t - tri_n(R));
    const int c = R / 6, r = R - 6 * c, d = C / 6, s = C - 6 * d;
    S[(size_t)R * lds + C] = -sblk[36 * tri_n(c) + 36 * d + 6 * r + s];
  } else if (t < nlow + (size_t)n) {
    const int R = (int)(t - nlow);
    ybc[R] = -ldexp((double)(long long)rfx[R], kx[R] + kq - 60);
  }
}

void launch_schur_y(hipStream_t s, const DevView& v, const double* points, const double* camtab, const double* PU,
                    const double* q, const double* scale_c, const SchurTiles& a, double* yrec,
                    unsigned long long* rhs_out) {
  if (a.nrec <= 0) return;
  const size_t lds = small_tabs_bytes(v.E, v.NI) + sizeof(unsigned long long) * 6 * (size_t)v.NC +
                     sizeof(double) * 4 * 32 * 18;  // + a half-wave record stage per wave
  DAB_LOSS_SWITCH(v.loss, k_schur_y<LOSS><<<std::min(grid_for(a.nrec, 256, 1 << 20), kSmallGrid), 256, lds, s>>>(
                              v, points, camtab, PU, q, scale_c, a, yrec, rhs_out));
}
void launch_schur_tiles(hipStream_t s, const double* yrec, const SchurTiles& a, int NC) {
  static bool attr = false;
  if (!attr) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(k_schur_tiles), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)kTileLdsMax);
    attr = true;
  }
  k_schur_tiles<<<a.nsub * a.ngroup, kTileThreads, kTileLdsMax, s>>>(yrec, a, NC);
}
void launch_schur_scale(hipStream_t s, int NC, const double* ug, const double* scale_c, int* kx) {
  if (NC > 0) k_schur_scale<<<grid_for(6 * NC, 256, 1 << 20), 256, 0, s>>>(NC, ug, scale_c, kx);
}
void launch_schur_sum(hipStream_t s, int ngroup, size_t stride, size_t count, const double* partial, double* out) {
  if (count > 0) k_schur_sum<<<(unsigned)((count + 255) / 256), 256, 0, s>>>(ngroup, stride, count, partial, out);
}
void launch_schur_unpack(hipStream_t s, int NC, const double* sblk, const unsigned long long* rfx, const int* kx,
                         int kq, double* S, int lds, double* ybc) {
  const size_t n = (size_t)6 * NC, cnt = (size_t)tri_n((long long)n) + n;
  if (cnt > 0) k_schur_unpack<<<(unsigned)((cnt + 255) / 256), 256, 0, s>>>(NC, sblk, rfx, kx, kq, S, lds, ybc);
}

// delta_p = -PU (q - sum_e Y_e^T y_c): lane = point, walking its SELL observation slots
// (coalesced planar Y records of both extrinsic slots)
template <class YT>
__global__ __launch_bounds__(256) void k_backsub(DevView v, const double* __restrict__ PU,
                                                 const double* __restrict__ q, const YT* __restrict__ Ypm,
                                                 const double* __restrict__ yc, double* __restrict__ dp) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= v.NP) return;
  const size_t NPs = (size_t)v.NP, NS = (size_t)v.N;
  const double2 qa = reinterpret_cast<const double2*>(q)[2 * (size_t)p];
  double r[3] = {qa.x, qa.y, q[4 * (size_t)p + 2]};
  if (yc) {
    const int sl = p >> 6, lane = p & 63;
    const int off = v.slice_off[sl], len = (v.slice_off[sl + 1] - off) >> 6;
    for (int k = 0; k < len; ++k) {
      const int s = off + 64 * k + lane;
      const int4 id = v.obs_idx[s];
      if (id.x < 0) continue;
#pragma unroll
      for (int slot = 0; slot < 2; ++slot) {
        const int e = slot ? id.z : id.y;
        const int c = e >= 0 ? v.ext_col[e] : -1;
        if (c < 0) continue;
        double y[18];
        load_yplane(Ypm + slot * 18 * NS, NS, (size_t)s, y);
#pragma unroll
        for (int a = 0; a < 6; ++a) {
          const double ycv = yc[6 * c + a];
          r[0] -= y[3 * a] * ycv;
          r[1] -= y[3 * a + 1] * ycv;
          r[2] -= y[3 * a + 2] * ycv;
        }
      }
    }
  }
  // step = -y (Ceres solves J y = r then negates); delta = step * s = -PU (...)
  const double* pu = PU + 6 * (size_t)p;
  dp[p] = -(pu[0] * r[0] + pu[1] * r[1] + pu[2] * r[2]);
  dp[NPs + p] = -(pu[3] * r[1] + pu[4] * r[2]);
  dp[2 * NPs + p] = -(pu[5] * r[2]);
}

// ------------------------------------------------------------------------------------
// Matrix-free implicit Schur (small camera sets: NC <= kMfCams and the tables fit in LDS,
// i.e. the rig and BAL problems of up to ~100 cameras).
// ------------------------------------------------------------------------------------
// The stored-Y PCG writes Y_e = diag(s_c) (J_c^T J_p) PU_p (144 B fp64 / 72 B fp32 per
// entry) once per LM step and streams it twice per CG product: at C5 that is 1.38 GB
// per pass (fp32), 430 us per product and 1.2 ms per step to build. Here nothing is
// stored: every pass re-evaluates the observation's rows from its 32-B inputs (tables
// and s_c in LDS) and applies the factors directly,
//   t_p  = PU_p^T sum_e J_p^T (J_c (s_c o v_c))          (Y_e^T v, summed over the point)
//   w_c -= s_c o J_c^T (J_p (PU_p t_p))                   (Y_e t_p, per entry)
// with J_p shared by both extrinsic slots of an arc∘ring observation. One product = two
// sweeps over a point's SELL rows (lane = point); the camera sums go to per-wave LDS
// accumulators (LDS atomics only between the lanes of one instruction; waves, then
// work-groups, summed in fixed order: bitwise repeatable). All arithmetic fp64.
constexpr int kMfCams = kMfCamsMax;
constexpr int kMfBlock = 256;
// -DDAB_ABL_MF_NOSUMS (timing only, wrong results): the products' sweep-2 camera sums go to
// a register instead of the per-wave fp64 LDS atomics (scripts/runs/r06y2.sh)
#ifdef DAB_ABL_MF_NOSUMS
#define MF_LDS_ADD(ptr, x) (mf_sink += (x))
#else
#define MF_LDS_ADD(ptr, x) atomicAdd((ptr), (x))
#endif
bool mf_schur_fits(int NC, int E, int NI) { return NC > 0 && NC <= kMfCams && small_tabs_fit(E, NI); }
__device__ __forceinline__ void mv3(const double* __restrict__ M, const double (&x)[3], double (&o)[3]) {
  o[0] = M[0] * x[0] + M[1] * x[1] + M[2] * x[2];
  o[1] = M[3] * x[0] + M[4] * x[1] + M[5] * x[2];
  o[2] = M[6] * x[0] + M[7] * x[1] + M[8] * x[2];
}
__device__ __forceinline__ void mtv3(const double* __restrict__ M, const double (&x)[3], double (&o)[3]) {
  o[0] = M[0] * x[0] + M[3] * x[1] + M[6] * x[2];
  o[1] = M[1] * x[0] + M[4] * x[1] + M[7] * x[2];
  o[2] = M[2] * x[0] + M[5] * x[1] + M[8] * x[2];
}
__device__ __forceinline__ void cross3(const double (&a)[3], const double (&b)[3], double (&o)[3]) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}
// The same products in the rotated frame. With J_l = Rd Jd (the left Jacobian; Rd = R, or
// I for the small-angle tables) and Z = Rd Y (= P - t, or Y itself for the small-angle
// tables), Rd (Y x (Jd dw)) = Z x (J_l dw) and Jd^T (Y x (Rd^T g)) = J_l^T (Z x g), so
//   J_c0 d = A (dt_a - Z_a x w~_a)      w~ = J_l dw: one 3-vector per camera and product
//   J_c0^T z = [J_l^T (Z_a x g); g]     J_l^T applied once per camera to the summed [Z x g]
// (ring slot: Z_r = Q - t_r or X, and R_a as before). Per observation and sweep the rows
// need only R, t (and K) from LDS: the 18 Rd | Jd doubles per slot of the directional
// (Rd | Jd) form, the s_c reads and the 3 x 3 products with them drop out. LDS: rt [E][12] | small-angle
// flags [E] | w~, dt per camera [NC][6] | J_l per camera [NC][9] | per-wave sums [4][NC][6].
// R | t rows of 14 doubles (12 used): 112 B = 28 banks apart, so the 16-B reads of 16
// different cameras fall in 16 disjoint bank quads (a 12-double row gives only 8)
constexpr int kRtStride = 14;
static size_t mf2_lds_bytes(int E, int NI, int NC, bool product) {
  return sizeof(double) * (kRtStride * (size_t)E + 6 * (size_t)NI + 6 * (size_t)NC + 9 * (size_t)NC +
                           (product ? (kMfBlock / 64) * 6 * (size_t)(NC | 1) : 0)) +
         2 * sizeof(int) * (size_t)E;
}
template <int MODE, int LOSS = DAB_LOSS_TRIVIAL>
__global__ __launch_bounds__(kMfBlock, 4) void k_mf_frame(DevView v, const double* __restrict__ points,
                                                       const double* __restrict__ camtab,
                                                       const double* __restrict__ scc,
                                                       const double* __restrict__ PU,
                                                       const double* __restrict__ vec,
                                                       const double* __restrict__ q, double* __restrict__ out,
                                                       const PcgState* st) {
  extern __shared__ double mf_lds[];
  if (MODE == 0 && st->status != kPcgRunning) return;
  const int NC6 = 6 * v.NC;
  double* rt_s = mf_lds;                               // [E][12]
  double* k_s = rt_s + kRtStride * (size_t)v.E;        // [NI][6]
  double* dv_s = k_s + 6 * (size_t)v.NI;               // [NC][6]: w~ | dt (MODE 0, 1)
  double* jl_s = dv_s + NC6;                           // [NC][9]: J_l (MODE 0, 2)
  // per-wave camera sums (MODE 0, 2), component-major [waves][6][NCP], odd NCP: the lanes of
  // one atomic add one component of their cameras, which fall in different banks
  const int NCP = v.NC | 1;
  double* accs = jl_s + 9 * (size_t)v.NC;
  int* sm_s = reinterpret_cast<int*>(accs + (MODE != 1 ? (kMfBlock / 64) * 6 * NCP : 0));  // [E]
  int* col_s = sm_s + v.E;                             // [E] ext_col: no dependent global load per slot
  for (int i = threadIdx.x; i < 12 * v.E; i += blockDim.x) rt_s[kRtStride * (i / 12) + i % 12] = camtab[(size_t)kCamTab * (i / 12) + i % 12];
  for (int i = threadIdx.x; i < 6 * v.NI; i += blockDim.x) k_s[i] = v.intr[(size_t)kIntr * (i / 6) + i % 6];
  for (int e = threadIdx.x; e < v.E; e += blockDim.x) {
    const double* T = camtab + (size_t)kCamTab * e;  // R t Rd Jd
    sm_s[e] = (T[12] == 1.0 && T[13] == 0.0 && T[14] == 0.0 && T[15] == 0.0 && T[16] == 1.0 && T[17] == 0.0 &&
               T[18] == 0.0 && T[19] == 0.0 && T[20] == 1.0)
                  ? 1
                  : 0;  // Rd = I: the small-angle tables
    const int c = v.ext_col[e];
    col_s[e] = c;
    if (c < 0) continue;
    double J[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int cc = 0; cc < 3; ++cc)
        J[3 * r + cc] = T[12 + 3 * r] * T[21 + cc] + T[12 + 3 * r + 1] * T[24 + cc] + T[12 + 3 * r + 2] * T[27 + cc];
    if constexpr (MODE != 2) {
      double d[6];
#pragma unroll
      for (int k = 0; k < 6; ++k) d[k] = scc[6 * c + k] * vec[6 * c + k];
#pragma unroll
      for (int r = 0; r < 3; ++r) dv_s[6 * c + r] = J[3 * r] * d[0] + J[3 * r + 1] * d[1] + J[3 * r + 2] * d[2];
#pragma unroll
      for (int k = 3; k < 6; ++k) dv_s[6 * c + k] = d[k];
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) jl_s[9 * c + k] = J[k];
  }
  if constexpr (MODE != 1)
    for (int i = threadIdx.x; i < (kMfBlock / 64) * 6 * NCP; i += blockDim.x) accs[i] = 0.0;
  __syncthreads();
  const SmallTabs tabs{nullptr, k_s};
  auto rt = [&](int e, double (&o)[12]) {
    const double2* pp = reinterpret_cast<const double2*>(rt_s + kRtStride * e);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const double2 u = pp[k];
      o[2 * k] = u.x;
      o[2 * k + 1] = u.y;
    }
  };
  double* acc = accs + (threadIdx.x >> 6) * 6 * NCP;
#ifdef DAB_ABL_MF_NOSUMS
  double mf_sink = 0.0;  // kept live (a store no run takes) so the sums' arithmetic stays
  struct SinkGuard {
    double& s;
    double* o;
    __device__ ~SinkGuard() {
      if (s == -1.25e300) o[0] = s;
    }
  } sink_guard{mf_sink, out};
#endif
  const size_t NPs = (size_t)v.NP;
  auto rot9 = [&](int e, double (&o)[9]) {
    const double2* pp = reinterpret_cast<const double2*>(rt_s + kRtStride * e);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const double2 u = pp[k];
      o[2 * k] = u.x;
      o[2 * k + 1] = u.y;
    }
    o[8] = rt_s[kRtStride * e + 8];
  };
  // one observation's geometry: A (2 x 3), R_a, and the rotated-frame points Z of both
  // slots; with RB, vout = R_b vin (vin for single-extrinsic observations) while the ring
  // table is in registers, so that R_b never outlives its read
  auto geo = [&](auto rb_tag, const int4 id, const double2 xy, const double (&X)[3], double (&A0)[3],
                 double (&A1)[3], double (&Ra)[9], double (&Z0)[3], double (&Z1)[3], bool& comp,
                 const double (&vin)[3], double (&vout)[3]) {
    constexpr bool RB = decltype(rb_tag)::value;
    double Ta[12];
    rt(id.y, Ta);
    double Kr[6];
    tabs.k(id.w, Kr);
    comp = id.z >= 0;
    double Q[3];
    if constexpr (RB) {
#pragma unroll
      for (int k = 0; k < 3; ++k) vout[k] = vin[k];
    }
    if (comp) {
      double Tb[12];
      rt(id.z, Tb);
      matvec_add(Tb, X, Tb + 9, Q);
      if constexpr (RB) mv3(Tb, vin, vout);
      const bool sb = sm_s[id.z] != 0;
#pragma unroll
      for (int k = 0; k < 3; ++k) Z1[k] = sb ? X[k] : Q[k] - Tb[9 + k];
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k) Q[k] = X[k];
    }
    double P[3];
    matvec_add(Ta, Q, Ta + 9, P);
    const bool sa = sm_s[id.y] != 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) Z0[k] = sa ? Q[k] : P[k] - Ta[9 + k];
    Proj pr;
    // every product below is A^T A applied to a vector: the two scaled factors give rho'
    project<LOSS>(P, Kr, xy.x, xy.y, pr, true, loss_of(v));
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      A0[k] = pr.A0[k];
      A1[k] = pr.A1[k];
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) Ra[k] = Ta[k];
  };
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < v.NP; p += gridDim.x * blockDim.x) {
    const int sl = p >> 6, lane = p & 63;
    const int off = v.slice_off[sl], len = (v.slice_off[sl + 1] - off) >> 6;
    const double X[3] = {points[3 * (size_t)p], points[3 * (size_t)p + 1], points[3 * (size_t)p + 2]};
    double pu[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) pu[k] = PU[6 * (size_t)p + k];
    double up[3];
    if constexpr (MODE == 2) {
      const double q0 = q[4 * (size_t)p], q1 = q[4 * (size_t)p + 1], q2 = q[4 * (size_t)p + 2];
      up[0] = pu[0] * q0 + pu[1] * q1 + pu[2] * q2;
      up[1] = pu[3] * q1 + pu[4] * q2;
      up[2] = pu[5] * q2;
    } else {
      // sweep 1: a = sum_e J_p^T (J_c (s_c o v_c)); the next slot's index is in flight
      double a[3] = {0.0, 0.0, 0.0};
      int4 nid = len > 0 ? v.obs_idx[off + lane] : make_int4(-1, 0, -1, 0);
      for (int k = 0; k < len; ++k) {
        const int s = off + 64 * k + lane;
        const int4 id = nid;
        if (k + 1 < len) nid = v.obs_idx[s + 64];
        if (id.x < 0) continue;
        const int c0 = col_s[id.y], c1 = id.z >= 0 ? col_s[id.z] : -1;
        if (c0 < 0 && c1 < 0) continue;
        double A0[3], A1[3], Ra[9], Z0[3], Z1[3], unused[3];
        bool comp;
        geo(std::false_type{}, id, v.obs_xy[s], X, A0, A1, Ra, Z0, Z1, comp, unused, unused);
        double dP[3] = {0.0, 0.0, 0.0};
        if (c0 >= 0) {
          const double* d = dv_s + 6 * c0;
          const double w[3] = {d[0], d[1], d[2]};
          double cz[3];
          cross3(Z0, w, cz);
#pragma unroll
          for (int k2 = 0; k2 < 3; ++k2) dP[k2] = d[3 + k2] - cz[k2];
        }
        if (c1 >= 0) {
          const double* d = dv_s + 6 * c1;
          const double w[3] = {d[0], d[1], d[2]};
          double cz[3], r[3], r2[3];
          cross3(Z1, w, cz);
#pragma unroll
          for (int k2 = 0; k2 < 3; ++k2) r[k2] = d[3 + k2] - cz[k2];
          mv3(Ra, r, r2);
#pragma unroll
          for (int k2 = 0; k2 < 3; ++k2) dP[k2] += r2[k2];
        }
        const double u0 = A0[0] * dP[0] + A0[1] * dP[1] + A0[2] * dP[2];
        const double u1 = A1[0] * dP[0] + A1[1] * dP[1] + A1[2] * dP[2];
        const double au[3] = {u0 * A0[0] + u1 * A1[0], u0 * A0[1] + u1 * A1[1], u0 * A0[2] + u1 * A1[2]};
        double h[3];
        mtv3(Ra, au, h);
        if (comp) {
          double Rb[9], h2[3];
          rot9(id.z, Rb);  // re-read: fewer live registers than carrying it from geo
          mtv3(Rb, h, h2);
#pragma unroll
          for (int k2 = 0; k2 < 3; ++k2) h[k2] = h2[k2];
        }
        a[0] += h[0];
        a[1] += h[1];
        a[2] += h[2];
      }
      const double t0 = pu[0] * a[0], t1 = pu[1] * a[0] + pu[3] * a[1];
      const double t2 = pu[2] * a[0] + pu[4] * a[1] + pu[5] * a[2];
      if constexpr (MODE == 1) {
        const double r0 = q[4 * (size_t)p] - t0, r1 = q[4 * (size_t)p + 1] - t1, r2 = q[4 * (size_t)p + 2] - t2;
        out[p] = -(pu[0] * r0 + pu[1] * r1 + pu[2] * r2);
        out[NPs + p] = -(pu[3] * r1 + pu[4] * r2);
        out[2 * NPs + p] = -(pu[5] * r2);
        continue;
      }
      up[0] = pu[0] * t0 + pu[1] * t1 + pu[2] * t2;
      up[1] = pu[3] * t1 + pu[4] * t2;
      up[2] = pu[5] * t2;
    }
    if constexpr (MODE != 1) {
      // sweep 2: per camera, sum [Z x g | g] (J_l^T and -s_c applied after the sums)
      int4 nid = len > 0 ? v.obs_idx[off + lane] : make_int4(-1, 0, -1, 0);
      for (int k = 0; k < len; ++k) {
        const int s = off + 64 * k + lane;
        const int4 id = nid;
        if (k + 1 < len) nid = v.obs_idx[s + 64];
        if (id.x < 0) continue;
        const int c0 = col_s[id.y], c1 = id.z >= 0 ? col_s[id.z] : -1;
        if (c0 < 0 && c1 < 0) continue;
        double A0[3], A1[3], Ra[9], Z0[3], Z1[3], kk[3];
        bool comp;
        geo(std::true_type{}, id, v.obs_xy[s], X, A0, A1, Ra, Z0, Z1, comp, up, kk);
        double m[3];
        mv3(Ra, kk, m);
        const double z0 = A0[0] * m[0] + A0[1] * m[1] + A0[2] * m[2];
        const double z1 = A1[0] * m[0] + A1[1] * m[1] + A1[2] * m[2];
        const double gz[3] = {z0 * A0[0] + z1 * A1[0], z0 * A0[1] + z1 * A1[1], z0 * A0[2] + z1 * A1[2]};
        if (c0 >= 0) {
          double cz[3];
          cross3(Z0, gz, cz);
#pragma unroll
          for (int a = 0; a < 3; ++a) MF_LDS_ADD(acc + a * NCP + c0, cz[a]);
#pragma unroll
          for (int a = 0; a < 3; ++a) MF_LDS_ADD(acc + (3 + a) * NCP + c0, gz[a]);
        }
        if (c1 >= 0) {
          double hz[3], cz[3];
          mtv3(Ra, gz, hz);
          cross3(Z1, hz, cz);
#pragma unroll
          for (int a = 0; a < 3; ++a) MF_LDS_ADD(acc + a * NCP + c1, cz[a]);
#pragma unroll
          for (int a = 0; a < 3; ++a) MF_LDS_ADD(acc + (3 + a) * NCP + c1, hz[a]);
        }
      }
    }
  }
  if constexpr (MODE != 1) {
    __syncthreads();
    for (int i = threadIdx.x; i < NC6; i += blockDim.x) {
      const int c = i / 6, k = i - 6 * c;
      double x;
      if (k < 3) {  // J_l^T of the summed rotation parts
        x = 0.0;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          double t = accs[r * NCP + c];
#pragma unroll
          for (int w = 1; w < kMfBlock / 64; ++w) t += accs[(w * 6 + r) * NCP + c];
          x += jl_s[9 * c + 3 * r + k] * t;
        }
      } else {
        x = accs[k * NCP + c];
#pragma unroll
        for (int w = 1; w < kMfBlock / 64; ++w) x += accs[(w * 6 + k) * NCP + c];
      }
      out[(size_t)blockIdx.x * NC6 + i] = -scc[i] * x;
    }
  }
}

// ---- mixed precision (BASELINE config 5): the Schur product in fp32 arithmetic ----------
// k_mf_frame<0> with every per-observation operation in fp32: the R, t tables, the focal and
// distortion terms, w~ and dt per camera are staged in LDS as floats (24 instead of 48 B per
// table read), the point, PU_p and the projection Jacobian A are fp32, and so are the two
// sweeps' 3-vectors. Accumulation stays fp64: each observation's camera terms are widened
// before the per-wave LDS sums, J_l^T and -s_c are applied to the fp64 sums, and the
// work-group partials are added in fixed order (launch_pcg_fused_final). The product is
// accurate to ~1e-7 relative; the PCG keeps its recurrences, dot products and the periodic
// true residual r = b - S x in fp64 (that product is the fp64 k_mf_frame<0>), which is the
// iterative refinement that bounds the drift of the fp32 products. The observed pixel is
// not read: the products need the Jacobian only.
__device__ __forceinline__ void mv3f(const float* __restrict__ M, const float (&x)[3], float (&o)[3]) {
  o[0] = M[0] * x[0] + M[1] * x[1] + M[2] * x[2];
  o[1] = M[3] * x[0] + M[4] * x[1] + M[5] * x[2];
  o[2] = M[6] * x[0] + M[7] * x[1] + M[8] * x[2];
}
__device__ __forceinline__ void mtv3f(const float* __restrict__ M, const float (&x)[3], float (&o)[3]) {
  o[0] = M[0] * x[0] + M[3] * x[1] + M[6] * x[2];
  o[1] = M[1] * x[0] + M[4] * x[1] + M[7] * x[2];
  o[2] = M[2] * x[0] + M[5] * x[1] + M[8] * x[2];
}
__device__ __forceinline__ void cross3f(const float (&a)[3], const float (&b)[3], float (&o)[3]) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}
// d (ru, rv) / d P of projectPoint (the Jacobian half of `project`), K = fx fy k0 k1
__device__ __forceinline__ void proj_jac32(const float (&P)[3], const float4 K, float (&A0)[3], float (&A1)[3]) {
  float iz = __builtin_amdgcn_rcpf(P[2]);
  iz = fmaf(iz, fmaf(-P[2], iz, 1.0f), iz);
  const float xp = P[0] * iz, yp = P[1] * iz;
  const float r2 = xp * xp + yp * yp;
  const float d = 1.0f + r2 * (K.z + K.w * r2);
  const float dd = K.z + 2.0f * K.w * r2;
  const float du_dx = K.x * (d + 2.0f * xp * xp * dd), du_dy = K.x * (2.0f * xp * yp * dd);
  const float dv_dx = K.y * (2.0f * xp * yp * dd), dv_dy = K.y * (d + 2.0f * yp * yp * dd);
  A0[0] = du_dx * iz;
  A0[1] = du_dy * iz;
  A0[2] = -(du_dx * xp + du_dy * yp) * iz;
  A1[0] = dv_dx * iz;
  A1[1] = dv_dy * iz;
  A1[2] = -(dv_dx * xp + dv_dy * yp) * iz;
}
static size_t mf32_lds_bytes(int E, int NI, int NC) {
  return sizeof(double) * (9 * (size_t)NC + (kMfBlock / 64) * 6 * (size_t)(NC | 1)) +
         sizeof(float) * (12 * (size_t)E + 4 * (size_t)NI + 6 * (size_t)NC) + 2 * sizeof(int) * (size_t)E;
}
// The camera sums: fp64 per-wave LDS atomics (round 3: without them the kernel took 81.5
// against 163.6 us; measured and dropped: fp32 LDS sums, 3x slower, and a copy of the sums
// per half wave, no gain: the atomics are not bank-conflict bound)
__global__ __launch_bounds__(kMfBlock, 4) void k_mf_frame32(DevView v, const double* __restrict__ points,
                                                         const double* __restrict__ camtab,
                                                         const double* __restrict__ scc,
                                                         const double* __restrict__ PU,
                                                         const double* __restrict__ vec, double* __restrict__ out,
                                                         const PcgState* st) {
  extern __shared__ double mf_lds[];
  if (st->status != kPcgRunning) return;
  const int NC6 = 6 * v.NC;
  double* jl_s = mf_lds;                                        // [NC][9] J_l (fp64, applied to the sums)
  // per-wave fp64 camera sums, component-major [waves][6][NCP] with an odd row length: the
  // 64 lanes of one atomic add the same component of their cameras, which then fall in
  // different banks (camera-major [NC][6] put 6 doubles per camera, 16 bank offsets)
  const int NCP = v.NC | 1;
  double* accs = jl_s + 9 * (size_t)v.NC;
  float* rt_s = reinterpret_cast<float*>(accs + (kMfBlock / 64) * 6 * NCP);  // [E][12] R | t
  float* k_s = rt_s + 12 * (size_t)v.E;                         // [NI][4] fx fy k0 k1
  float* dv_s = k_s + 4 * (size_t)v.NI;                         // [NC][6] w~ | dt
  int* sm_s = reinterpret_cast<int*>(dv_s + NC6);               // [E] small-angle tables
  int* col_s = sm_s + v.E;                                      // [E] ext_col
  for (int i = threadIdx.x; i < 12 * v.E; i += blockDim.x)
    rt_s[i] = (float)camtab[(size_t)kCamTab * (i / 12) + i % 12];
  for (int i = threadIdx.x; i < 4 * v.NI; i += blockDim.x) k_s[i] = (float)v.intr[(size_t)kIntr * (i / 4) + 2 + i % 4];
  for (int e = threadIdx.x; e < v.E; e += blockDim.x) {
    const double* T = camtab + (size_t)kCamTab * e;  // R t Rd Jd
    sm_s[e] = (T[12] == 1.0 && T[13] == 0.0 && T[14] == 0.0 && T[15] == 0.0 && T[16] == 1.0 && T[17] == 0.0 &&
               T[18] == 0.0 && T[19] == 0.0 && T[20] == 1.0)
                  ? 1
                  : 0;
    const int c = v.ext_col[e];
    col_s[e] = c;
    if (c < 0) continue;
    double J[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int cc = 0; cc < 3; ++cc)
        J[3 * r + cc] = T[12 + 3 * r] * T[21 + cc] + T[12 + 3 * r + 1] * T[24 + cc] + T[12 + 3 * r + 2] * T[27 + cc];
    double d[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) d[k] = scc[6 * c + k] * vec[6 * c + k];
#pragma unroll
    for (int r = 0; r < 3; ++r) dv_s[6 * c + r] = (float)(J[3 * r] * d[0] + J[3 * r + 1] * d[1] + J[3 * r + 2] * d[2]);
#pragma unroll
    for (int k = 3; k < 6; ++k) dv_s[6 * c + k] = (float)d[k];
#pragma unroll
    for (int k = 0; k < 9; ++k) jl_s[9 * c + k] = J[k];
  }
  for (int i = threadIdx.x; i < (kMfBlock / 64) * 6 * NCP; i += blockDim.x) accs[i] = 0.0;
  __syncthreads();
  double* acc = accs + (threadIdx.x >> 6) * 6 * NCP;
#ifdef DAB_ABL_MF_NOSUMS
  double mf_sink = 0.0;  // kept live (a store no run takes) so the sums' arithmetic stays
  struct SinkGuard {
    double& s;
    double* o;
    __device__ ~SinkGuard() {
      if (s == -1.25e300) o[0] = s;
    }
  } sink_guard{mf_sink, out};
#endif
  auto add = [&](int c, int a, float x) {
    MF_LDS_ADD(acc + a * NCP + c, (double)x);  // fp64 per-wave sums
  };
  auto sum_of = [&](int c, int a) {  // fixed order over the waves
    double t = accs[a * NCP + c];
#pragma unroll
    for (int w = 1; w < kMfBlock / 64; ++w) t += accs[(w * 6 + a) * NCP + c];
    return t;
  };
  auto rt = [&](int e, float (&o)[12]) {
    const float4* pp = reinterpret_cast<const float4*>(rt_s + 12 * e);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float4 u = pp[k];
      o[4 * k] = u.x;
      o[4 * k + 1] = u.y;
      o[4 * k + 2] = u.z;
      o[4 * k + 3] = u.w;
    }
  };
  // one observation's geometry (as k_mf_frame's geo): A (2 x 3), R_a, the rotated-frame
  // points Z of both slots, and vout = R_b vin while the ring table is in registers
  auto geo = [&](const int4 id, const float (&X)[3], float (&A0)[3], float (&A1)[3], float (&Ra)[12],
                 float (&Z0)[3], float (&Z1)[3], bool& comp, const float (&vin)[3], float (&vout)[3]) {
    rt(id.y, Ra);
    const float4 K = *reinterpret_cast<const float4*>(k_s + 4 * id.w);
    comp = id.z >= 0;
    float Q[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) vout[k] = vin[k];
    if (comp) {
      float Tb[12];
      rt(id.z, Tb);
      float RX[3];
      mv3f(Tb, X, RX);
#pragma unroll
      for (int k = 0; k < 3; ++k) Q[k] = RX[k] + Tb[9 + k];
      mv3f(Tb, vin, vout);
      const bool sb = sm_s[id.z] != 0;
#pragma unroll
      for (int k = 0; k < 3; ++k) Z1[k] = sb ? X[k] : RX[k];  // Q - t_b
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k) Q[k] = X[k];
    }
    float RQ[3], P[3];
    mv3f(Ra, Q, RQ);
#pragma unroll
    for (int k = 0; k < 3; ++k) P[k] = RQ[k] + Ra[9 + k];
    const bool sa = sm_s[id.y] != 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) Z0[k] = sa ? Q[k] : RQ[k];  // P - t_a
    proj_jac32(P, K, A0, A1);
  };
  for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < v.NP; p += gridDim.x * blockDim.x) {
    const int sl = p >> 6, lane = p & 63;
    const int off = v.slice_off[sl], len = (v.slice_off[sl + 1] - off) >> 6;
    const float X[3] = {(float)points[3 * (size_t)p], (float)points[3 * (size_t)p + 1],
                        (float)points[3 * (size_t)p + 2]};
    float pu[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) pu[k] = (float)PU[6 * (size_t)p + k];
    // sweep 1: a = sum_e J_p^T (J_c (s_c o v_c))
    float a[3] = {0.0f, 0.0f, 0.0f};
    const float zero3[3] = {0.0f, 0.0f, 0.0f};
    int4 nid = len > 0 ? v.obs_idx[off + lane] : make_int4(-1, 0, -1, 0);
    for (int k = 0; k < len; ++k) {
      const int s = off + 64 * k + lane;
      const int4 id = nid;
      if (k + 1 < len) nid = v.obs_idx[s + 64];
      if (id.x < 0) continue;
      const int c0 = col_s[id.y], c1 = id.z >= 0 ? col_s[id.z] : -1;
      if (c0 < 0 && c1 < 0) continue;
      float A0[3], A1[3], Ra[12], Z0[3], Z1[3], unused[3];
      bool comp;
      geo(id, X, A0, A1, Ra, Z0, Z1, comp, zero3, unused);
      float dP[3] = {0.0f, 0.0f, 0.0f};
      if (c0 >= 0) {
        const float* d = dv_s + 6 * c0;
        const float w[3] = {d[0], d[1], d[2]};
        float cz[3];
        cross3f(Z0, w, cz);
#pragma unroll
        for (int k2 = 0; k2 < 3; ++k2) dP[k2] = d[3 + k2] - cz[k2];
      }
      if (c1 >= 0) {
        const float* d = dv_s + 6 * c1;
        const float w[3] = {d[0], d[1], d[2]};
        float cz[3], r[3], r2[3];
        cross3f(Z1, w, cz);
#pragma unroll
        for (int k2 = 0; k2 < 3; ++k2) r[k2] = d[3 + k2] - cz[k2];
        mv3f(Ra, r, r2);
#pragma unroll
        for (int k2 = 0; k2 < 3; ++k2) dP[k2] += r2[k2];
      }
      const float u0 = A0[0] * dP[0] + A0[1] * dP[1] + A0[2] * dP[2];
      const float u1 = A1[0] * dP[0] + A1[1] * dP[1] + A1[2] * dP[2];
      const float au[3] = {u0 * A0[0] + u1 * A1[0], u0 * A0[1] + u1 * A1[1], u0 * A0[2] + u1 * A1[2]};
      float h[3];
      mtv3f(Ra, au, h);
      if (comp) {
        float Rb[12], h2[3];
        rt(id.z, Rb);
        mtv3f(Rb, h, h2);
#pragma unroll
        for (int k2 = 0; k2 < 3; ++k2) h[k2] = h2[k2];
      }
      a[0] += h[0];
      a[1] += h[1];
      a[2] += h[2];
    }
    const float t0 = pu[0] * a[0], t1 = pu[1] * a[0] + pu[3] * a[1];
    const float t2 = pu[2] * a[0] + pu[4] * a[1] + pu[5] * a[2];
    const float up[3] = {pu[0] * t0 + pu[1] * t1 + pu[2] * t2, pu[3] * t1 + pu[4] * t2, pu[5] * t2};
    // sweep 2: per camera, sum [Z x g | g] (fp64 sums; J_l^T and -s_c after the sums)
    nid = len > 0 ? v.obs_idx[off + lane] : make_int4(-1, 0, -1, 0);
    for (int k = 0; k < len; ++k) {
      const int s = off + 64 * k + lane;
      const int4 id = nid;
      if (k + 1 < len) nid = v.obs_idx[s + 64];
      if (id.x < 0) continue;
      const int c0 = col_s[id.y], c1 = id.z >= 0 ? col_s[id.z] : -1;
      if (c0 < 0 && c1 < 0) continue;
      float A0[3], A1[3], Ra[12], Z0[3], Z1[3], kk[3];
      bool comp;
      geo(id, X, A0, A1, Ra, Z0, Z1, comp, up, kk);
      float m[3];
      mv3f(Ra, kk, m);
      const float z0 = A0[0] * m[0] + A0[1] * m[1] + A0[2] * m[2];
      const float z1 = A1[0] * m[0] + A1[1] * m[1] + A1[2] * m[2];
      const float gz[3] = {z0 * A0[0] + z1 * A1[0], z0 * A0[1] + z1 * A1[1], z0 * A0[2] + z1 * A1[2]};
      if (c0 >= 0) {
        float cz[3];
        cross3f(Z0, gz, cz);
#pragma unroll
        for (int a2 = 0; a2 < 3; ++a2) add(c0, a2, cz[a2]);
#pragma unroll
        for (int a2 = 0; a2 < 3; ++a2) add(c0, 3 + a2, gz[a2]);
      }
      if (c1 >= 0) {
        float hz[3], cz[3];
        mtv3f(Ra, gz, hz);
        cross3f(Z1, hz, cz);
#pragma unroll
        for (int a2 = 0; a2 < 3; ++a2) add(c1, a2, cz[a2]);
#pragma unroll
        for (int a2 = 0; a2 < 3; ++a2) add(c1, 3 + a2, hz[a2]);
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < NC6; i += blockDim.x) {
    const int c = i / 6, k = i - 6 * c;
    double x;
    if (k < 3) {
      x = 0.0;
#pragma unroll
      for (int r = 0; r < 3; ++r) x += jl_s[9 * c + 3 * r + k] * sum_of(c, r);
    } else {
      x = sum_of(c, k);
    }
    out[(size_t)blockIdx.x * NC6 + i] = -scc[i] * x;
  }
}

// Per chunk of camera-major positions (the rig's PCG preconditioner and rhs): 21 upper of
// sum Z Z^T over same-point runs (Z = the run's Y sum, the diagonal block of the Schur term)
// | 6 of -sum Y q_p -> partial[chunk][27]; one lane per run, from a per-chunk run record
// {first position, length, point, camera} so that the point, PU_p and q_p loads leave with
// the record. In the rotated frame (as k_mf_frame; round 5, replacing the Rd | Jd row form
// k_mf_diag_rhs, 733 -> 710 us at C5): a row of J_c is D w with
// D = blockdiag(J_l^T, I) constant per camera and w = [Z x a | a] (slot 0: the projection
// row a, Z = P - t_a or Q on small-angle tables; slot 1: a R_a in place of a, Z = Q - t_b or
// X), so a run's W = D W~ with W~ = sum of w j_p^T, its y = s o (D W~ PU) and
//   sum y y^T = S D (sum Y~ Y~^T) D^T S,   -sum y q = -S D (sum Y~ q),   Y~ = W~ PU:
// the loop sums Y~ Y~^T and Y~ q (27) in the frame, and the chunk's J_l and s_c are applied
// once to the sums (cam_frame_entry). Per entry only R, t (and K) from LDS: no Rd | Jd rows,
// no per-row J_d products, and no s_c in the loop.
// Under a loss the weight needs the residual: the entry's pixel (cm_xy, 16 B per entry) is
// loaded in the non-trivial instantiations only; w and j_p each carry sqrt(rho').
template <int LOSS>
__global__ __launch_bounds__(256) void k_mf_diag_frame(DevView v, int nchunk, const int* __restrict__ run_beg,
                                                       const int4* __restrict__ run_rec,
                                                       const double* __restrict__ points,
                                                       const double* __restrict__ camtab,
                                                       const double* __restrict__ scc, const double* __restrict__ PU,
                                                       const double* __restrict__ q, double* __restrict__ partial) {
  extern __shared__ double mf_lds[];
  double* rt_s = mf_lds;                         // [E][kRtStride]: R | t
  double* k_s = rt_s + kRtStride * (size_t)v.E;  // [NI][6]
  double* jl_s = k_s + 6 * (size_t)v.NI;        // [NC][9]: J_l per camera column
  int* sm_s = reinterpret_cast<int*>(jl_s + 9 * (size_t)v.NC);  // [E] small-angle tables
  __shared__ double wsum[kRedBlock / 64][27];
  for (int i = threadIdx.x; i < 12 * v.E; i += blockDim.x)
    rt_s[kRtStride * (i / 12) + i % 12] = camtab[(size_t)kCamTab * (i / 12) + i % 12];
  for (int i = threadIdx.x; i < 6 * v.NI; i += blockDim.x) k_s[i] = v.intr[(size_t)kIntr * (i / 6) + i % 6];
  for (int e = threadIdx.x; e < v.E; e += blockDim.x) {
    const double* T = camtab + (size_t)kCamTab * e;
    sm_s[e] = (T[12] == 1.0 && T[13] == 0.0 && T[14] == 0.0 && T[15] == 0.0 && T[16] == 1.0 && T[17] == 0.0 &&
               T[18] == 0.0 && T[19] == 0.0 && T[20] == 1.0)
                  ? 1
                  : 0;
    const int c = v.ext_col[e];
    if (c < 0) continue;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int cc = 0; cc < 3; ++cc)
        jl_s[9 * c + 3 * r + cc] =
            T[12 + 3 * r] * T[21 + cc] + T[12 + 3 * r + 1] * T[24 + cc] + T[12 + 3 * r + 2] * T[27 + cc];
  }
  __syncthreads();
  const SmallTabs tabs{nullptr, k_s};
  auto rt = [&](int e, double (&o)[12]) {
    const double2* pp = reinterpret_cast<const double2*>(rt_s + kRtStride * e);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const double2 u = pp[k];
      o[2 * k] = u.x;
      o[2 * k + 1] = u.y;
    }
  };
  for (int c = blockIdx.x; c < nchunk; c += gridDim.x) {
    const int b = run_beg[c], e = run_beg[c + 1];
    const int cam = b < e ? __builtin_amdgcn_readfirstlane(run_rec[b].w) : 0;  // the chunk's camera column
    double acc[27];
#pragma unroll
    for (int i = 0; i < 27; ++i) acc[i] = 0.0;
    for (int k = b + threadIdx.x; k < e; k += blockDim.x) {
      const int4 rr = run_rec[k];
      const int i = rr.x, len = rr.y, p = rr.z;
      const double X[3] = {points[3 * (size_t)p], points[3 * (size_t)p + 1], points[3 * (size_t)p + 2]};
      const double* pu = PU + 6 * (size_t)p;
      const double u00 = pu[0], u01 = pu[1], u02 = pu[2], u11 = pu[3], u12 = pu[4], u22 = pu[5];
      const double q0 = q[4 * (size_t)p], q1 = q[4 * (size_t)p + 1], q2 = q[4 * (size_t)p + 2];
      double y[18];  // W~ (6 x 3), then Y~ = W~ PU in place
#pragma unroll
      for (int t = 0; t < 18; ++t) y[t] = 0.0;
      for (int j = 0; j < len; ++j) {
        int4 id = v.cm_idx[i + j];
        const bool slot1 = (id.w & kSlotBit) != 0;
        id.w &= ~kSlotBit;
        const bool comp = id.z >= 0;
        double Ta[12], Kr[6], Qp[3], Zb[3], Rb[9];
        rt(id.y, Ta);
        tabs.k(id.w, Kr);
        if (comp) {
          double Tb[12];
          rt(id.z, Tb);
          matvec_add(Tb, X, Tb + 9, Qp);
          const bool sb = sm_s[id.z] != 0;
#pragma unroll
          for (int t = 0; t < 3; ++t) Zb[t] = sb ? X[t] : Qp[t] - Tb[9 + t];
#pragma unroll
          for (int t = 0; t < 9; ++t) Rb[t] = Tb[t];
        } else {
#pragma unroll
          for (int t = 0; t < 3; ++t) Qp[t] = Zb[t] = X[t];
        }
        double P[3];
        matvec_add(Ta, Qp, Ta + 9, P);
        const bool sa = sm_s[id.y] != 0;
        double Z[3];
#pragma unroll
        for (int t = 0; t < 3; ++t) Z[t] = slot1 ? Zb[t] : (sa ? Qp[t] : P[t] - Ta[9 + t]);
        Proj pr;
        if constexpr (LOSS == DAB_LOSS_TRIVIAL) {
          project(P, Kr, 0.0, 0.0, pr, true);
        } else {
          const double2 xy = v.cm_xy[i + j];
          project<LOSS>(P, Kr, xy.x, xy.y, pr, true, loss_of(v));
        }
#pragma unroll
        for (int row = 0; row < 2; ++row) {
          const double* a = row == 0 ? pr.A0 : pr.A1;
          const double ar[3] = {a[0], a[1], a[2]};
          double ja[3];  // a R_a
          mtv3(Ta, ar, ja);
          double jp[3];  // j_p = a R_a R_b (or a R_a)
          if (comp) {
            mtv3(Rb, ja, jp);
          } else {
#pragma unroll
            for (int t = 0; t < 3; ++t) jp[t] = ja[t];
          }
          double g[3];
#pragma unroll
          for (int t = 0; t < 3; ++t) g[t] = slot1 ? ja[t] : ar[t];
          double w[6];
          cross3(Z, g, *reinterpret_cast<double(*)[3]>(w));
#pragma unroll
          for (int t = 0; t < 3; ++t) w[3 + t] = g[t];
#pragma unroll
          for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int t = 0; t < 3; ++t) y[3 * r + t] = fma(w[r], jp[t], y[3 * r + t]);
        }
      }
#pragma unroll
      for (int r = 0; r < 6; ++r) {  // Y~ = W~ PU, PU upper triangular (00 01 02 11 12 22)
        const double w0 = y[3 * r], w1 = y[3 * r + 1], w2 = y[3 * r + 2];
        y[3 * r] = w0 * u00;
        y[3 * r + 1] = w0 * u01 + w1 * u11;
        y[3 * r + 2] = w0 * u02 + w1 * u12 + w2 * u22;
      }
#pragma unroll
      for (int a = 0; a < 6; ++a) acc[21 + a] -= y[3 * a] * q0 + y[3 * a + 1] * q1 + y[3 * a + 2] * q2;
      int t = 0;
#pragma unroll
      for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int bb = a; bb < 6; ++bb)
          acc[t++] += y[3 * a] * y[3 * bb] + y[3 * a + 1] * y[3 * bb + 1] + y[3 * a + 2] * y[3 * bb + 2];
    }
    wave_sums_transposed<27>(acc, wsum[threadIdx.x >> 6]);
    __syncthreads();
    if (threadIdx.x < 27) {
      double t = wsum[0][threadIdx.x];
#pragma unroll
      for (int w = 1; w < kRedBlock / 64; ++w) t += wsum[w][threadIdx.x];
      wsum[0][threadIdx.x] = t;
    }
    __syncthreads();
    if (threadIdx.x < 27) {
      const int k = threadIdx.x;
      int ia = 0, ib = 0;  // the entry's (row, column), or (row, -) of the 6 q terms
      if (k >= 21) {
        ia = k - 21;
      } else {
        int r = k;
        while (r >= 6 - ia) {
          r -= 6 - ia;
          ++ia;
        }
        ib = ia + r;
      }
      const double f = k >= 21 ? scc[6 * cam + ia] : scc[6 * cam + ia] * scc[6 * cam + ib];
      partial[27 * (size_t)c + k] = f * cam_frame_entry(wsum[0], jl_s + 9 * cam, k);
    }
    __syncthreads();  // wsum is reused by the next chunk
  }
}

int mf_grid(int NP, int ncu) { return std::max(1, std::min((NP + kMfBlock - 1) / kMfBlock, 4 * ncu)); }
void launch_mf_product(hipStream_t s, const DevView& v, const double* points, const double* camtab,
                       const double* scale_c, const double* PU, const double* vec, double* partial, double* w,
                       int grid, const PcgState* st) {
  DAB_LOSS_SWITCH(v.loss, k_mf_frame<0, LOSS><<<grid, kMfBlock, mf2_lds_bytes(v.E, v.NI, v.NC, true), s>>>(
                              v, points, camtab, scale_c, PU, vec, nullptr, partial, st));
  if (w) launch_pcg_fused_final(s, grid, 6 * v.NC, partial, w, st);
}
void launch_mf_product32(hipStream_t s, const DevView& v, const double* points, const double* camtab,
                         const double* scale_c, const double* PU, const double* vec, double* partial, double* w,
                         int grid, const PcgState* st) {
  k_mf_frame32<<<grid, kMfBlock, mf32_lds_bytes(v.E, v.NI, v.NC), s>>>(v, points, camtab, scale_c, PU, vec, partial,
                                                                      st);
  if (w) launch_pcg_fused_final(s, grid, 6 * v.NC, partial, w, st);
}
void launch_mf_backsub(hipStream_t s, const DevView& v, const double* points, const double* camtab,
                       const double* scale_c, const double* PU, const double* q, const double* yc, double* dp,
                       int grid) {
  DAB_LOSS_SWITCH(v.loss, k_mf_frame<1, LOSS><<<grid, kMfBlock, mf2_lds_bytes(v.E, v.NI, v.NC, false), s>>>(
                              v, points, camtab, scale_c, PU, yc, q, dp, nullptr));
}
void launch_mf_diag_rhs(hipStream_t s, const DevView& v, int nchunk, const int* run_beg, const int4* run_rec,
                        const double* points, const double* camtab, const double* scale_c, const double* PU,
                        const double* q, double* partial) {
  if (nchunk <= 0) return;
  // persistent blocks: the tables are staged once per block, not once per chunk (they fit:
  // NC <= E, so 14 E + 6 NI + 9 NC doubles stay below the 30 E + 6 NI of small_tabs_fit)
  const size_t lds =
      sizeof(double) * (kRtStride * (size_t)v.E + 6 * (size_t)v.NI + 9 * (size_t)v.NC) + sizeof(int) * (size_t)v.E;
  DAB_LOSS_SWITCH(v.loss, k_mf_diag_frame<LOSS><<<std::min(nchunk, kSmallGrid), 256, lds, s>>>(
                              v, nchunk, run_beg, run_rec, points, camtab, scale_c, PU, q, partial));
}

void launch_backsub(hipStream_t s, const DevView& v, const double* PU, const double* q, YBufs Y,
                    const double* yc, double* delta_p) {
  if (v.NP <= 0) return;
  const int g = grid_for(v.NP, 256, 1 << 20);
  if (Y.f32) k_backsub<float><<<g, 256, 0, s>>>(v, PU, q, (const float*)Y.pm, yc, delta_p);
  else k_backsub<double><<<g, 256, 0, s>>>(v, PU, q, (const double*)Y.pm, yc, delta_p);
}

__global__ __launch_bounds__(256) void k_axpy_points(int NP, const double* __restrict__ x,
                                                     const double* __restrict__ d,
                                                     double* __restrict__ xc, double* __restrict__ partial) {
  double acc[2] = {0.0, 0.0};
  const size_t NPs = (size_t)NP;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < 3 * NP; i += gridDim.x * blockDim.x) {
    const int p = i / 3, k = i - 3 * (i / 3);
    const double xv = x[i];
    const double c = xv + d[k * NPs + p];
    xc[i] = c;
    const double dd = xv - c;
    acc[0] += dd * dd;
    acc[1] += c * c;
  }
  block_reduce_store<2>(acc, partial + 2 * (size_t)blockIdx.x);
}

void launch_axpy_points(hipStream_t s, int NP, const double* x, const double* d, double* xc,
                        double* partial, int grid) {
  k_axpy_points<<<grid, 256, 0, s>>>(NP, x, d, xc, partial);
}

__global__ void k_cam_candidate(int E, const int* __restrict__ ext_col, const double* __restrict__ ext,
                                const double* __restrict__ yc, const double* __restrict__ scc,
                                double* __restrict__ ext_c, double* __restrict__ dc) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 6 * E) return;
  const int e = t / 6, k = t - 6 * (t / 6);
  const int c = ext_col[e];
  if (c >= 0 && yc) {
    const double d = -yc[6 * c + k] * scc[6 * c + k];
    ext_c[t] = ext[t] + d;
    dc[6 * c + k] = d;
  } else {
    ext_c[t] = ext[t];
  }
}

void launch_cam_candidate(hipStream_t s, int E, const int* ext_col, const double* ext, const double* yc,
                          const double* scale_c, double* ext_c, double* delta_c) {
  if (E <= 0) return;
  k_cam_candidate<<<grid_for(6 * E, 256, 1 << 20), 256, 0, s>>>(E, ext_col, ext, yc, scale_c, ext_c, delta_c);
}

// Model cost change -(J delta).(r + J delta / 2) and the candidate residual at x + delta
// in one observation pass; J and r at x are re-evaluated (bitwise what the evaluation
// pass saw), the candidate point is formed as x + delta exactly as k_axpy_points does.
// Under a loss: m and r are those of the scaled rows, and the candidate's term is rho(s_c).
template <bool SMALL, int LOSS = DAB_LOSS_TRIVIAL>
__global__ __launch_bounds__(256) void k_candidate(DevView v, const double* __restrict__ points,
                                                   const double* __restrict__ camtab,
                                                   const double* __restrict__ dp,
                                                   const double* __restrict__ dc,
                                                   const double* __restrict__ camtab_c,
                                                   double* __restrict__ partial) {
  extern __shared__ double tabs_lds[];
  SmallTabs st{nullptr, nullptr};
  SmallTabs stc{nullptr, nullptr};  // R, t at x + delta (rt() only) in its own LDS region
  if constexpr (SMALL) {
    double* tc = tabs_lds + 30 * (size_t)v.E + 6 * (size_t)v.NI;
    for (int i = threadIdx.x; i < 30 * v.E; i += blockDim.x)
      tc[i] = camtab_c[(size_t)kCamTab * (i / 30) + i % 30];
    st = stage_small_tabs(tabs_lds, v.E, v.NI, camtab, v.intr);  // barrier inside
    stc = SmallTabs{tc, st.k_s};
  }
  double acc[3] = {0.0, 0.0, 0.0};
  const size_t NPs = (size_t)v.NP;
  for (int s = blockIdx.x * blockDim.x + threadIdx.x; s < v.N; s += gridDim.x * blockDim.x) {
    const int4 id = v.obs_idx[s];
    if (id.x < 0) continue;  // padding slot
    const double2 xy = v.obs_xy[s];
    const double X[3] = {points[3 * (size_t)id.x], points[3 * (size_t)id.x + 1], points[3 * (size_t)id.x + 2]};
    const double d3[3] = {dp[id.x], dp[NPs + id.x], dp[2 * NPs + id.x]};
    double m0 = 0.0, m1 = 0.0, ru, rv;
    {
      ObsJac o;
      if constexpr (SMALL) obs_jacobian_t<LOSS>(id, xy, X, st, o, loss_of(v));
      else obs_jacobian_t<LOSS>(id, xy, X, GlobalTabs{camtab, v.intr}, o, loss_of(v));
      ru = o.pr.ru;
      rv = o.pr.rv;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        m0 += o.jx0[c] * d3[c];
        m1 += o.jx1[c] * d3[c];
      }
      const int c0 = v.ext_col[id.y];
      if (c0 >= 0) {
        const double* d = dc + 6 * c0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          m0 += o.jw0a[k] * d[k];
          m1 += o.jw0b[k] * d[k];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          m0 += o.pr.A0[k] * d[3 + k];
          m1 += o.pr.A1[k] * d[3 + k];
        }
      }
      const int c1 = id.z >= 0 ? v.ext_col[id.z] : -1;
      if (c1 >= 0) {
        const double* d = dc + 6 * c1;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          m0 += o.jw1a[k] * d[k];
          m1 += o.jw1b[k] * d[k];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          m0 += o.jt1a[k] * d[3 + k];
          m1 += o.jt1b[k] * d[3 + k];
        }
      }
    }
    acc[0] += -(m0 * (ru + m0 / 2.0) + m1 * (rv + m1 / 2.0));
    // candidate residual at (x + delta)
    const double Xc[3] = {X[0] + d3[0], X[1] + d3[1], X[2] + d3[2]};
    double T0[12], Kc[6];
    if constexpr (SMALL) {
      stc.rt(id.y, T0);
      stc.k(id.w, Kc);
    } else {
      load_tab<12>(camtab_c, id.y, T0);
      load_intr(v.intr, id.w, Kc);
    }
    double P[3];
    if (id.z >= 0) {
      double T1[12], P2[3];
      if constexpr (SMALL) stc.rt(id.z, T1);
      else load_tab<12>(camtab_c, id.z, T1);
      matvec_add(T1, Xc, T1 + 9, P2);
      matvec_add(T0, P2, T0 + 9, P);
    } else {
      matvec_add(T0, Xc, T0 + 9, P);
    }
    Proj pc;
    project<LOSS>(P, Kc, xy.x, xy.y, pc, false, loss_of(v));
    if constexpr (LOSS == DAB_LOSS_TRIVIAL) acc[1] += pc.ru * pc.ru + pc.rv * pc.rv;
    else acc[1] += pc.rho;
    acc[2] += (isfinite(pc.ru) && isfinite(pc.rv)) ? 0.0 : 1.0;
  }
  block_reduce_store<3>(acc, partial + 3 * (size_t)blockIdx.x);
}

// k_candidate for staged tables in the rotated frame (as k_mf_frame sweep 1): the model
// change m = A dP with dP = dt_a - Z_a x w~_a + R_a (R_b dp_X + dt_r - Z_r x w~_r) and
// w~ = J_l dw once per camera, instead of building every row of the observation; the
// candidate residual as k_candidate. LDS: R, t at x | R, t at x + delta | K | small-angle
// flags | [w~ | dt] per camera.
template <int LOSS>
__global__ __launch_bounds__(256) void k_candidate_frame(DevView v, const double* __restrict__ points,
                                                         const double* __restrict__ camtab,
                                                         const double* __restrict__ dp,
                                                         const double* __restrict__ dc,
                                                         const double* __restrict__ camtab_c,
                                                         double* __restrict__ partial) {
  extern __shared__ double cf_lds[];
  double* rt_s = cf_lds;
  double* rtc_s = rt_s + kRtStride * (size_t)v.E;  // rows padded (bank quads, see kRtStride)
  double* k_s = rtc_s + kRtStride * (size_t)v.E;
  double* dv_s = k_s + 6 * (size_t)v.NI;
  int* sm_s = reinterpret_cast<int*>(dv_s + 6 * (size_t)v.NC);
  for (int i = threadIdx.x; i < 12 * v.E; i += blockDim.x) {
    rt_s[kRtStride * (i / 12) + i % 12] = camtab[(size_t)kCamTab * (i / 12) + i % 12];
    rtc_s[kRtStride * (i / 12) + i % 12] = camtab_c[(size_t)kCamTab * (i / 12) + i % 12];
  }
  for (int i = threadIdx.x; i < 6 * v.NI; i += blockDim.x) k_s[i] = v.intr[(size_t)kIntr * (i / 6) + i % 6];
  for (int e = threadIdx.x; e < v.E; e += blockDim.x) {
    const double* T = camtab + (size_t)kCamTab * e;
    sm_s[e] = (T[12] == 1.0 && T[13] == 0.0 && T[14] == 0.0 && T[15] == 0.0 && T[16] == 1.0 && T[17] == 0.0 &&
               T[18] == 0.0 && T[19] == 0.0 && T[20] == 1.0)
                  ? 1
                  : 0;
    const int c = v.ext_col[e];
    if (c < 0) continue;
    const double* d = dc + 6 * c;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      double w = 0.0;
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        const double jl = T[12 + 3 * r] * T[21 + q] + T[12 + 3 * r + 1] * T[24 + q] + T[12 + 3 * r + 2] * T[27 + q];
        w += jl * d[q];
      }
      dv_s[6 * c + r] = w;
      dv_s[6 * c + 3 + r] = d[3 + r];
    }
  }
  __syncthreads();
  const SmallTabs tk{nullptr, k_s};
  auto rt = [&](const double* base, int e, double (&o)[12]) {
    const double2* pp = reinterpret_cast<const double2*>(base + kRtStride * e);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const double2 u = pp[k];
      o[2 * k] = u.x;
      o[2 * k + 1] = u.y;
    }
  };
  double acc[3] = {0.0, 0.0, 0.0};
  const size_t NPs = (size_t)v.NP;
  for (int s = blockIdx.x * blockDim.x + threadIdx.x; s < v.N; s += gridDim.x * blockDim.x) {
    const int4 id = v.obs_idx[s];
    if (id.x < 0) continue;  // padding slot
    const double2 xy = v.obs_xy[s];
    const double X[3] = {points[3 * (size_t)id.x], points[3 * (size_t)id.x + 1], points[3 * (size_t)id.x + 2]};
    const double d3[3] = {dp[id.x], dp[NPs + id.x], dp[2 * NPs + id.x]};
    double Kr[6];
    tk.k(id.w, Kr);
    double m0, m1, ru, rv;
    {
      double Ta[12];
      rt(rt_s, id.y, Ta);
      const bool comp = id.z >= 0;
      double Q[3], inner[3];  // inner: R_b dp_X (+ the ring term), rotated by R_a below
      if (comp) {
        double Tb[12];
        rt(rt_s, id.z, Tb);
        matvec_add(Tb, X, Tb + 9, Q);
        mv3(Tb, d3, inner);
        const int c1 = v.ext_col[id.z];
        if (c1 >= 0) {
          const bool sb = sm_s[id.z] != 0;
          double Z1[3], cz[3];
#pragma unroll
          for (int k = 0; k < 3; ++k) Z1[k] = sb ? X[k] : Q[k] - Tb[9 + k];
          const double* d = dv_s + 6 * c1;
          const double w[3] = {d[0], d[1], d[2]};
          cross3(Z1, w, cz);
#pragma unroll
          for (int k = 0; k < 3; ++k) inner[k] += d[3 + k] - cz[k];
        }
      } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          Q[k] = X[k];
          inner[k] = d3[k];
        }
      }
      double P[3], dP[3];
      matvec_add(Ta, Q, Ta + 9, P);
      mv3(Ta, inner, dP);
      const int c0 = v.ext_col[id.y];
      if (c0 >= 0) {
        const bool sa = sm_s[id.y] != 0;
        double Z0[3], cz[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) Z0[k] = sa ? Q[k] : P[k] - Ta[9 + k];
        const double* d = dv_s + 6 * c0;
        const double w[3] = {d[0], d[1], d[2]};
        cross3(Z0, w, cz);
#pragma unroll
        for (int k = 0; k < 3; ++k) dP[k] += d[3 + k] - cz[k];
      }
      Proj pr;
      project<LOSS>(P, Kr, xy.x, xy.y, pr, true, loss_of(v));
      ru = pr.ru;
      rv = pr.rv;
      m0 = pr.A0[0] * dP[0] + pr.A0[1] * dP[1] + pr.A0[2] * dP[2];
      m1 = pr.A1[0] * dP[0] + pr.A1[1] * dP[1] + pr.A1[2] * dP[2];
    }
    acc[0] += -(m0 * (ru + m0 / 2.0) + m1 * (rv + m1 / 2.0));
    // candidate residual at (x + delta)
    const double Xc[3] = {X[0] + d3[0], X[1] + d3[1], X[2] + d3[2]};
    double T0[12];
    rt(rtc_s, id.y, T0);
    double P[3];
    if (id.z >= 0) {
      double T1[12], P2[3];
      rt(rtc_s, id.z, T1);
      matvec_add(T1, Xc, T1 + 9, P2);
      matvec_add(T0, P2, T0 + 9, P);
    } else {
      matvec_add(T0, Xc, T0 + 9, P);
    }
    Proj pc;
    project<LOSS>(P, Kr, xy.x, xy.y, pc, false, loss_of(v));
    if constexpr (LOSS == DAB_LOSS_TRIVIAL) acc[1] += pc.ru * pc.ru + pc.rv * pc.rv;
    else acc[1] += pc.rho;
    acc[2] += (isfinite(pc.ru) && isfinite(pc.rv)) ? 0.0 : 1.0;
  }
  block_reduce_store<3>(acc, partial + 3 * (size_t)blockIdx.x);
}

void launch_candidate(hipStream_t s, const DevView& v, const double* points, const double* camtab,
                      const double* delta_p, const double* delta_c, const double* camtab_c, double* partial,
                      int grid) {
  if (small_tabs_fit(v.E, v.NI)) {
    const size_t lds = sizeof(double) * (2 * kRtStride * (size_t)v.E + 6 * (size_t)v.NI + 6 * (size_t)v.NC) +
                       sizeof(int) * (size_t)v.E;
    DAB_LOSS_SWITCH(v.loss, k_candidate_frame<LOSS><<<grid, 256, lds, s>>>(v, points, camtab, delta_p, delta_c,
                                                                          camtab_c, partial));
  } else {
    DAB_LOSS_SWITCH(v.loss, k_candidate<false, LOSS><<<grid, 256, 0, s>>>(v, points, camtab, delta_p, delta_c,
                                                                         camtab_c, partial));
  }
}

__global__ __launch_bounds__(256) void k_grad_points(int NP, const double* __restrict__ x,
                                                     const double* __restrict__ g,
                                                     double* __restrict__ partial) {
  double acc[3] = {0.0, 0.0, 0.0};
  const size_t NPs = (size_t)NP;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < 3 * NP; i += gridDim.x * blockDim.x) {
    const int p = i / 3, k = i - 3 * (i / 3);
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

void launch_grad_points(hipStream_t s, int NP, const double* x, const double* g, double* partial,
                        int grid) {
  k_grad_points<<<grid, 256, 0, s>>>(NP, x, g, partial);
}

// ------------------------------------------------------------------------------------
// Free intrinsics (dab_set_intrinsics_free): the block z of six slots (cx, cy, f0, f1, k0,
// k1) per free intrinsic beside the cameras in the exact Schur step. Every kernel here
// re-evaluates the observation's rows through obs_jacobian_t / project, so residual, point
// and camera rows are those of the evaluation pass; the intrinsic rows come from intr_rows.
// All sums: one owner thread per output element and a fixed order, no floating-point atomics.
// ------------------------------------------------------------------------------------
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

// dab_eval_intrinsic_jacobians: raw rows per slot, J[s][2][6]; columns of scalars the intrinsic
// does not have (meta bits 8..13) are zero
__global__ __launch_bounds__(256) void k_intr_jac(DevView v, const double* __restrict__ points,
                                                  const double* __restrict__ camtab, const int2* __restrict__ meta,
                                                  double* __restrict__ J) {
  const GlobalTabs tb{camtab, v.intr};
  for (int s = blockIdx.x * blockDim.x + threadIdx.x; s < v.N; s += gridDim.x * blockDim.x) {
    const int4 id = v.obs_idx[s];
    if (id.x < 0) continue;  // padding slot
    const double2 xy = v.obs_xy[s];
    const double X[3] = {points[3 * (size_t)id.x], points[3 * (size_t)id.x + 1], points[3 * (size_t)id.x + 2]};
    double P[3], K[6], z0[6], z1[6];
    obs_cam_point(id, X, tb, P);
    tb.k(id.w, K);
    const int m = meta[id.w].y;
    intr_rows<DAB_LOSS_TRIVIAL>(P, K, xy.x, xy.y, LossK{}, (m >> 8) & 63, ((m >> 16) & 1) != 0, z0, z1);
    double* o = J + 12 * (size_t)s;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      o[a] = z0[a];
      o[6 + a] = z1[a];
    }
  }
}
void launch_intr_jac(hipStream_t s, const DevView& v, const double* points, const double* camtab, const int2* meta,
                     double* J) {
  if (v.N <= 0) return;
  k_intr_jac<<<grid_for(v.N, 256, 1 << 20), 256, 0, s>>>(v, points, camtab, meta, J);
}

// Per free intrinsic [U_zz upper 21 | g_z 6 | observation count] of the (scaled) rows at x:
// a work-group stages the 28 values of 256 slots in LDS, thread (free intrinsic, k) adds the
// slots of its intrinsic in slot order -> partial[group][nfi][28], then a fixed-order sum over groups
template <int LOSS>
__global__ __launch_bounds__(256) void k_intr_eval(DevView v, const double* __restrict__ points,
                                                   const double* __restrict__ camtab,
                                                   const int2* __restrict__ meta, int nfi,
                                                   double* __restrict__ partial) {
  __shared__ double val_s[256][kIntrRec + 1];
  __shared__ int col_s[256];
  static_assert(sizeof(double) * 256 * (kIntrRec + 1) + sizeof(int) * 256 <= 64 * 1024, "k_intr_eval: static LDS");
  const GlobalTabs tb{camtab, v.intr};
  const LossK lk = loss_of(v);
  const int K = nfi * kIntrRec;
  double acc[2] = {0.0, 0.0};  // elements tid and tid + 256 (K <= kIntrFreeMax * 28 = 448)
  for (int s0 = blockIdx.x * 256; s0 < v.N; s0 += gridDim.x * 256) {
    const int s = s0 + threadIdx.x;
    int col = -1;
    if (s < v.N) {
      const int4 id = v.obs_idx[s];
      if (id.x >= 0) {
        const int2 mt = meta[id.w];
        col = mt.x;
        if (col >= 0) {
          const double2 xy = v.obs_xy[s];
          const double X[3] = {points[3 * (size_t)id.x], points[3 * (size_t)id.x + 1], points[3 * (size_t)id.x + 2]};
          // the (scaled) residual only: no point or camera rows
          double ru, rv, rho;
          obs_rows_l<LOSS, false, -1>(lk, rho, id, xy, X, tb, ru, rv, nullptr, nullptr, nullptr, nullptr);
          double P[3], Kr[6], z0[6], z1[6];
          obs_cam_point(id, X, tb, P);
          tb.k(id.w, Kr);
          intr_rows<LOSS>(P, Kr, xy.x, xy.y, lk, mt.y & 63, ((mt.y >> 16) & 1) != 0, z0, z1);
          double* o28 = val_s[threadIdx.x];
          int q = 0;
#pragma unroll
          for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = a; b < 6; ++b) o28[q++] = z0[a] * z0[b] + z1[a] * z1[b];
#pragma unroll
          for (int a = 0; a < 6; ++a) o28[21 + a] = z0[a] * ru + z1[a] * rv;
          o28[27] = 1.0;
        }
      }
    }
    col_s[threadIdx.x] = col;
    __syncthreads();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int e = threadIdx.x + 256 * h;
      if (e < K) {
        const int i = e / kIntrRec, k = e - kIntrRec * i;
        double a = acc[h];
        for (int t = 0; t < 256; ++t)
          if (col_s[t] == i) a += val_s[t][k];
        acc[h] = a;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int e = threadIdx.x + 256 * h;
    if (e < K) partial[(size_t)blockIdx.x * K + e] = acc[h];
  }
}
int intr_eval_grid(int N) { return grid_for(N, 256, 512); }
void launch_intr_eval(hipStream_t s, const DevView& v, const double* points, const double* camtab, const int2* meta,
                      int nfi, double* partial, double* zg) {
  if (nfi <= 0) return;
  const int grid = intr_eval_grid(v.N);
  DAB_LOSS_SWITCH(v.loss, k_intr_eval<LOSS><<<grid, 256, 0, s>>>(v, points, camtab, meta, nfi, partial));
  // one thread per element, the groups' partials added in group order
  launch_schur_sum(s, grid, (size_t)nfi * kIntrRec, (size_t)nfi * kIntrRec, partial, zg);
}

// s_z = 1 / (1 + sqrt(diag U_zz)) of the active slots (1 without Jacobi scaling), 0 for the others
__global__ void k_intr_scale(int nfi, const double* __restrict__ zg, const int* __restrict__ act,
                             double* __restrict__ sz, int on) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 6 * nfi) return;
  const int i = t / 6, a = t - 6 * i;
  const int q = a * 6 - (a * (a - 1)) / 2;  // upper-packed index of (a, a)
  const bool active = (act[i] >> a) & 1;
  sz[t] = !active ? 0.0 : (on ? 1.0 / (1.0 + sqrt(zg[kIntrRec * (size_t)i + q])) : 1.0);
}
void launch_intr_scale(hipStream_t s, int nfi, const double* zg, const int* act, double* sz, int on) {
  if (nfi > 0) k_intr_scale<<<1, 128, 0, s>>>(nfi, zg, act, sz, on);
}

// One observation of point p (slot s) for the border kernels: a_o = J_p PU_p -> a_row[6] (rows 0,
// 1), s_c J_c of the free camera slots -> jc_row[24] (slot 0 rows 0, 1 | slot 1 rows 0, 1), s_z J_z
// -> jz_row[12] when its intrinsic is free with index <= zi_max; c0 / c1 / zi = the free camera and
// intrinsic indices or -1 (a padding slot: all -1, nothing written)
template <int LOSS>
__device__ __forceinline__ void border_stage_obs(const DevView& v, const GlobalTabs& tb, const LossK& lk, int s, int p,
                                                 const double* __restrict__ points, const double* __restrict__ PU,
                                                 const double* __restrict__ scc, const double* __restrict__ sz,
                                                 const int2* __restrict__ meta, int zi_max, double* a_row,
                                                 double* jc_row, double* jz_row, int& c0, int& c1, int& zi) {
  c0 = c1 = zi = -1;
  const int4 id = v.obs_idx[s];
  if (id.x < 0) return;
  const double2 xy = v.obs_xy[s];
  const double X[3] = {points[3 * (size_t)p], points[3 * (size_t)p + 1], points[3 * (size_t)p + 2]};
  ObsJac o;
  obs_jacobian_t<LOSS>(id, xy, X, tb, o, lk);
  const double* pu = PU + 6 * (size_t)p;  // upper-packed 00 01 02 11 12 22
  a_row[0] = o.jx0[0] * pu[0];
  a_row[1] = o.jx0[0] * pu[1] + o.jx0[1] * pu[3];
  a_row[2] = o.jx0[0] * pu[2] + o.jx0[1] * pu[4] + o.jx0[2] * pu[5];
  a_row[3] = o.jx1[0] * pu[0];
  a_row[4] = o.jx1[0] * pu[1] + o.jx1[1] * pu[3];
  a_row[5] = o.jx1[0] * pu[2] + o.jx1[1] * pu[4] + o.jx1[2] * pu[5];
  c0 = v.ext_col[id.y];
  c1 = id.z >= 0 ? v.ext_col[id.z] : -1;
  if (c0 >= 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      jc_row[k] = scc[6 * c0 + k] * o.jw0a[k];
      jc_row[3 + k] = scc[6 * c0 + 3 + k] * o.pr.A0[k];
      jc_row[6 + k] = scc[6 * c0 + k] * o.jw0b[k];
      jc_row[9 + k] = scc[6 * c0 + 3 + k] * o.pr.A1[k];
    }
  }
  if (c1 >= 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      jc_row[12 + k] = scc[6 * c1 + k] * o.jw1a[k];
      jc_row[15 + k] = scc[6 * c1 + 3 + k] * o.jt1a[k];
      jc_row[18 + k] = scc[6 * c1 + k] * o.jw1b[k];
      jc_row[21 + k] = scc[6 * c1 + 3 + k] * o.jt1b[k];
    }
  }
  const int2 mt = meta[id.w];
  if (mt.x < 0 || mt.x > zi_max) return;
  zi = mt.x;
  double P[3], Kr[6], z0[6], z1[6];
  obs_cam_point(id, X, tb, P);
  tb.k(id.w, Kr);
  intr_rows<LOSS>(P, Kr, xy.x, xy.y, lk, mt.y & 63, ((mt.y >> 16) & 1) != 0, z0, z1);
#pragma unroll
  for (int a = 0; a < 6; ++a) {
    jz_row[a] = sz[6 * zi + a] * z0[a];
    jz_row[6 + a] = sz[6 * zi + a] * z1[a];
  }
}

// Border of the reduced system, one point at a time per work-group of one wave (a group owns a fixed range
// of SELL slices and its own partial[6 nfi][ldp], ldp = n + 6 nfi + 1: camera columns, z
// columns, rhs). Per point: its observations' rows go to LDS in batches of kIntrBatch
// (a_o = J_p PU_p, s_c J_c of both camera slots, s_z J_z); sweep 0 sums Gz_p,i = sum_o T_o in
// LDS (owner thread per element, observation order); sweep 1 adds, per observation and free
// camera slot, (s_z J_z)^T (s_c J_c) - Gz_p,i Y_e^T into block (i, c) for every free intrinsic i
// of the point, then -Gz_i Gz_j^T (j <= i) and -Gz_i q_p. Element (6 i + a, column) of the
// partial always belongs to the same thread, so its sum has one order.
constexpr int kIntrBatch = 64;   // observations per batch = threads of the work-group (one wave)
constexpr int kIntrBorderThreads = 64;
template <int LOSS>
__global__ __launch_bounds__(kIntrBorderThreads) void k_intr_border_g(DevView v, const double* __restrict__ points,
                                                     const double* __restrict__ camtab,
                                                     const double* __restrict__ scc, const double* __restrict__ PU,
                                                     const double* __restrict__ q, const double* __restrict__ sz,
                                                     const int2* __restrict__ meta, int nfi, int spg,
                                                     double* __restrict__ partial) {
  __shared__ double a_s[kIntrBatch][6];    // a_o rows 0, 1
  __shared__ double jc_s[kIntrBatch][25];  // s_c J_c: slot 0 rows 0, 1 | slot 1 rows 0, 1 (odd stride)
  __shared__ double jz_s[kIntrBatch][13];  // s_z J_z rows 0, 1
  __shared__ int c0_s[kIntrBatch], c1_s[kIntrBatch], zi_s[kIntrBatch];
  __shared__ double gz_s[kIntrFreeMax][18];
  __shared__ int zmask_s;
  const int n = 6 * v.NC, ldp = n + 6 * nfi + 1;
  double* __restrict__ out = partial + (size_t)blockIdx.x * (size_t)(6 * nfi) * ldp;
  const GlobalTabs tb{camtab, v.intr};
  const LossK lk = loss_of(v);
  const int tid = threadIdx.x;
  const int sl_end = min(v.nslice, ((int)blockIdx.x + 1) * spg);
  for (int sl = blockIdx.x * spg; sl < sl_end; ++sl) {
    const int off = v.slice_off[sl], len = (v.slice_off[sl + 1] - off) >> 6;
    const int nb = (len + kIntrBatch - 1) / kIntrBatch;
    for (int lane = 0; lane < 64; ++lane) {
      const int p = 64 * sl + lane;
      if (p >= v.NP) break;
      __syncthreads();
      for (int t = tid; t < kIntrFreeMax * 18; t += kIntrBorderThreads) (&gz_s[0][0])[t] = 0.0;
      if (tid == 0) zmask_s = 0;
      __syncthreads();
      for (int sweep = 0; sweep < 2; ++sweep) {
        for (int b = 0; b < nb; ++b) {
          const int cnt = min(kIntrBatch, len - b * kIntrBatch);
          if (sweep == 0 || nb > 1) {
            __syncthreads();
            if (tid < cnt) {
              const int s = off + 64 * (b * kIntrBatch + tid) + lane;
              int c0, c1, zi;
              border_stage_obs<LOSS>(v, tb, lk, s, p, points, PU, scc, sz, meta, kIntrFreeMax, a_s[tid], jc_s[tid],
                                     jz_s[tid], c0, c1, zi);
              if (zi >= 0) atomicOr(&zmask_s, 1 << zi);
              c0_s[tid] = c0;
              c1_s[tid] = c1;
              zi_s[tid] = zi;
            }
            __syncthreads();
          }
          const int zmask = zmask_s;
          if (sweep == 0) {
            // Gz_i[a][k] += sum_o (s_z J_z)[.][a] a_o[.][k]
            for (int w = tid; w < nfi * 18; w += kIntrBorderThreads) {
              const int i = w / 18, ak = w - 18 * i, a = ak / 3, k = ak - 3 * a;
              if (!((zmask >> i) & 1)) continue;
              double g = gz_s[i][ak];
              for (int o = 0; o < cnt; ++o)
                if (zi_s[o] == i) g += jz_s[o][a] * a_s[o][k] + jz_s[o][6 + a] * a_s[o][3 + k];
              gz_s[i][ak] = g;
            }
          } else {
            for (int w = tid; w < nfi * 36; w += kIntrBorderThreads) {
              const int i = w / 36, ab = w - 36 * i, a = ab / 6, bb = ab - 6 * a;
              if (!((zmask >> i) & 1)) continue;
              const double g0 = gz_s[i][3 * a], g1 = gz_s[i][3 * a + 1], g2 = gz_s[i][3 * a + 2];
              double* row = out + (size_t)(6 * i + a) * ldp;
              for (int o = 0; o < cnt; ++o) {
                const int c0 = c0_s[o], c1 = c1_s[o];
                if (c0 < 0 && c1 < 0) continue;
                const double d0 = g0 * a_s[o][0] + g1 * a_s[o][1] + g2 * a_s[o][2];
                const double d1 = g0 * a_s[o][3] + g1 * a_s[o][4] + g2 * a_s[o][5];
                const bool mine = zi_s[o] == i;
                const double z0 = mine ? jz_s[o][a] : 0.0, z1 = mine ? jz_s[o][6 + a] : 0.0;
                if (c0 >= 0) {
                  const double j0 = jc_s[o][bb], j1 = jc_s[o][6 + bb];
                  row[6 * c0 + bb] += (z0 * j0 + z1 * j1) - (j0 * d0 + j1 * d1);
                }
                if (c1 >= 0) {
                  const double j0 = jc_s[o][12 + bb], j1 = jc_s[o][18 + bb];
                  row[6 * c1 + bb] += (z0 * j0 + z1 * j1) - (j0 * d0 + j1 * d1);
                }
              }
            }
          }
        }
        __syncthreads();  // sweep 0: Gz complete; sweep 1: the LDS rows are free again
      }
      const int zmask = zmask_s;
      if (zmask == 0) continue;
      for (int w = tid; w < nfi * nfi * 36; w += kIntrBorderThreads) {
        const int i = w / (nfi * 36), r = w - i * (nfi * 36), j = r / 36, ab = r - 36 * j, a = ab / 6, bb = ab - 6 * a;
        if (j > i || (j == i && bb > a)) continue;
        if (!((zmask >> i) & 1) || !((zmask >> j) & 1)) continue;
        const double d = gz_s[i][3 * a] * gz_s[j][3 * bb] + gz_s[i][3 * a + 1] * gz_s[j][3 * bb + 1] +
                         gz_s[i][3 * a + 2] * gz_s[j][3 * bb + 2];
        out[(size_t)(6 * i + a) * ldp + n + 6 * j + bb] -= d;
      }
      for (int w = tid; w < nfi * 6; w += kIntrBorderThreads) {
        const int i = w / 6, a = w - 6 * i;
        if (!((zmask >> i) & 1)) continue;
        const double* qp = q + 4 * (size_t)p;
        out[(size_t)(6 * i + a) * ldp + n + 6 * nfi] -=
            gz_s[i][3 * a] * qp[0] + gz_s[i][3 * a + 1] * qp[1] + gz_s[i][3 * a + 2] * qp[2];
      }
    }
  }
}

// Which free intrinsics each point sees (bit i = free intrinsic i): structure only, once per solve
__global__ __launch_bounds__(256) void k_intr_ptmask(DevView v, const int2* __restrict__ meta, int* __restrict__ ptmask) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= v.NP) return;
  const int sl = p >> 6, lane = p & 63;
  const int off = v.slice_off[sl], len = (v.slice_off[sl + 1] - off) >> 6;
  int m = 0;
  for (int k = 0; k < len; ++k) {
    const int4 id = v.obs_idx[off + 64 * k + lane];
    if (id.x < 0) continue;
    const int zi = meta[id.w].x;
    if (zi >= 0) m |= 1 << zi;
  }
  ptmask[p] = m;
}
void launch_intr_ptmask(hipStream_t s, const DevView& v, const int2* meta, int* ptmask) {
  if (v.NP > 0) k_intr_ptmask<<<grid_for(v.NP, 256, 1 << 20), 256, 0, s>>>(v, meta, ptmask);
}

// The same border with the sums in LDS (the six rows of ONE free intrinsic, [6][ldp], fit for the
// small camera sets of the rig): work-group (g, i) of one wave walks the points of group g that see
// free intrinsic i (ptmask), one at a time. Per point: rows to LDS as k_intr_border_g, Gz_j of
// the point's intrinsics j <= i, then lanes (a, b) add, observation by observation, the
// (s_z J_z)^T (s_c J_c) - Gz_i Y_e^T terms of block (i, c), lanes (j, a, b) the -Gz_i Gz_j^T terms
// and lanes a the -Gz_i q_p terms into the LDS rows. Every element has one owner lane and one
// order; the rows leave once, at the end, into partial[g][6 i .. 6 i + 5][ldp]: no global
// read-modify-write per observation (k_intr_border_g at C5: 152 ms of dependent L2 round trips).
constexpr int kIntrBatchL = 32;
template <int LOSS>
__global__ __launch_bounds__(kIntrBorderThreads) void k_intr_border_lds(
    DevView v, const double* __restrict__ points, const double* __restrict__ camtab, const double* __restrict__ scc,
    const double* __restrict__ PU, const double* __restrict__ q, const double* __restrict__ sz,
    const int2* __restrict__ meta, const int* __restrict__ ptmask, int nfi, int spg, double* __restrict__ partial) {
  extern __shared__ double acc_s[];             // [6][ldp]
  __shared__ double a_s[kIntrBatchL][6];    // a_o rows 0, 1
  __shared__ double jc_s[kIntrBatchL][25];  // s_c J_c: slot 0 rows 0, 1 | slot 1 rows 0, 1 (odd stride)
  __shared__ double jz_s[kIntrBatchL][13];  // s_z J_z rows 0, 1
  __shared__ int c0_s[kIntrBatchL], c1_s[kIntrBatchL], zi_s[kIntrBatchL];
  __shared__ double gz_s[kIntrFreeMax][18];
  const int zi0 = blockIdx.y;
  const int n = 6 * v.NC, ldp = n + 6 * nfi + 1;
  const GlobalTabs tb{camtab, v.intr};
  const LossK lk = loss_of(v);
  const int tid = threadIdx.x;
  for (int t = tid; t < 6 * ldp; t += kIntrBorderThreads) acc_s[t] = 0.0;
  __syncthreads();
  const int sl_end = min(v.nslice, ((int)blockIdx.x + 1) * spg);
  for (int sl = blockIdx.x * spg; sl < sl_end; ++sl) {
    const int off = v.slice_off[sl], len = (v.slice_off[sl + 1] - off) >> 6;
    const int nb = (len + kIntrBatchL - 1) / kIntrBatchL;
    const int pl = 64 * sl + tid;
    const int mymask = pl < v.NP ? ptmask[pl] : 0;
    unsigned long long todo = __ballot((mymask >> zi0) & 1);
    while (todo) {
      const int lane = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const int p = 64 * sl + lane;
      const int zmask = __shfl(mymask, lane, 64) & ((2 << zi0) - 1);  // the point's intrinsics j <= i
      __syncthreads();
      for (int t = tid; t < kIntrFreeMax * 18; t += kIntrBorderThreads) (&gz_s[0][0])[t] = 0.0;
      __syncthreads();
      for (int sweep = 0; sweep < 2; ++sweep) {
        for (int b = 0; b < nb; ++b) {
          const int cnt = min(kIntrBatchL, len - b * kIntrBatchL);
          if (sweep == 0 || nb > 1) {
            __syncthreads();
            if (tid < cnt) {
              const int s = off + 64 * (b * kIntrBatchL + tid) + lane;
              int c0, c1, zi;
              border_stage_obs<LOSS>(v, tb, lk, s, p, points, PU, scc, sz, meta, zi0, a_s[tid], jc_s[tid], jz_s[tid],
                                     c0, c1, zi);
              c0_s[tid] = c0;
              c1_s[tid] = c1;
              zi_s[tid] = zi;
            }
            __syncthreads();
          }
          if (sweep == 0) {
            for (int w = tid; w < (zi0 + 1) * 18; w += kIntrBorderThreads) {
              const int i = w / 18, ak = w - 18 * i, a = ak / 3, k = ak - 3 * a;
              if (!((zmask >> i) & 1)) continue;
              double g = gz_s[i][ak];
              for (int o = 0; o < cnt; ++o)
                if (zi_s[o] == i) g += jz_s[o][a] * a_s[o][k] + jz_s[o][6 + a] * a_s[o][3 + k];
              gz_s[i][ak] = g;
            }
          } else if (tid < 36) {
            const int a = tid / 6, bb = tid - 6 * a;
            const double g0 = gz_s[zi0][3 * a], g1 = gz_s[zi0][3 * a + 1], g2 = gz_s[zi0][3 * a + 2];
            double* row = acc_s + a * ldp;
            for (int o = 0; o < cnt; ++o) {
              const int c0 = c0_s[o], c1 = c1_s[o];
              if (c0 < 0 && c1 < 0) continue;
              const double d0 = g0 * a_s[o][0] + g1 * a_s[o][1] + g2 * a_s[o][2];
              const double d1 = g0 * a_s[o][3] + g1 * a_s[o][4] + g2 * a_s[o][5];
              const bool mine = zi_s[o] == zi0;
              const double z0 = mine ? jz_s[o][a] : 0.0, z1 = mine ? jz_s[o][6 + a] : 0.0;
              if (c0 >= 0) {
                const double j0 = jc_s[o][bb], j1 = jc_s[o][6 + bb];
                row[6 * c0 + bb] += (z0 * j0 + z1 * j1) - (j0 * d0 + j1 * d1);
              }
              if (c1 >= 0) {
                const double j0 = jc_s[o][12 + bb], j1 = jc_s[o][18 + bb];
                row[6 * c1 + bb] += (z0 * j0 + z1 * j1) - (j0 * d0 + j1 * d1);
              }
            }
          }
        }
        __syncthreads();  // sweep 0: Gz complete; sweep 1: the LDS rows are free again
      }
      for (int w = tid; w < (zi0 + 1) * 36; w += kIntrBorderThreads) {
        const int j = w / 36, ab = w - 36 * j, a = ab / 6, bb = ab - 6 * a;
        if (!((zmask >> j) & 1) || (j == zi0 && bb > a)) continue;
        acc_s[a * ldp + n + 6 * j + bb] -= gz_s[zi0][3 * a] * gz_s[j][3 * bb] + gz_s[zi0][3 * a + 1] * gz_s[j][3 * bb + 1] +
                                           gz_s[zi0][3 * a + 2] * gz_s[j][3 * bb + 2];
      }
      if (tid < 6) {
        const double* qp = q + 4 * (size_t)p;
        acc_s[tid * ldp + n + 6 * nfi] -=
            gz_s[zi0][3 * tid] * qp[0] + gz_s[zi0][3 * tid + 1] * qp[1] + gz_s[zi0][3 * tid + 2] * qp[2];
      }
    }
  }
  __syncthreads();
  double* __restrict__ out = partial + ((size_t)blockIdx.x * nfi + zi0) * 6 * (size_t)ldp;
  for (int t = tid; t < 6 * ldp; t += kIntrBorderThreads) out[t] = acc_s[t];
}

int intr_border_groups(int nslice, int NC, int nfi, int* spg) {
  const size_t per = sizeof(double) * (size_t)(6 * nfi) * (size_t)(6 * NC + 6 * nfi + 1);
  // one wave per group; the groups' partials are capped at 256 MB
  int g = (int)std::min<size_t>(4096, std::max<size_t>(1, ((size_t)256 << 20) / std::max<size_t>(1, per)));
  g = std::max(1, std::min(g, nslice));
  *spg = (nslice + g - 1) / g;
  return (nslice + *spg - 1) / *spg;
}
// the LDS rows of one free intrinsic fit
bool intr_border_lds_fits(int NC, int nfi) {
  return sizeof(double) * 6 * (size_t)(6 * NC + 6 * nfi + 1) <= 48 * 1024;
}
void launch_intr_border(hipStream_t s, const DevView& v, const double* points, const double* camtab,
                        const double* scale_c, const double* PU, const double* q, const double* sz, const int2* meta,
                        const int* ptmask, int nfi, double* partial, double* bsum, bool allow_lds) {
  if (nfi <= 0 || v.nslice <= 0) return;
  int spg = 1;
  const int groups = intr_border_groups(v.nslice, v.NC, nfi, &spg);
  const int ldp = 6 * v.NC + 6 * nfi + 1;
  const size_t count = (size_t)(6 * nfi) * (size_t)ldp;
  if (allow_lds && intr_border_lds_fits(v.NC, nfi)) {
    const size_t lds = sizeof(double) * 6 * (size_t)ldp;
    DAB_LOSS_SWITCH(v.loss, k_intr_border_lds<LOSS><<<dim3(groups, nfi), kIntrBorderThreads, lds, s>>>(
                                v, points, camtab, scale_c, PU, q, sz, meta, ptmask, nfi, spg, partial));
  } else {
    (void)hipMemsetAsync(partial, 0, sizeof(double) * count * groups, s);
    DAB_LOSS_SWITCH(v.loss, k_intr_border_g<LOSS><<<groups, kIntrBorderThreads, 0, s>>>(v, points, camtab, scale_c, PU, q,
                                                                                       sz, meta, nfi, spg, partial));
  }
  launch_schur_sum(s, groups, count, count, partial, bsum);
}

// Rows n .. n' - 1 of the dense S (lower part) and the rhs tail of row n' from the all-reduced
// border sums, the U_zz part (+ D_z^2) and s_z g_z; an inactive slot gets a unit diagonal
__global__ void k_intr_scatter(int n, int nfi, const double* __restrict__ bsum, const double* __restrict__ zg,
                               const double* __restrict__ sz, const int* __restrict__ act, StepScalars sc,
                               double* __restrict__ S, int lds) {
  const int nz = 6 * nfi, ldp = n + nz + 1;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nz * ldp) return;
  const int r = t / ldp, col = t - r * ldp;
  const int i = r / 6, a = r - 6 * i;
  const bool active = (act[i] >> a) & 1;
  double val = bsum[t];
  if (col < n) {
    S[(size_t)(n + r) * lds + col] = val;
  } else if (col < n + nz) {
    const int cz = col - n;
    if (cz > r) return;  // upper triangle
    const int j = cz / 6, b = cz - 6 * j;
    if (j == i) {
      const int qi = b * 6 - (b * (b - 1)) / 2 + (a - b);  // upper-packed index of (b, a)
      double u = sz[r] * zg[kIntrRec * (size_t)i + qi] * sz[cz];
      if (cz == r) {
        const double d = fmin(fmax(u, sc.min_diag), sc.max_diag);
        const double D = sqrt(d / sc.radius);
        u += D * D;
      }
      val += u;
    }
    if (cz == r && !active) val = 1.0;
    S[(size_t)(n + r) * lds + col] = val;
  } else {
    S[(size_t)(n + nz) * lds + n + r] = active ? sz[r] * zg[kIntrRec * (size_t)i + 21 + a] + val : 0.0;
  }
}
void launch_intr_scatter(hipStream_t s, int n, int nfi, const double* bsum, const double* zg, const double* sz,
                         const int* act, StepScalars sc, double* S, int lds) {
  if (nfi <= 0) return;
  const int count = 6 * nfi * (n + 6 * nfi + 1);
  k_intr_scatter<<<grid_for(count, 256, 1 << 20), 256, 0, s>>>(n, nfi, bsum, zg, sz, act, sc, S, lds);
}

// delta_p += PU_p PU_p^T sum_o J_p,o^T (J_z,o (s_z o y_z)), one thread per point over its SELL slots
template <int LOSS>
__global__ __launch_bounds__(256) void k_intr_backsub(DevView v, const double* __restrict__ points,
                                                      const double* __restrict__ camtab,
                                                      const double* __restrict__ PU, const double* __restrict__ sz,
                                                      const double* __restrict__ yz, const int2* __restrict__ meta,
                                                      double* __restrict__ dp) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= v.NP) return;
  const GlobalTabs tb{camtab, v.intr};
  const LossK lk = loss_of(v);
  const size_t NPs = (size_t)v.NP;
  const int sl = p >> 6, lane = p & 63;
  const int off = v.slice_off[sl], len = (v.slice_off[sl + 1] - off) >> 6;
  const double X[3] = {points[3 * (size_t)p], points[3 * (size_t)p + 1], points[3 * (size_t)p + 2]};
  double t[3] = {0.0, 0.0, 0.0};
  for (int k = 0; k < len; ++k) {
    const int s = off + 64 * k + lane;
    const int4 id = v.obs_idx[s];
    if (id.x < 0) continue;
    const int2 mt = meta[id.w];
    if (mt.x < 0) continue;
    const double2 xy = v.obs_xy[s];
    double ru, rv, jx0[3], jx1[3], rho;
    obs_rows_l<LOSS, true, -1>(lk, rho, id, xy, X, tb, ru, rv, jx0, jx1, nullptr, nullptr);
    double P[3], Kr[6], z0[6], z1[6];
    obs_cam_point(id, X, tb, P);
    tb.k(id.w, Kr);
    intr_rows<LOSS>(P, Kr, xy.x, xy.y, lk, mt.y & 63, ((mt.y >> 16) & 1) != 0, z0, z1);
    double m0 = 0.0, m1 = 0.0;
#pragma unroll
    for (int a = 0; a < 6; ++a) {
      const double y = sz[6 * mt.x + a] * yz[6 * mt.x + a];
      m0 += z0[a] * y;
      m1 += z1[a] * y;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) t[c] += jx0[c] * m0 + jx1[c] * m1;
  }
  const double* pu = PU + 6 * (size_t)p;
  const double u0 = pu[0] * t[0];
  const double u1 = pu[1] * t[0] + pu[3] * t[1];
  const double u2 = pu[2] * t[0] + pu[4] * t[1] + pu[5] * t[2];
  dp[p] += pu[0] * u0 + pu[1] * u1 + pu[2] * u2;
  dp[NPs + p] += pu[3] * u1 + pu[4] * u2;
  dp[2 * NPs + p] += pu[5] * u2;
}
void launch_intr_backsub(hipStream_t s, const DevView& v, const double* points, const double* camtab,
                         const double* PU, const double* sz, const double* yz, const int2* meta, double* dp) {
  if (v.NP <= 0) return;
  DAB_LOSS_SWITCH(v.loss, k_intr_backsub<LOSS><<<grid_for(v.NP, 256, 1 << 20), 256, 0, s>>>(v, points, camtab, PU, sz,
                                                                                           yz, meta, dp));
}

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

// Candidate intrinsics x_z + delta_z (delta_z = -s_z y_z on the active slots; with one focal
// length fy follows fx), delta_z[nfi][6], and out[5] as launch_cam_norms over the active
// scalars: {sum (x - xc)^2, sum xc^2, max |x - (x - g)|, sum (x - (x - g))^2, sum x^2}.
// yz = nullptr: the norms at x only (out[0] = 0, out[1] = out[4]). One thread: <= 96 scalars.
__global__ void k_intr_candidate(int NI, const int2* __restrict__ meta, const double* __restrict__ intr,
                                 const double* __restrict__ sz, const double* __restrict__ yz,
                                 const double* __restrict__ zg, double* __restrict__ intr_c,
                                 double* __restrict__ dz, double* __restrict__ out) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  double a[5] = {0, 0, 0, 0, 0};
  for (int i = 0; i < NI; ++i) {
    const int2 mt = meta[i];
    double K[kIntr];
    for (int k = 0; k < kIntr; ++k) K[k] = intr[(size_t)kIntr * i + k];
    if (mt.x >= 0) {
      for (int k = 0; k < 6; ++k) {
        const bool active = (mt.y >> k) & 1;
        const double x = K[k];
        double xc = x;
        if (yz) {
          const double d = active ? -sz[6 * mt.x + k] * yz[6 * mt.x + k] : 0.0;
          dz[6 * mt.x + k] = d;
          xc = x + d;
          K[k] = xc;
        }
        if (!active) continue;
        const double dd = x - xc;
        a[0] += dd * dd;
        a[1] += xc * xc;
        const double gg = zg ? x - (x + (-zg[kIntrRec * (size_t)mt.x + 21 + k])) : 0.0;
        a[2] = fmax(a[2], fabs(gg));
        a[3] += gg * gg;
        a[4] += x * x;
      }
      if ((mt.y >> 16) & 1) K[3] = K[2];
    }
    if (intr_c)
      for (int k = 0; k < kIntr; ++k) intr_c[(size_t)kIntr * i + k] = K[k];
  }
  for (int k = 0; k < 5; ++k) out[k] = a[k];
}
void launch_intr_candidate(hipStream_t s, int NI, const int2* meta, const double* intr, const double* sz,
                           const double* yz, const double* zg, double* intr_c, double* dz, double* out) {
  k_intr_candidate<<<1, 64, 0, s>>>(NI, meta, intr, sz, yz, zg, intr_c, dz, out);
}

// k_candidate with free intrinsics: m gains J_z delta_z and the candidate residual is taken at
// the candidate intrinsics
template <int LOSS>
__global__ __launch_bounds__(256) void k_candidate_z(DevView v, const double* __restrict__ points,
                                                     const double* __restrict__ camtab,
                                                     const double* __restrict__ dp, const double* __restrict__ dc,
                                                     const double* __restrict__ camtab_c,
                                                     const int2* __restrict__ meta, const double* __restrict__ dz,
                                                     const double* __restrict__ intr_c,
                                                     double* __restrict__ partial) {
  double acc[3] = {0.0, 0.0, 0.0};
  const size_t NPs = (size_t)v.NP;
  const GlobalTabs tb{camtab, v.intr};
  const LossK lk = loss_of(v);
  for (int s = blockIdx.x * blockDim.x + threadIdx.x; s < v.N; s += gridDim.x * blockDim.x) {
    const int4 id = v.obs_idx[s];
    if (id.x < 0) continue;  // padding slot
    const double2 xy = v.obs_xy[s];
    const double X[3] = {points[3 * (size_t)id.x], points[3 * (size_t)id.x + 1], points[3 * (size_t)id.x + 2]};
    const double d3[3] = {dp[id.x], dp[NPs + id.x], dp[2 * NPs + id.x]};
    double m0 = 0.0, m1 = 0.0, ru, rv;
    {
      ObsJac o;
      obs_jacobian_t<LOSS>(id, xy, X, tb, o, lk);
      ru = o.pr.ru;
      rv = o.pr.rv;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        m0 += o.jx0[c] * d3[c];
        m1 += o.jx1[c] * d3[c];
      }
      const int c0 = v.ext_col[id.y];
      if (c0 >= 0) {
        const double* d = dc + 6 * c0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          m0 += o.jw0a[k] * d[k];
          m1 += o.jw0b[k] * d[k];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          m0 += o.pr.A0[k] * d[3 + k];
          m1 += o.pr.A1[k] * d[3 + k];
        }
      }
      const int c1 = id.z >= 0 ? v.ext_col[id.z] : -1;
      if (c1 >= 0) {
        const double* d = dc + 6 * c1;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          m0 += o.jw1a[k] * d[k];
          m1 += o.jw1b[k] * d[k];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          m0 += o.jt1a[k] * d[3 + k];
          m1 += o.jt1b[k] * d[3 + k];
        }
      }
      const int2 mt = meta[id.w];
      if (mt.x >= 0) {
        double P[3], Kr[6], z0[6], z1[6];
        obs_cam_point(id, X, tb, P);
        tb.k(id.w, Kr);
        intr_rows<LOSS>(P, Kr, xy.x, xy.y, lk, mt.y & 63, ((mt.y >> 16) & 1) != 0, z0, z1);
#pragma unroll
        for (int a = 0; a < 6; ++a) {
          m0 += z0[a] * dz[6 * mt.x + a];
          m1 += z1[a] * dz[6 * mt.x + a];
        }
      }
    }
    acc[0] += -(m0 * (ru + m0 / 2.0) + m1 * (rv + m1 / 2.0));
    // candidate residual at (x + delta)
    const double Xc[3] = {X[0] + d3[0], X[1] + d3[1], X[2] + d3[2]};
    double T0[12], Kc[6];
    load_tab<12>(camtab_c, id.y, T0);
    load_intr(intr_c, id.w, Kc);
    double P[3];
    if (id.z >= 0) {
      double T1[12], P2[3];
      load_tab<12>(camtab_c, id.z, T1);
      matvec_add(T1, Xc, T1 + 9, P2);
      matvec_add(T0, P2, T0 + 9, P);
    } else {
      matvec_add(T0, Xc, T0 + 9, P);
    }
    Proj pc;
    project<LOSS>(P, Kc, xy.x, xy.y, pc, false, lk);
    if constexpr (LOSS == DAB_LOSS_TRIVIAL) acc[1] += pc.ru * pc.ru + pc.rv * pc.rv;
    else acc[1] += pc.rho;
    acc[2] += (isfinite(pc.ru) && isfinite(pc.rv)) ? 0.0 : 1.0;
  }
  block_reduce_store<3>(acc, partial + 3 * (size_t)blockIdx.x);
}
void launch_candidate_z(hipStream_t s, const DevView& v, const double* points, const double* camtab,
                        const double* delta_p, const double* delta_c, const double* camtab_c, const int2* meta,
                        const double* dz, const double* intr_c, double* partial, int grid) {
  DAB_LOSS_SWITCH(v.loss, k_candidate_z<LOSS><<<grid, 256, 0, s>>>(v, points, camtab, delta_p, delta_c, camtab_c, meta,
                                                                  dz, intr_c, partial));
}

// Loads this translation unit's code object on the current device now: otherwise the first
// launch of any of its kernels pays for it (10-40 ms, inside a process's first LM iteration).
void warm_kernels() {
  hipFuncAttributes a;
  (void)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(k_cam_tables));
}

}  // namespace dab

#ifdef DAB_TRACE
extern "C" int dab_trace_fetch(unsigned long long* out) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(dab::g_trace), sizeof(dab::g_trace)) == hipSuccess ? 0 : -1;
}
extern "C" int dab_trace_hwid(unsigned* out) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(dab::g_hwid), sizeof(dab::g_hwid)) == hipSuccess ? 0 : -1;
}
extern "C" int dab_trace_clear() {
  static unsigned long long z[256 * 16 * 8];
  return hipMemcpyToSymbol(HIP_SYMBOL(dab::g_trace), z, sizeof(z)) == hipSuccess ? 0 : -1;
}
#endif
