// dab_k_points.hip — the point side of the evaluation pass as a pass of its own: k_eval_points and
// its LDS-table and deep-prefetch variants (the variants DAB_EVAL_WPS selects), with the cost
// partial sums only they use. Row arithmetic and data layout: dab_rows.h.
#include <hip/hip_runtime.h>

#include "dab_kernels.h"
#include "dab_reduce.h"
#include "dab_rows.h"
#include "dab_warm.h"
#include "dab_wave.h"

namespace dab {

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

DAB_WARM_TU(k_eval_points_lds<128, 4, false, DAB_LOSS_TRIVIAL>);

}  // namespace dab
