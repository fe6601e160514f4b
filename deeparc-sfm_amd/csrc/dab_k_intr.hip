// dab_k_intr.hip — free intrinsics in the exact Schur step (dab_set_intrinsics_free).
// Row arithmetic and data layout: dab_rows.h.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "dab_kernels.h"
#include "dab_reduce.h"
#include "dab_rows.h"
#include "dab_warm.h"
#include "dab_wave.h"

namespace dab {

// ------------------------------------------------------------------------------------
// Free intrinsics (dab_set_intrinsics_free): the block z of six slots (cx, cy, f0, f1, k0,
// k1) per free intrinsic beside the cameras in the exact Schur step. Every kernel here
// re-evaluates the observation's rows through obs_jacobian_t / project, so residual, point
// and camera rows are those of the evaluation pass; the intrinsic rows come from intr_rows.
// All sums: one owner thread per output element and a fixed order, no floating-point atomics.
// ------------------------------------------------------------------------------------

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

DAB_WARM_TU(k_intr_jac);

}  // namespace dab
