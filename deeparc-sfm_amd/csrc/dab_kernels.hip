// dab_kernels.hip — gfx950 kernels of the BA hot path that are not an evaluation pass of their
// own file: the reduction kernels, the per-extrinsic tables, the parity kernels, the camera side
// (k_eval_cams), the rig's pair-major passes, the matrix-free PCG products and the candidate
// pass. The point-side pass is in dab_k_points.hip, the fused pass in dab_k_fused.hip, the
// explicit-Schur step in dab_k_step.hip, its tile path in dab_k_tiles.hip, the free intrinsics
// in dab_k_intr.hip.
// Row arithmetic and data layout: dab_rows.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cstdlib>
#include <type_traits>

#include "dab_kernels.h"
#include "dab_reduce.h"
#include "dab_rows.h"
#include "dab_warm.h"
#include "dab_wave.h"

namespace dab {

int grid_for(int n, int block, int cap) {
  int g = (n + block - 1) / block;
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return g;
}

// ------------------------------------------------------------------------------------
// reductions
// ------------------------------------------------------------------------------------
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

DAB_WARM_TU(k_cam_tables);

}  // namespace dab
