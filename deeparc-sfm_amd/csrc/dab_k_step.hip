// dab_k_step.hip — the explicit-Schur LM step: point factor, entry Y, the pair-table S blocks,
// camera rhs, back-substitution, and the candidate's point and camera updates and norms.
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

DAB_WARM_TU(k_point_factor);

}  // namespace dab
