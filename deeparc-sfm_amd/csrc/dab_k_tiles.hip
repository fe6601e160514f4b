// dab_k_tiles.hip — the explicit reduced camera system of small camera sets by register-owned
// block tiles (k_schur_y, k_schur_tiles and their sums).
// Row arithmetic and data layout: dab_rows.h.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "dab_kernels.h"
#include "dab_reduce.h"
#include "dab_rows.h"
#include "dab_warm.h"
#include "dab_wave.h"

namespace dab {

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

DAB_WARM_TU(k_schur_tiles);

}  // namespace dab
