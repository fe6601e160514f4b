// dab_k_fused.hip — k_eval_bal, the fused evaluation pass of BAL-shaped problems, with the
// camera waves' point-frame loop and the per-wave trace of timing builds (-DDAB_TRACE).
// Row arithmetic and data layout: dab_rows.h.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "dab_kernels.h"
#include "dab_reduce.h"
#include "dab_rows.h"
#include "dab_warm.h"
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

DAB_WARM_TU(k_eval_bal<0, 0, DAB_LOSS_TRIVIAL>);

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
