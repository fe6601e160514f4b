// dab_handle.h — struct dab_handle and what the host files of the library share (not part of
// the ABI): the error macros, the environment knobs, the small host helpers of the set-up, and
// the functions that cross files (namespace dab). See DESIGN §1 for which file holds what.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <limits>
#include <array>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "dab_devmem.h"
#include "dab_internal.h"
#include "dab_kernels.h"
#include "dab_p2p.h"
#include "dab_setup.h"

#define HIP_OK(expr)                                                                           \
  do {                                                                                         \
    hipError_t e_ = (expr);                                                                    \
    if (e_ != hipSuccess)                                                                      \
      return set_error(DAB_E_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));      \
  } while (0)
#define NCCL_OK(expr)                                                                          \
  do {                                                                                         \
    ncclResult_t e_ = (expr);                                                                  \
    if (e_ != ncclSuccess)                                                                     \
      return set_error(DAB_E_COMM, std::string(#expr) + ": " + ncclGetErrorString(e_));       \
  } while (0)
#define CHECK_RC(expr)       \
  do {                       \
    int rc_ = (expr);        \
    if (rc_ != 0) return rc_; \
  } while (0)

namespace dab {

inline double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// Host set-up runs again after every filterPoint3d round (sfm.cc:118-127), so its
// O(observations) passes are spread over host threads. Every pass below gives the same
// result as its sequential form (each thread owns a contiguous index range; the counting
// sorts are stable: per-thread bucket counts are offset in (bucket, thread) order).
inline int setup_threads() {
  static const int t = [] {
    int n = (int)std::thread::hardware_concurrency();
    return std::max(1, std::min(n, 16));
  }();
  return t;
}
template <class F>
void par_for(long long n, F f, long long grain = 65536) {  // f(begin, end, thread), contiguous ranges
  const int T = (int)std::min<long long>(setup_threads(), std::max(1LL, n / grain));
  if (T <= 1) {
    f(0LL, n, 0);
    return;
  }
  std::vector<std::thread> th;
  for (int t = 0; t < T; ++t) th.emplace_back([&, t] { f(n * t / T, n * (t + 1) / T, t); });
  for (auto& x : th) x.join();
}
// vectors whose elements are default-initialised (no zero fill): the large set-up arrays
// are first touched by the parallel passes that fill them, not by one thread
template <class T>
struct NoInit : std::allocator<T> {
  template <class U>
  struct rebind {
    using other = NoInit<U>;
  };
  NoInit() = default;
  template <class U>
  NoInit(const NoInit<U>&) {}
  template <class U, class... Args>
  void construct(U* p, Args&&... args) {
    ::new ((void*)p) U(std::forward<Args>(args)...);
  }
  template <class U>
  void construct(U* p) {
    ::new ((void*)p) U;
  }
};
template <class T>
using big_vec = std::vector<T, NoInit<T>>;

// stable counting sort of [0, n) by key(i) in [0, nb): out[pos] = i; start[nb + 1] = bucket
// offsets. key(i) < 0 drops i.
template <class K, class V>
void bucket_sort(long long n, int nb, K key, V& out, std::vector<long long>& start) {
  const int T = (int)std::min<long long>(setup_threads(), std::max(1LL, n / 65536));
  std::vector<std::vector<int>> cnt(T, std::vector<int>((size_t)nb, 0));
  std::vector<std::thread> th;
  auto range = [&](int t) { return std::make_pair(n * t / T, n * (t + 1) / T); };
  auto count = [&](int t) {
    auto r = range(t);
    for (long long i = r.first; i < r.second; ++i) {
      const int k = key(i);
      if (k >= 0) cnt[t][k]++;
    }
  };
  if (T > 1) {
    for (int t = 0; t < T; ++t) th.emplace_back(count, t);
    for (auto& x : th) x.join();
    th.clear();
  } else {
    count(0);
  }
  start.assign((size_t)nb + 1, 0);
  long long acc = 0;
  for (int b = 0; b < nb; ++b) {
    start[b] = acc;
    for (int t = 0; t < T; ++t) {
      const int c = cnt[t][b];
      cnt[t][b] = (int)acc;  // thread t's first position in bucket b
      acc += c;
    }
  }
  start[nb] = acc;
  out.resize((size_t)acc);
  auto place = [&](int t) {
    auto r = range(t);
    std::vector<int>& pos = cnt[t];
    for (long long i = r.first; i < r.second; ++i) {
      const int k = key(i);
      if (k >= 0) out[pos[k]++] = (int)i;
    }
  };
  if (T > 1) {
    for (int t = 0; t < T; ++t) th.emplace_back(place, t);
    for (auto& x : th) x.join();
  } else {
    place(0);
  }
}

// scalar slots of the per-handle scalar buffer
enum Slot {
  S_COST = 0,      // sum r^2 at x
  S_COST_BAD,      // non-finite residuals at x
  S_GMAX_P,        // max |x-(x-g)| over points
  S_GNORM_P,       // sum (x-(x-g))^2 over points
  S_XNORM_P,       // sum x^2 over points
  S_MODEL,         // model cost change
  S_CAND,          // sum r^2 at candidate
  S_CAND_BAD,      // non-finite residuals at candidate
  S_STEP_P,        // sum (x - xc)^2 over points
  S_XCNORM_P,      // sum xc^2 over points
  S_CAM0,          // 5 camera slots (launch_cam_norms)
  S_TIME = S_CAM0 + 5,  // solver wall-clock (max over ranks)
  S_END,
  // fixed-point cost shards of the prefetch point kernel (uint64 bit patterns: sum r^2
  // integer part, fraction * 2^52, non-finite count per shard; cost_fx_add)
  S_CFX = 16,  // two sets of kFxWords, alternating between passes
  S_XERR = S_CFX + 2 * kFxWords,  // k_eval_bal's error word (uint32 bits; 0 = ok)
  S_PRIOR,  // 0.5 sum |A (x - mu)|^2 over the effective extrinsic priors at x (k_prior_blocks)
  S_PPRIOR,  // the same over this rank's effective point priors (k_pt_prior_blocks), then over the ranks
  S_SYNC,    // 2 words: what a multi-rank call decides once for all ranks (call_state), max-reduced
  S_SYNC1,
  S_ZPRIOR,  // 0.5 sum |A (x_i - mu)|^2 over the effective intrinsic priors at x (k_zprior_blocks)
  S_NSLOTS
};

// Device buffers of one problem come from a Dev (dab_devmem.h): dab_set_problem releases
// them all into a pool instead of freeing them, and an allocation takes the smallest pooled
// block that holds it without wasting more than half (or 1 MiB), so the sfm.cc loop's
// re-set-up after every filter round (the same problem, a little smaller) finds its ~50
// buffers there instead of paying a hipMalloc / hipFree pair each. A pooled block unused
// through one whole set-up and solve cycle is freed at the next release. The stream is
// synchronised before a release (dab_set_problem), so no queued kernel still reads a block
// that gets reused.

template <class T, class A>
int upload(T** dptr, Dev& dev, const std::vector<T, A>& h, hipStream_t s) {
  CHECK_RC(dev.alloc(dptr, h.size()));
  if (!h.empty()) HIP_OK(hipMemcpyAsync(*dptr, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, s));
  return 0;
}

// Tuning / test knobs from the environment, read once when the handle is created (never
// on a launch path). Unset = the production default.
struct Knobs {
  int chunk = 0;            // DAB_CHUNK: entries per camera-side reduction chunk (0: kChunk)
  int xchunk = 0;           // DAB_XCHUNK: most entries per pair-major chunk (0: kPairChunk)
  int pair_eval = -1;       // DAB_PAIR_EVAL=0: rig camera side camera-major + cross passes
  int eval_wps = INT_MIN;   // DAB_EVAL_WPS: point-kernel variant of the two-kernel pass
  int eval_fused = 1;       // DAB_EVAL_FUSED=0: two-kernel pass even where the fused one fits
  int eval_split = 0;       // DAB_EVAL_SPLIT=1: the multi-rank split schedule on one rank
  int pcg_fused = 1;        // DAB_PCG_FUSED=0
  int pcg_mf = 1;           // DAB_PCG_MF=0: stored-Y PCG even for small camera sets
  int cg_onewg = 0;         // DAB_CG_ONEWG=1: single-work-group CG update
  int bench_sample = 8;     // DAB_BENCH_SAMPLE: timing-event stride of dab_bench_eval_pass
  int schur_tiles = 1;      // DAB_SCHUR_TILES=0: explicit S from the pair tables even for small NC
  int tile_balance = 1;     // DAB_TILE_BALANCE=0: one work-group per tile and group of batches
  int tile_single = 1;      // DAB_TILE_SINGLE=0: k_schur_tiles with two LDS buffers (batches half as
                            // large, the next one in flight; round 6: one buffer, C5 EXACT 5.5 -> 5.2 ms)
  int tile_minb = 2;        // DAB_TILE_MINB: fewest batches per k_schur_tiles work-group (8 until round 6)
  int p2p = -1;             // DAB_P2P: one-shot xGMI all-reduce of small sums (-1 auto: RCCL handles
                            // only; 1 also on host-staged handles, the one-GPU rehearsal; 0 off)
  int intr_border_lds = 1;  // DAB_INTR_BORDER_LDS=0: the free-intrinsic border's sums in global memory
                            // (k_intr_border_g) even where its LDS rows fit
  int setup_host = 0;       // DAB_SETUP_HOST=1: dab_set_problem's host passes instead of the device ones
  int eval_side = 0;        // DAB_EVAL_SIDE: 7 (test) a k_eval_bal frame wait that times out (the pass
                            // must fail with DAB_E_DEVICE on every rank). Builds with -DDAB_ABLATIONS
                            // also take the timing ablations (wrong results) 1 the point side only, 2
                            // the camera side only, 3 the tables only, 4 no tables or frames, 5 no
                            // point tables, 6 no camera frames; a release build refuses them
                            // (eval_side_ok: DAB_E_INVALID) instead of returning wrong sums
  int fused_tab = -1;       // DAB_FUSED_TAB: the fused pass reads the camera tables of the current x
                            // instead of building them in every work-group — -1 (default) when they
                            // exist already (the LM loop: the accepted candidate's tables), 1 always
                            // (building them first where they do not), 0 never
  int points_direct = 1;    // DAB_POINTS_DIRECT=0: the general masked step even when no rank has a free
                            // point (the A/B of the direct camera step, S = U + D^2)
  void read() {
    auto get = [](const char* name, int& out) {
      if (const char* e = getenv(name)) out = atoi(e);
    };
    get("DAB_CHUNK", chunk);
    get("DAB_XCHUNK", xchunk);
    get("DAB_PAIR_EVAL", pair_eval);
    get("DAB_EVAL_WPS", eval_wps);
    get("DAB_EVAL_FUSED", eval_fused);
    get("DAB_EVAL_SPLIT", eval_split);
    get("DAB_PCG_FUSED", pcg_fused);
    get("DAB_PCG_MF", pcg_mf);
    get("DAB_CG_ONEWG", cg_onewg);
    get("DAB_BENCH_SAMPLE", bench_sample);
    get("DAB_SCHUR_TILES", schur_tiles);
    get("DAB_TILE_BALANCE", tile_balance);
    get("DAB_TILE_MINB", tile_minb);
    get("DAB_TILE_SINGLE", tile_single);
    get("DAB_P2P", p2p);
    get("DAB_FUSED_TAB", fused_tab);
    get("DAB_SETUP_HOST", setup_host);
    get("DAB_INTR_BORDER_LDS", intr_border_lds);
    get("DAB_EVAL_SIDE", eval_side);
    get("DAB_POINTS_DIRECT", points_direct);
  }
  // the evaluation side this build accepts from DAB_EVAL_SIDE
  bool eval_side_ok() const {
#ifdef DAB_ABLATIONS
    return eval_side >= 0 && eval_side <= 7;
#else
    return eval_side == 0 || eval_side == 7;
#endif
  }
};

// DAB_SETUP_TIMING=1: phase times on stderr. fmt prints one line from (phase name, ms since
// the previous line, extra...).
struct PhaseTimer {
  const char* fmt;
  double t = now_s();
  static bool on() {
    static const bool v = getenv("DAB_SETUP_TIMING") != nullptr;
    return v;
  }
  template <class... A>
  void operator()(const char* what, A... extra) {
    if (!on()) return;
    const double now = now_s();
    std::fprintf(stderr, fmt, what, 1e3 * (now - t), extra...);
    t = now;
  }
};

// The handle's state. dab.h's opaque dab_handle (below) is this struct: it is written inside the
// namespace so that its members name the library's types without qualification.
struct Handle {
  Knobs knobs;
  int device = 0;
  int rank = 0, world = 1;
  hipStream_t stream = nullptr;
  ncclComm_t comm = nullptr;
  CholCtx* chol = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr, ev3 = nullptr;
  // multi-GPU: the camera-block all-reduce runs on its own stream, overlapping the
  // point-side kernel (ev_cam: camera blocks ready; ev_comm: all-reduce done)
  hipStream_t comm_stream = nullptr;
  hipEvent_t ev_cam = nullptr, ev_comm = nullptr;
  // bench bookkeeping
  double bench_jac_ms = 0, bench_asm_ms = 0, bench_pair_ms = 0;
  int bench_count = 0, bench_pending = 0, bench_pair_count = 0;
  // per-step events (dab_bench_eval_pass): start, point kernel start / end, end, and the
  // rig's pair-major camera kernel (k_eval_pair) start / end
  std::vector<std::array<hipEvent_t, 6>> bench_ev;
  std::vector<char> bench_pair_rec;  // per pending step: the pair events were recorded

  // ---- host-side problem structure ----
  bool have_problem = false;
  bool local_compose = false;       // some observation of this rank is composed (arc∘ring)
  bool host_entries = false;        // h_pt_ent_ptr / h_ent_* hold the entry lists (host set-up path)
  dab_problem prob{};               // caller's arrays (pointers valid until next set_problem)
  int N = 0, NP = 0, E = 0, NI = 0, NC = 0, NE = 0, nplanes = 18;
  bool any_compose = false;
  std::vector<int> perm;            // sorted obs -> caller's obs index
  std::vector<int> pt_of;           // local point -> caller's point id
  std::vector<int> ext_col;         // ext -> free camera column
  std::vector<uint8_t> ext_fixed;   // ext is constant (ext_const or freeze_camera): known exactly
  int nchunk = 0, nxchunk = 0, ncross = 0, nblk = 0, nslice = 0;
  int max_seg_chunks = 1, max_xseg_chunks = 1;  // largest chunk count of one camera / cross pair
  int NS = 0;  // observation slots (SELL-64, incl. padding)
  long long npairs = 0;
  int lds = 0;                      // leading dim of dense S
  bool schur_built = false;
  bool pcg_built = false;
  int nxlist = 0;
  std::vector<int> h_pt_ent_ptr;  // kept for build_schur_tables
  big_vec<int> h_ent_cam, h_ent_pos, h_ent_os;

  // ---- device buffers ----
  Dev dev{"problem buffers"};
  Dev setup_tmp{"set-up scratch"};  // the device set-up's scratch (released by the next set-up)
  Dev keep_dev{"kept buffers"};     // the Sticky buffers below (never released, re-sized by drop + alloc)
  DevView view{};
  // robust loss (dab_set_loss): the type and a, b, c live in view (loss, loss_a..c), which
  // set_problem fills field by field and so never resets; this is the scale as it was given
  double loss_scale = 0.0;
  int4* d_obs_idx = nullptr;
  double2* d_obs_xy = nullptr;
  // fused pass: packed 4-B slot records of the point waves (DevView::obs_e)
  int* d_obs_e = nullptr;
  int4* d_cm_idx = nullptr;
  double2* d_cm_xy = nullptr;
  int4* d_x_idx = nullptr;
  double2* d_x_xy = nullptr;
  int *d_slice_off = nullptr, *d_pt_ent_ptr = nullptr, *d_ent_os = nullptr, *d_ent_cam = nullptr,
      *d_ent_pt = nullptr, *d_ent_pos = nullptr, *d_cm_pt = nullptr, *d_ext_col = nullptr;
  int *d_chunk_beg = nullptr, *d_seg_chunk = nullptr;
  int2* d_chunk_uni = nullptr;
  int uni_affine = 0, uni_ox = 0, uni_oi = 0;  // chunk_uni[c] = (c + ox, c + oi) for every chunk
  unsigned* d_arrivals = nullptr;  // last-arriver counter of the point kernel (kept zeroed)
  int* d_chunk_lists = nullptr;  // uniform chunk ids, then the others
  ChunkLists chunks;
  int *d_xchunk_beg = nullptr, *d_xseg_chunk = nullptr;
  int2* d_cross_cam = nullptr;
  int2 *d_pairs = nullptr, *d_blk_cam = nullptr;
  int2* d_blk_zero = nullptr;  // lower blocks of S without pairs (one rank: zeroed directly)
  int nzero = 0;
  int* d_blk_pair_beg = nullptr;
  double* d_intr = nullptr;
  // free intrinsics (dab_set_intrinsics_free). The mask is state of the handle, reset by
  // dab_set_problem; the free set is worked out from it at each call that needs it
  // (intr_free_set): referenced on some rank and at least one active scalar selected.
  std::vector<uint8_t> intr_mask;         // [NI] requested groups (DAB_INTR_*)
  std::vector<uint8_t> intr_ref;          // [NI] referenced by an observation (union over ranks once intr_ref_union)
  bool intr_ref_union = false;
  std::vector<double> intr_host;          // [NI][6] dab_problem layout: what dab_get_intrinsics fills unused slots from
  std::vector<int> intr_nf, intr_nk;
  std::vector<int2> intr_meta;            // host copy of d_intr_meta (kernels.h)
  int nfi = 0;                            // free intrinsics of the meta now on the device
  // constant points (dab_set_points_constant). The mask is state of the handle, reset by
  // dab_set_problem; empty = never set or NULL. pt_const_sync works out the constant set
  // (referenced on this rank and flagged) at each call that honours it and leaves its device
  // form in d_ptc: null while the set is empty, so that every launch is then the unmasked one.
  std::vector<uint8_t> pt_const;          // [num_points], caller order
  bool pt_const_dirty = false;            // lz.d_pt_const does not hold pt_const
  const uint8_t* d_ptc = nullptr;         // [NP] device point order (lz.d_pt_const), or null
  int n_pt_const = 0;                     // constant points of this rank (of the last sync)
  // constant scalars of an extrinsic (dab_set_ext_scalars_constant). The mask is state of the
  // handle, reset by dab_set_problem; empty = never set or NULL. ext_sub_sync works out the
  // effective set (bits on an extrinsic with a camera column) at each call that honours it and
  // leaves it per camera column in d_exs: null while the set is empty, so that every launch is
  // then the unmasked one.
  std::vector<uint8_t> ext_sub;           // [num_ext] bits as set
  bool ext_sub_dirty = false;             // lz.d_ext_sub does not hold the effective set
  const uint8_t* d_exs = nullptr;         // [NC] bits by camera column (lz.d_ext_sub), or null
  int n_ext_sub = 0;                      // effective constant scalars (of the last sync)
  // extrinsic priors (dab_set_ext_priors), as set: state of the handle, reset by dab_set_problem.
  // prior_sync works out the effective set (the extrinsic has a camera column) at each call that
  // honours it and leaves its device records in lz.d_prior_*; n_prior = 0 while the set is empty,
  // so that no prior kernel is launched then.
  std::vector<int> prior_idx;             // [count]
  std::vector<double> prior_mean;         // [count][6]
  std::vector<double> prior_A;            // [count][6][6] row-major
  bool prior_dirty = false;               // lz.d_prior_* do not hold the effective set
  int n_prior = 0;                        // effective priors (of the last sync)
  // point priors (dab_set_point_priors), as set: state of the handle, reset by dab_set_problem.
  // pt_prior_sync (after pt_const_sync) works out this rank's effective set (the point is
  // referenced here and not constant), sorted by device point, at each call that honours it;
  // call_state then tells whether any rank has one (pt_prior_any: the calls are collective, every
  // rank takes the same path). n_pt_prior = 0 and pt_prior_any = false while no rank has one, and
  // no kernel runs then.
  std::vector<int> pt_prior_idx;          // [count] caller's point ids
  std::vector<double> pt_prior_mean;      // [count][3]
  std::vector<double> pt_prior_A;         // [count][3][3] row-major
  bool pt_prior_dirty = false;            // lz.d_ptp_* do not hold the effective set
  std::vector<int> pt_prior_pos;          // [count] place in the effective set or -1 (of the last upload)
  int pt_prior_n = 0;                     // size of the effective set (of the last upload)
  int n_pt_prior = 0;                     // effective point priors of this rank (of the last sync)
  bool pt_prior_any = false;              // some rank has an effective point prior (of the last sync)
  // intrinsic priors (dab_set_intr_priors), as set: state of the handle, reset by dab_set_problem.
  // zprior_sync (after the free set of the call is on the handle) works out the effective set (the
  // intrinsic has a free column), sorted by that column, with the inactive columns of A and entries
  // of the mean zeroed, and leaves its device records in lz.d_zp_*; n_zprior = 0 while the set is
  // empty, so that no prior kernel is launched then.
  std::vector<int> zprior_idx;            // [count]
  std::vector<double> zprior_mean;        // [count][6]
  std::vector<double> zprior_A;           // [count][6][6] row-major
  std::vector<int2> zprior_dev_idx;       // host copies of lz.d_zp_idx / lz.d_zp_rec (uploaded on change)
  std::vector<double> zprior_dev_rec;
  std::vector<int> zprior_pos;            // [count] place in the effective set or -1 (of the last sync)
  int n_zprior = 0;                       // effective intrinsic priors (of the last sync)
  int ldz = 0;
  // Buffers allocated from `dev` by the first call that needs them (null / capacity 0: not yet).
  // They die with dev.release(): dab_set_problem resets this whole sub-object there, so a member
  // added here cannot be left pointing into the previous problem's memory.
  struct Lazy {
    double* d_Jfull = nullptr;  // parity API only
    double* d_Yrec = nullptr;   // EXPLICIT: Y as [NE][18] records for k_s_blocks
    float *d_Y32c = nullptr, *d_Y32p = nullptr;  // pcg_fp32
    // free intrinsics (intr_free_set)
    double* d_intr_c = nullptr;   // candidate intrinsics [NI][kIntr]
    int2* d_intr_meta = nullptr;  // [NI]
    int* d_intr_act = nullptr;    // [kIntrFreeMax]
    // [zg nfi*28 | sz 96 | dz 96 | norms 5+3] and the k_intr_eval / k_intr_border partials
    double *d_zg = nullptr, *d_sz = nullptr, *d_dz = nullptr, *d_znorm = nullptr, *d_zpart = nullptr;
    double *d_bpart = nullptr, *d_bsum = nullptr, *d_Sz = nullptr, *d_yz = nullptr;
    int* d_ptmask = nullptr;  // [NP] free intrinsics each point sees (k_intr_ptmask, per solve)
    uint8_t* d_pt_const = nullptr;  // [NP] constant points, device point order (pt_const_sync)
    double* d_zero6 = nullptr;      // [6 NC] zeros: the rhs part of a step without free points
    uint8_t* d_ext_sub = nullptr;   // [NC] constant scalars by camera column (ext_sub_sync)
    // effective extrinsic priors (prior_sync): (extrinsic, camera column) and kPriorRec doubles each
    int2* d_prior_idx = nullptr;
    double* d_prior_rec = nullptr;
    double* d_prior_res = nullptr;  // [n][6] + cost: dab_eval_ext_priors
    double* d_prior_part = nullptr;  // [2 n] per-prior terms of k_prior_blocks / k_prior_candidate
    unsigned* d_prior_cnt = nullptr; // their arrival count (zero between launches)
    int prior_cap = 0;
    // effective point priors (pt_prior_sync): device point and the planar records [kPtPriorRec][n]
    int* d_ptp_idx = nullptr;
    double* d_ptp_rec = nullptr;
    double* d_ptp_res = nullptr;   // [n][3] + cost: dab_eval_point_priors
    double* d_ptp_part = nullptr;  // [2 groups] work-group sums of k_pt_prior_blocks / k_pt_prior_candidate
    unsigned* d_ptp_cnt = nullptr; // their arrival count (zero between launches), apart from d_prior_cnt
    int ptp_cap = 0;
    // effective intrinsic priors (zprior_sync): (intrinsic, free column), kPriorRec doubles each
    int2* d_zp_idx = nullptr;       // [kIntrFreeMax]
    double* d_zp_rec = nullptr;     // [kIntrFreeMax][kPriorRec]
    double* d_zp_res = nullptr;     // [kIntrFreeMax][6] + cost: dab_eval_intr_priors
    size_t bpart_cap = 0, Sz_cap = 0;
    // dab_covariance: Z = L^-1 [n][lds], the point blocks [NP][6], the extrinsic blocks [NC][21],
    // the rank test's scalars and partials
    double *d_covZ = nullptr, *d_cov_pts = nullptr, *d_cov_ext = nullptr, *d_cov_stat = nullptr;
    int* d_cov_idx = nullptr;  // [NE] camera of each merged record | [NP] records per point
    // dab_covariance_intrinsics: Z of the bordered system [n'][ldz], the fold-back's records
    // [cap][18] and [camera of each record cap | records per point NP | first record of each
    // point NP + 1]
    double *d_covZz = nullptr, *d_cov_rec = nullptr;
    int* d_cov_ridx = nullptr;
    size_t covZz_cap = 0, cov_rec_cap = 0;
    // dab_covariance_blocks: the translated pair lists [pp | pe | pz] and their blocks
    // [pp 9 | pe 18 | pz 18 each], kept while they fit
    int2* d_covx_pairs = nullptr;
    double* d_covx_out = nullptr;
    size_t covx_pairs_cap = 0, covx_out_cap = 0;
  } lz;
  double *d_points = nullptr, *d_points_c = nullptr, *d_ext = nullptr, *d_ext_c = nullptr;
  double *d_camtab = nullptr, *d_camtab_c = nullptr;
  double* d_r = nullptr;
  double *d_V = nullptr, *d_g = nullptr, *d_scale_p = nullptr, *d_scale_c = nullptr;
  double *d_L = nullptr, *d_q = nullptr, *d_Y = nullptr, *d_Yp = nullptr;  // Y camera-/point-major
  // events of the covariance's stage times, and around its border rows
  hipEvent_t cov_ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  hipEvent_t cov_ev_z[2] = {nullptr, nullptr};
  hipEvent_t cov_ev_x[2] = {nullptr, nullptr};  // around the cross-block kernels
  double* d_camred = nullptr;  // [Ucc NC*21 | gc NC*6 | Ux ncross*36] (all-reduced)
  double* d_partial = nullptr; // chunk partials (max of chunk counts * 36)
  double* d_xpartial = nullptr; // cross-block chunk partials
  // pair-major evaluation of the composed observations (launch_eval_pair): the other
  // entries' camera-major copy and chunks, and per camera its pair-chunk halves
  bool pair_eval = false;
  bool pair_uni_intr = false;  // one intrinsic per (arc, ring) pair: k_eval_pair's uniform tables
  double pair_bytes = 0.0, last_pair_ms = 0.0;  // k_eval_pair: algorithmic bytes per launch, bench time
  int nchunk2 = 0;
  int4* d_cm2_idx = nullptr;
  double2* d_cm2_xy = nullptr;
  int *d_chunk2_beg = nullptr, *d_seg2_chunk = nullptr, *d_xcam_ptr = nullptr, *d_xcam_list = nullptr;
  double *d_partial2 = nullptr, *d_xcpart = nullptr;
  double* d_spack = nullptr;   // [packed nblk*36 | ybc NC*6] (all-reduced)
  double* d_S = nullptr;
  // explicit S by fixed-point tiles (small camera sets, k_schur_tiles)
  bool schur_tiles = false;
  SchurTiles tiles{};
  int* d_kx = nullptr;                  // [6 NC] rhs row exponents
  double* d_sblk = nullptr;             // [nelem] Schur part of S by block (group sums, all-reduced)
  unsigned long long* d_rfx = nullptr;  // [6 NC] fixed-point rhs part (all-reduced as integers)
  double* d_yrec = nullptr;             // [nrec][18] Y of every record (this LM step)
  // implicit-Schur PCG (lazily allocated)
  double *d_pcg_b = nullptr, *d_pcg_r = nullptr, *d_pcg_z = nullptr, *d_pcg_p = nullptr, *d_pcg_q = nullptr,
         *d_pcg_w = nullptr, *d_pcg_Ad = nullptr, *d_pcg_Minv = nullptr, *d_pcg_red = nullptr,
         *d_pcg_t = nullptr;
  PcgState* d_pcg_state = nullptr;
  PcgState* h_pcg_state = nullptr;  // pinned
  int *d_xptr = nullptr, *d_xlist = nullptr, *d_run = nullptr;
  int* d_run_beg = nullptr;  // per chunk: its runs in d_run_rec
  int4* d_run_rec = nullptr;
  double *d_yc = nullptr, *d_dp = nullptr, *d_dc = nullptr;
  double* d_gpart = nullptr;   // grid partials
  double* d_scal = nullptr;    // S_NSLOTS
  int* d_flags = nullptr;      // [0] point factor fail, [1] chol fail
  double* h_scal = nullptr;    // pinned
  bool cost_fx_pending = false;  // fixed-point set fx_last holds the last evaluation's cost (read_scalars converts)
  int fx_last = 1;               // set of the last fixed-point pass (both sets start zeroed)
  int* h_flags = nullptr;      // pinned
  int red_grid = 1;
  bool fused_split = false;  // fused kernel as camera-side then point-side launches (world > 1)
  int eval_grid = 1;  // k_eval_points blocks (one SELL slice per block)
  int ncu = 256;      // compute units of the device
  int fused_grid = 0;  // > 0: single-pass PCG matvec (small camera systems)
  bool mf = false;     // matrix-free implicit Schur (no Y records; DAB_PCG_MF=0 disables)
  bool mf32 = false;   // this solve's matrix-free products in fp32 arithmetic (pcg_fp32)
  int mf_grid_n = 0;
  double* d_mf_partial = nullptr;
  const double* cg_wpart = nullptr;  // set by pcg_matvec: the partials the next CG update sums
  int pcg_hint = 2;    // CG iterations of the previous solve (first batch size)
  double* d_cg_partial = nullptr;  // multi-work-group CG update: grid partials + counter
  unsigned* d_cg_cnt = nullptr;
  double* d_fused_partial = nullptr;
  int eval_wps = 0;   // 0: LDS tables; else waves per slice (DAB_EVAL_WPS tuning knob)
  bool fused = false;  // evaluation pass as one launch (k_eval_bal; DAB_EVAL_FUSED=0 disables)

  // Buffers kept across dab_set_problem while the new problem's size fits: the dense S, the
  // camera step and the flags. The Cholesky's captured graph is keyed on their addresses, so
  // a problem re-set with the same camera count (the sfm.cc loop after every filter round)
  // replays the graph instead of capturing a new one.
  struct Sticky {
    void* p = nullptr;
    size_t cap = 0;
  };
  Sticky st_S, st_yc, st_flags;
  template <class T>
  int sticky(Sticky& st, T** out, size_t n) {
    const size_t bytes = std::max<size_t>(1, n) * sizeof(T);
    if (bytes > st.cap) {
      keep_dev.drop(st.p);
      st.p = nullptr;
      st.cap = 0;
      char* q = nullptr;
      CHECK_RC(keep_dev.alloc(&q, bytes));
      st.p = q;
      st.cap = bytes;
    }
    *out = static_cast<T*>(st.p);
    return 0;
  }

  ~Handle() {
    PhaseTimer phase{"destroy %-22s %.2f ms (%zu live, %zu pooled blocks)\n"};
    phase("start", dev.live.size(), dev.pool.size());
    dev.clear();
    phase("device buffers", dev.live.size(), dev.pool.size());
    keep_dev.clear();
    pinned_give(h_scal, sizeof(double) * S_NSLOTS);
    pinned_give(h_flags, sizeof(int) * 4);
    pinned_give(h_pcg_state, sizeof(PcgState));
    if (h_stage) (void)hipHostFree(h_stage);
    phase("pinned", dev.live.size(), dev.pool.size());
    if (chol) chol_destroy(chol);
    phase("Cholesky context", dev.live.size(), dev.pool.size());
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (ev2) (void)hipEventDestroy(ev2);
    if (ev3) (void)hipEventDestroy(ev3);
    for (hipEvent_t e : cov_ev)
      if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : cov_ev_z)
      if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : cov_ev_x)
      if (e) (void)hipEventDestroy(e);
    for (auto& e : bench_ev)
      for (hipEvent_t x : e) (void)hipEventDestroy(x);
    if (ev_cam) (void)hipEventDestroy(ev_cam);
    if (ev_comm) (void)hipEventDestroy(ev_comm);
    stream_give(device, comm_stream);
    p2p_destroy(p2p_main);
    p2p_destroy(p2p_comm);
    if (comm) ncclCommDestroy(comm);
    stream_give(device, stream);
  }

  unsigned* xerr() { return reinterpret_cast<unsigned*>(d_scal + S_XERR); }  // k_eval_bal's error word
  double* ug() { return d_camred; }  // [NC][27]: U upper-packed (21) | g_c (6)
  double* Ux() { return d_camred + (size_t)27 * NC; }
  size_t camred_count() const { return (size_t)27 * NC + (size_t)36 * ncross; }
  double* packed() { return d_spack; }
  double* ybc() { return d_spack + (size_t)36 * nblk; }
  size_t spack_count() const { return (size_t)36 * nblk + (size_t)6 * NC; }

  // one-shot xGMI all-reduce (dab_p2p.hip) of sums up to kP2pWords, one context per stream
  // (the main stream and the communication stream of the overlapped camera all-reduce)
  P2pComm* p2p_main = nullptr;
  P2pComm* p2p_comm = nullptr;
  static constexpr size_t kP2pWords = 65536;
  // an all-reduce on comm_stream can overlap the point-side kernel (RCCL or peer-to-peer)
  // rccl1: a one-rank handle on a real one-rank RCCL communicator (dab_create_dist with
  // world_size 1 and a unique id): every collective and the overlapped camera all-reduce run
  // through RCCL although they sum one rank, so the multi-GPU transport executes on one GPU
  bool rccl1 = false;
  bool coll() const { return world > 1 || rccl1; }
  bool can_overlap() const { return coll() && ((comm && !host_cb) || p2p_comm); }
  int allreduce_comm_stream(double* buf, size_t n) {
    if (p2p_comm && n <= kP2pWords) return p2p_allreduce_sum(p2p_comm, comm_stream, buf, n);
    if (!comm || host_cb) return set_error(DAB_E_STATE, "no collective for the communication stream");
    NCCL_OK(ncclAllReduce(buf, buf, n, ncclDouble, ncclSum, comm, comm_stream));
    return 0;
  }

  // host-staged collective (dab_create_dist_host): rehearsal path, not the product path
  dab_host_allreduce_fn host_cb = nullptr;
  void* host_user = nullptr;
  double* h_stage = nullptr;  // pinned
  size_t stage_cap = 0;

  int stage(size_t n) {
    if (n <= stage_cap) return 0;
    if (h_stage) (void)hipHostFree(h_stage);
    h_stage = nullptr;
    stage_cap = 0;
    if (hipHostMalloc(reinterpret_cast<void**>(&h_stage), n * sizeof(double)) != hipSuccess)
      return set_error(DAB_E_NOMEM, "pinned staging allocation failed");
    stage_cap = n;
    return 0;
  }
  int host_allreduce(double* buf, size_t n, int op) {
    CHECK_RC(stage(n));
    HIP_OK(hipMemcpyAsync(h_stage, buf, n * sizeof(double), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));
    if (host_cb(h_stage, (int64_t)n, op, host_user) != 0)
      return set_error(DAB_E_COMM, "host all-reduce callback failed");
    HIP_OK(hipMemcpyAsync(buf, h_stage, n * sizeof(double), hipMemcpyHostToDevice, stream));
    HIP_OK(hipStreamSynchronize(stream));
    return 0;
  }

  // exact integer sum over ranks of n uint64 words (the fixed-point cost); the host path
  // moves each word as three 22-bit pieces, which gloo's double sum adds exactly
  int allreduce_u64(uint64_t* buf, size_t n) {
    if (!coll() || n == 0) return 0;
    if (p2p_main && n <= kP2pWords)
      return p2p_allreduce_sum_u64(p2p_main, stream, reinterpret_cast<unsigned long long*>(buf), n);
    if (!host_cb) {
      NCCL_OK(ncclAllReduce(buf, buf, n, ncclUint64, ncclSum, comm, stream));
      return 0;
    }
    std::vector<uint64_t> tmp(n);
    CHECK_RC(stage(3 * n));
    HIP_OK(hipMemcpyAsync(tmp.data(), buf, n * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));
    for (size_t i = 0; i < n; ++i)
      for (int k = 0; k < 3; ++k) h_stage[3 * i + k] = (double)((tmp[i] >> (22 * k)) & 0x3fffffull);
    if (host_cb(h_stage, (int64_t)(3 * n), 0, host_user) != 0)
      return set_error(DAB_E_COMM, "host all-reduce callback failed");
    for (size_t i = 0; i < n; ++i) {
      uint64_t v = 0;
      for (int k = 0; k < 3; ++k) v += (uint64_t)h_stage[3 * i + k] << (22 * k);
      tmp[i] = v;
    }
    HIP_OK(hipMemcpyAsync(buf, tmp.data(), n * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
    HIP_OK(hipStreamSynchronize(stream));
    return 0;
  }
  unsigned long long* cost_fx(int set) const {
    return reinterpret_cast<unsigned long long*>(d_scal + S_CFX + (size_t)kFxWords * set);
  }
  // cost of the last evaluation pass summed over ranks (fixed point or double slots)
  int allreduce_cost() {
    if (cost_fx_pending) return allreduce_u64(reinterpret_cast<uint64_t*>(cost_fx(fx_last)), kFxWords);
    return allreduce(d_scal + S_COST, 2, ncclSum);
  }

  int allreduce(double* buf, size_t n, ncclRedOp_t op) {
    if (!coll() || n == 0) return 0;
    if (p2p_main && n <= kP2pWords && (op == ncclSum || op == ncclMax))
      return op == ncclSum ? p2p_allreduce_sum(p2p_main, stream, buf, n) : p2p_allreduce_max(p2p_main, stream, buf, n);
    if (host_cb) return host_allreduce(buf, n, op == ncclMax ? 1 : 0);
    NCCL_OK(ncclAllReduce(buf, buf, n, ncclDouble, op, comm, stream));
    return 0;
  }
  // max over ranks of small int flag arrays
  int allreduce_max_i32(int* buf, int n) {
    if (!coll() || n == 0) return 0;
    if (p2p_main) return p2p_allreduce_max_i32(p2p_main, stream, buf, (size_t)n);
    if (!host_cb) {
      NCCL_OK(ncclAllReduce(buf, buf, n, ncclInt32, ncclMax, comm, stream));
      return 0;
    }
    int tmp[16];
    if (n > 16) return set_error(DAB_E_INVALID, "flag all-reduce too large");
    CHECK_RC(stage(n));
    HIP_OK(hipMemcpyAsync(tmp, buf, n * sizeof(int), hipMemcpyDeviceToHost, stream));
    HIP_OK(hipStreamSynchronize(stream));
    for (int i = 0; i < n; ++i) h_stage[i] = tmp[i];
    if (host_cb(h_stage, n, 1, host_user) != 0) return set_error(DAB_E_COMM, "host all-reduce callback failed");
    for (int i = 0; i < n; ++i) tmp[i] = (int)h_stage[i];
    HIP_OK(hipMemcpyAsync(buf, tmp, n * sizeof(int), hipMemcpyHostToDevice, stream));
    HIP_OK(hipStreamSynchronize(stream));
    return 0;
  }
};

inline int bits_for(long long maxval) {  // radix-sort end bit for keys in [0, maxval]
  int b = 1;
  while (b < 31 && (1LL << b) <= maxval) ++b;
  return b;
}

// ---- dab_handle.hip ----
int guard_fail(dab_handle* h, const char* where, Dev* extra = nullptr);

// ---- dab_problem.hip: the free-intrinsic state ----
bool intr_mask_any(const dab_handle* h);
int intr_free_set(dab_handle* h, bool with_mask, int* nfi_out, int* nscal_out = nullptr);
int intr_eval(dab_handle* h);

// ---- dab_problem.hip: constant points ----
// the constant set of the mask on the handle -> h->d_ptc / h->n_pt_const (uploaded when changed)
int pt_const_sync(dab_handle* h);

// ---- dab_problem.hip: constant scalars of an extrinsic ----
// the effective set of the mask on the handle -> h->d_exs / h->n_ext_sub (uploaded when changed)
int ext_sub_sync(dab_handle* h);

// ---- dab_problem.hip: extrinsic priors ----
// the effective set of the priors on the handle -> lz.d_prior_* / h->n_prior (uploaded when changed)
int prior_sync(dab_handle* h);
// 0.5 sum |r|^2 of the effective priors as the last evaluation left it in h_scal (0 without any)
inline double prior_cost(const Handle* h) { return h->n_prior > 0 ? h->h_scal[S_PRIOR] : 0.0; }

// ---- dab_problem.hip: point priors ----
// this rank's effective set of the point priors on the handle -> lz.d_ptp_* / h->n_pt_prior
// (uploaded when changed; no collective). After pt_const_sync.
int pt_prior_sync(dab_handle* h);
// What a call decides once for all ranks, after pt_const_sync and pt_prior_sync, with one
// max-reduce of two words on a multi-rank handle (none on one rank): *points_state = 2 when some
// rank has a free referenced point, 1 when none has and some rank has a constant one, 0 without
// referenced points; h->pt_prior_any = some rank has an effective point prior.
int call_state(dab_handle* h, int* points_state);
// 0.5 sum |r|^2 of the effective point priors of all ranks as the last evaluation left it in h_scal
inline double pt_prior_cost(const Handle* h) { return h->pt_prior_any ? h->h_scal[S_PPRIOR] : 0.0; }

// ---- dab_problem.hip: intrinsic priors ----
// the effective set of the priors on the handle for the free set now on it (nfi: its size, after
// intr_free_set / cam_system_free_set; 0 = none) -> lz.d_zp_* / h->n_zprior (uploaded when changed)
int zprior_sync(dab_handle* h, int nfi);
// zg[column] += A^T A | A^T r and S_ZPRIOR, after intr_eval's sum over the ranks (no effective
// prior: no launch)
void zprior_blocks(dab_handle* h);
// 0.5 sum |r|^2 of the effective priors as the last evaluation left it in h_scal (0 without any)
inline double zprior_cost(const Handle* h) { return h->n_zprior > 0 ? h->h_scal[S_ZPRIOR] : 0.0; }

// ---- dab_schur_tables.hip: tables and buffers of the linear solvers, built on first use ----
int build_schur_tables(dab_handle* h);
int build_pcg_buffers(dab_handle* h);

// ---- dab_solver.hip ----
int eval_pass(dab_handle* h, bool camtab_ready, hipEvent_t ev_mid = nullptr, hipEvent_t ev_end = nullptr,
              hipEvent_t ev_pair0 = nullptr, hipEvent_t ev_pair1 = nullptr, bool* pair_rec = nullptr);
int eval_jacobian_and_blocks(dab_handle* h, bool with_norms, bool tables_current = false);
int xerr_fail(unsigned long long e);
int read_scalars(dab_handle* h);
void launch_jacobi_scale(dab_handle* h, int nfi, int on);
// The camera system of the exact step, shared by dab_solve and the covariance: the dense buffer
// S (n' rows and the rhs row, at ld) and its solution yc — the handle's plain buffers, or with
// free intrinsics the bordered ones
struct CamSystem {
  double* S = nullptr;
  int ld = 0;
  double* yc = nullptr;
  int n = 0, n2 = 0;         // 6 NC, n + 6 nfi
  int nfi = 0, nz_scal = 0;  // free intrinsics and their active scalars
};
int cam_system_free_set(dab_handle* h, const char* refuse_any, CamSystem* cs);
int cam_system_buffers(dab_handle* h, bool factor, CamSystem* cs);
int cam_system_assemble(dab_handle* h, const CamSystem& cs, const StepScalars& sc, double x_cost, bool with_pm);
int intr_border_rows(dab_handle* h, int nfi, const StepScalars& sc, double* S, int ld);

}  // namespace dab

struct dab_handle : dab::Handle {};
