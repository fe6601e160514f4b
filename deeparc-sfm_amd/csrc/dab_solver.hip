// dab_solver.hip — device-resident trust-region LM driver (dab_solve) and its building blocks.
//
// Replaces ceres::Solve(options{DENSE_SCHUR}, &problem, &summary) as called by
// solve() at src/sfm.cc:31-75. The minimizer mirrors Ceres' TrustRegionMinimizer +
// LevenbergMarquardtStrategy: Jacobi scaling computed at iteration 0,
// LM diagonal clamp [1e-6, 1e32] / radius, step quality = actual/model decrease,
// radius /= max(1/3, 1-(2q-1)^3) on accept, /= decrease_factor (doubling) on reject,
// parameter / function / gradient tolerance tests in Ceres' order, five consecutive
// invalid steps => FAILURE, final_cost = min over iteration costs. The step solves
// (Js^T Js + D^2) y = Js^T r exactly: points are eliminated per point (3x3 Cholesky)
// and the reduced camera system is factored densely (dab_chol.hip) — DENSE_SCHUR.
//
// Multi-GPU: one process per GPU, observations sharded by point; the camera-side
// normal-equation pieces (U, g_c, the reduced system S and its rhs) and the scalar
// reductions are all-reduced with RCCL over xGMI; every rank then factors the same S
// and back-substitutes its own points.
#include "dab_handle.h"
#include "dab_warm.h"

using namespace dab;

// S vec (Y part) -> d_pcg_w, all-reduced across ranks
// exact: the fp64 product even in a mixed-precision solve (the true residual r = b - S x)
static int pcg_matvec(dab_handle* h, YBufs yb, const double* vec, bool exact = false) {
  hipStream_t s = h->stream;
  // the stored-Y products all-reduce into d_pcg_w; only the one-rank matrix-free product
  // hands its work-group partials to the CG update (never left over from an earlier problem)
  h->cg_wpart = nullptr;
  if (h->mf) {
    // one rank with cross blocks (the rig): the product's partials are summed inside the CG
    // update (no all-reduce in between), one launch fewer per iteration. A one-rank RCCL
    // handle takes this path too (its all-reduce of a single rank is the identity, and the
    // separate partial-sum launch would regroup the sums: the trajectory would leave
    // dab_create's in the last bits)
    const bool fuse = h->world == 1 && h->nxlist > 0 && h->knobs.cg_onewg == 0;
    h->cg_wpart = fuse ? h->d_mf_partial : nullptr;
    double* w = fuse ? nullptr : h->d_pcg_w;
    if (h->mf32 && !exact)
      launch_mf_product32(s, h->view, h->d_points, h->d_camtab, h->d_scale_c, h->d_L, vec, h->d_mf_partial, w,
                          h->mf_grid_n, h->d_pcg_state);
    else
      launch_mf_product(s, h->view, h->d_points, h->d_camtab, h->d_scale_c, h->d_L, vec, h->d_mf_partial, w,
                        h->mf_grid_n, h->d_pcg_state);
    if (!fuse) CHECK_RC(h->allreduce(h->d_pcg_w, (size_t)6 * h->NC, ncclSum));
    return 0;
  }
  if (h->fused_grid > 0) {
    launch_pcg_fused(s, h->view, yb, vec, h->d_fused_partial, h->d_pcg_w, h->fused_grid, h->d_pcg_state);
    CHECK_RC(h->allreduce(h->d_pcg_w, (size_t)6 * h->NC, ncclSum));
    return 0;
  }
  const bool direct = h->nchunk == h->NC;
  launch_pcg_matvec_passes(s, h->view, h->nchunk, h->d_chunk_beg, yb, vec, h->d_pcg_t,
                           direct ? h->d_pcg_w : h->d_partial, h->d_pcg_state);
  if (!direct) launch_seg_final(s, h->NC, 6, h->d_seg_chunk, h->d_partial, h->d_pcg_w, h->max_seg_chunks);
  CHECK_RC(h->allreduce(h->d_pcg_w, (size_t)6 * h->NC, ncclSum));
  return 0;
}

// Solve S y = b (scaled, damped reduced camera system) into d_yc with preconditioned CG.
// Requires d_L, d_q (point factor) and d_Y (entry_y) of this step. Returns the number of
// CG iterations in *iters and the final PcgState status in *status.
static int pcg_solve(dab_handle* h, const dab_options& opt, StepScalars sc, YBufs yb, int* iters, int* status) {
  hipStream_t s = h->stream;
  const DevView& v = h->view;
  const int NC = h->NC;
  const bool direct = h->nchunk == h->NC;
  if (h->mf)
    launch_mf_diag_rhs(s, v, h->nchunk, h->d_run_beg, h->d_run_rec, h->d_points, h->d_camtab, h->d_scale_c, h->d_L,
                       h->d_q, direct ? h->d_pcg_red : h->d_partial);
  else
    launch_pcg_diag_rhs_partial(s, v, h->nchunk, h->d_chunk_beg, h->d_run, yb, h->d_q,
                                direct ? h->d_pcg_red : h->d_partial);
  if (!direct) launch_seg_final(s, NC, 27, h->d_seg_chunk, h->d_partial, h->d_pcg_red, h->max_seg_chunks);
  CHECK_RC(h->allreduce(h->d_pcg_red, (size_t)27 * NC, ncclSum));
  launch_pcg_setup(s, NC, h->ug(), h->d_scale_c, sc, h->d_pcg_red, h->d_pcg_Ad, h->d_pcg_Minv, h->d_pcg_b,
                   h->d_yc, h->d_pcg_r, h->d_flags + 1);
  const int max_it = std::max(0, opt.max_linear_solver_iterations);
  // constant scalars of an extrinsic: unit diagonal instead of min_lm_diagonal / radius in the
  // operator's and the preconditioner's blocks (their rows and columns are exact zeros, b too)
  launch_ext_unit_blocks(s, NC, h->d_exs, h->d_pcg_Ad, h->d_pcg_Minv);
  launch_pcg_init(s, NC, h->d_pcg_b, h->d_flags + 1, h->d_pcg_state, opt.eta, opt.min_linear_solver_iterations,
                  max_it, h->d_pcg_Minv, h->d_pcg_r, h->d_pcg_z, h->d_pcg_p);
  const int* xptr = h->nxlist > 0 ? h->d_xptr : nullptr;
  // the CG update: spread over work-groups (default) or one work-group (DAB_CG_ONEWG=1)
  const bool onewg = h->knobs.cg_onewg != 0;
  auto update = [&](int mode) {
    if (onewg)
      launch_pcg_update(s, NC, mode, h->d_pcg_Ad, h->d_pcg_w, xptr, h->d_xlist, h->d_cross_cam, h->Ux(),
                        h->d_scale_c, h->d_pcg_b, h->d_pcg_p, h->d_pcg_q, h->d_yc, h->d_pcg_r, h->d_pcg_state,
                        h->d_pcg_Minv, h->d_pcg_z);
    else
      launch_cg_update(s, NC, mode, h->d_pcg_Ad, h->d_pcg_w, xptr, h->d_xlist, h->d_cross_cam, h->Ux(),
                       h->d_scale_c, h->d_pcg_b, h->d_pcg_p, h->d_pcg_q, h->d_yc, h->d_pcg_r, h->d_pcg_state,
                       h->d_pcg_Minv, h->d_pcg_z, h->d_cg_partial, h->d_cg_cnt, h->cg_wpart, h->mf_grid_n);
  };
  // CG iterations are enqueued in batches between reads of the device-side state. The
  // first batch is the previous solve's count + 2 (counts change slowly between LM
  // iterations); a finished CG turns the rest of a batch into no-op launches (~4.5 us
  // each), a read costs a host round trip (~25 us).
  int done = 0, batch = std::min(32, std::max(2, h->pcg_hint + 2));
  for (;;) {
    for (int j = 0; j < batch && done < max_it; ++j) {
      ++done;
      CHECK_RC(pcg_matvec(h, yb, h->d_pcg_p));
      const bool reset = done % 10 == 0;  // r = b - S x every 10th iteration
      update(reset ? 1 : 0);
      if (reset) {
        CHECK_RC(pcg_matvec(h, yb, h->d_yc, true));
        update(2);
      }
    }
    HIP_OK(hipMemcpyAsync(h->h_pcg_state, h->d_pcg_state, sizeof(PcgState), hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    if (h->h_pcg_state->status != kPcgRunning || done >= max_it) break;
    batch = batch < 4 ? 4 : std::min(2 * batch, 32);
  }
  h->pcg_hint = h->h_pcg_state->iter;
  *iters = h->h_pcg_state->iter;
  *status = h->h_pcg_state->status;
  return 0;
}

// ------------------------------------------------------------------------------------
// evaluation building blocks
// ------------------------------------------------------------------------------------
// The evaluation pass proper (the benchmark "step"), matrix-free. The camera side goes
// first (k_eval_cams -> U, g_c; k_eval_cross -> arc∘ring blocks) so that, on several
// GPUs, its RCCL all-reduce runs on comm_stream while the point-side kernel
// (k_eval_points -> V, g, cost) runs on the main stream. Expects the camera tables of
// the current x in d_camtab. ev_mid / ev_end (nullable) bracket the point kernel.
// camtab_ready: the caller has just built the camera tables (the LM step needs them for
// later passes); otherwise they are built here only if a pass of this problem reads them.
int dab::eval_pass(dab_handle* h, bool camtab_ready, hipEvent_t ev_mid, hipEvent_t ev_end, hipEvent_t ev_pair0,
                   hipEvent_t ev_pair1, bool* pair_rec) {
  hipStream_t s = h->stream;
  const DevView& v = h->view;
  bool overlapped = false;
  if (!h->knobs.eval_side_ok())
    return set_error(DAB_E_INVALID, "DAB_EVAL_SIDE=" + std::to_string(h->knobs.eval_side) +
                                        " is a timing ablation (wrong results): only -DDAB_ABLATIONS builds run it");
  // the fused pass reads the tables when the caller has them (the LM loop) — C3: 21.3
  // against 23.2 us per launch — but does not launch a table build of its own for them
  // (k_cam_tables in front of the pass cost more than it saves: 25.6 against 23.9 us per
  // step), unless DAB_FUSED_TAB=1 asks for it
  const bool fused_tab = h->fused && (h->knobs.fused_tab > 0 || (h->knobs.fused_tab < 0 && camtab_ready));
  const bool need_tab = (h->NC > 0 && (h->chunks.ngen > 0 || h->ncross > 0)) || eval_points_needs_camtab(h->eval_wps) ||
                        fused_tab;
  if (!camtab_ready && need_tab) launch_cam_tables(s, h->E, h->d_ext, h->d_camtab);
  const bool fx = h->fused || eval_points_fx(h->eval_wps);
  if (fx) h->fx_last ^= 1;  // this pass adds into set fx_last and zeroes the other
  h->cost_fx_pending = fx;
  if (h->fused && !h->fused_split && ev_mid) HIP_OK(hipEventRecord(ev_mid, s));
  // k_eval_bal: both traversal orders in one launch (side 0), or one side per launch
  auto eval_fused = [&](int grid, int side) {
    launch_eval_bal(s, v, h->d_chunk_beg, h->d_points, h->d_ext, fused_tab ? h->d_camtab : nullptr, h->d_V, h->d_g,
                    h->ug(), h->cost_fx(h->fx_last), h->cost_fx(h->fx_last ^ 1), h->xerr(), grid, side);
  };
  // DAB_EVAL_SIDE=7: the test's frame wait that never completes; ablation builds: 1..6
  const int test_flag = h->knobs.eval_side == 7 ? kSideTestTimeout : 0;
  if (h->fused && !h->fused_split) {  // both halves of the pass in one launch
    eval_fused(h->ncu, h->knobs.eval_side == 7 ? kSideBoth | test_flag : h->knobs.eval_side);
    if (ev_end) HIP_OK(hipEventRecord(ev_end, s));
    if (h->NC > 0) CHECK_RC(h->allreduce(h->d_camred, h->camred_count(), ncclSum));
    return 0;
  }
  if (h->fused) {
    // several ranks: the same kernel as two launches, the camera side first so that its
    // RCCL all-reduce runs on the communication stream during the point side (which
    // leaves one CU per XCD free for it: eval_grid)
    if (ev_mid) HIP_OK(hipEventRecord(ev_mid, s));
    eval_fused(h->ncu, kSideCams | test_flag);
    bool ovl = false;
    if (h->can_overlap()) {
      HIP_OK(hipEventRecord(h->ev_cam, s));
      HIP_OK(hipStreamWaitEvent(h->comm_stream, h->ev_cam, 0));
      CHECK_RC(h->allreduce_comm_stream(h->d_camred, h->camred_count()));
      HIP_OK(hipEventRecord(h->ev_comm, h->comm_stream));
      ovl = true;
    } else {
      CHECK_RC(h->allreduce(h->d_camred, h->camred_count(), ncclSum));
    }
    eval_fused(h->eval_grid, kSidePoints);
    if (ev_end) HIP_OK(hipEventRecord(ev_end, s));
    if (ovl) HIP_OK(hipStreamWaitEvent(s, h->ev_comm, 0));
    return 0;
  }
  if (h->NC > 0 && h->pair_eval) {
    // the composed observations pair-major (camera halves + cross blocks in one pass),
    // the other entries camera-major, then one fixed-order sum per camera
    DevView v2 = v;
    v2.cm_idx = h->d_cm2_idx;
    v2.cm_xy = h->d_cm2_xy;
    launch_eval_cams_gen(s, v2, h->nchunk2, h->d_chunk2_beg, h->d_points, h->d_ext, h->d_camtab, h->d_partial2);
    if (ev_pair0) HIP_OK(hipEventRecord(ev_pair0, s));
    launch_eval_pair(s, v, h->nxchunk, h->d_xchunk_beg, h->d_x_idx, h->d_x_xy, h->d_points, h->d_camtab,
                     h->d_xpartial, h->d_xcpart, h->pair_uni_intr);
    if (ev_pair1) HIP_OK(hipEventRecord(ev_pair1, s));
    if (pair_rec) *pair_rec = ev_pair0 && ev_pair1 && h->nxchunk > 0;
    launch_cam_final(s, h->NC, h->d_seg2_chunk, h->d_partial2, h->d_xcam_ptr, h->d_xcam_list, h->d_xcpart, h->ug());
    launch_seg_final(s, h->ncross, 36, h->d_xseg_chunk, h->d_xpartial, h->Ux(), h->max_xseg_chunks);
  } else if (h->NC > 0) {
    // one chunk per camera: the chunk kernels write the camera rows directly
    const bool direct = h->nchunk == h->NC;
    launch_eval_cams(s, v, h->chunks, h->d_chunk_beg, h->d_points, h->d_ext, h->d_camtab,
                     direct ? h->ug() : h->d_partial);
    if (!direct) launch_seg_final(s, h->NC, 27, h->d_seg_chunk, h->d_partial, h->ug(), h->max_seg_chunks);
  }
  if (h->NC > 0) {
    if (h->ncross > 0 && !h->pair_eval) {
      if (h->nxchunk > 0) {
        launch_eval_cross(s, v, h->nxchunk, h->d_xchunk_beg, h->d_x_idx, h->d_x_xy, h->d_points, h->d_camtab,
                          h->d_xpartial);
        launch_seg_final(s, h->ncross, 36, h->d_xseg_chunk, h->d_xpartial, h->Ux(), h->max_xseg_chunks);
      } else {
        HIP_OK(hipMemsetAsync(h->Ux(), 0, sizeof(double) * 36 * (size_t)h->ncross, s));
      }
    }
    if (h->can_overlap()) {
      HIP_OK(hipEventRecord(h->ev_cam, s));
      HIP_OK(hipStreamWaitEvent(h->comm_stream, h->ev_cam, 0));
      CHECK_RC(h->allreduce_comm_stream(h->d_camred, h->camred_count()));
      HIP_OK(hipEventRecord(h->ev_comm, h->comm_stream));
      overlapped = true;
    } else {
      CHECK_RC(h->allreduce(h->d_camred, h->camred_count(), ncclSum));
    }
  }
  if (ev_mid) HIP_OK(hipEventRecord(ev_mid, s));
  launch_eval_points(s, h->view, h->d_points, h->d_ext, h->d_camtab, h->d_V, h->d_g, h->d_gpart, h->d_arrivals,
                     h->d_scal + S_COST, h->cost_fx(h->fx_last), h->cost_fx(h->fx_last ^ 1), h->eval_grid,
                     h->eval_wps);
  if (ev_end) HIP_OK(hipEventRecord(ev_end, s));
  if (overlapped) HIP_OK(hipStreamWaitEvent(s, h->ev_comm, 0));
  return 0;
}

// Residual + Jacobian at the current x and the J^T J / J^T r blocks (camera side
// all-reduced). Leaves cost / gradient scalars in d_scal (point parts all-reduced).
// tables_current: d_camtab already holds the tables of d_ext (after an accepted step, the
// candidate's tables swapped in with its parameters), so none are built here
int dab::eval_jacobian_and_blocks(dab_handle* h, bool with_norms, bool tables_current) {
  hipStream_t s = h->stream;
  if (!tables_current) launch_cam_tables(s, h->E, h->d_ext, h->d_camtab);
  CHECK_RC(eval_pass(h, true));
  // extrinsic priors: A^T A | A^T r into the camera rows, after the pass's sum over the ranks (the
  // overlapped one too) and before the norms, the Jacobi scale and every step kernel read them
  launch_prior_blocks(s, h->n_prior, h->lz.d_prior_idx, h->lz.d_prior_rec, h->d_ext, h->ug(), h->lz.d_prior_part,
                      h->lz.d_prior_cnt, h->d_scal + S_PRIOR);
  // point priors: A^T A | A^T r into this rank's V | g (a point belongs to one rank), before the
  // point gradient's norms, the Jacobi scale and the point factor read them. A rank without any,
  // where another has one, leaves a zero for the sum over the ranks
  if (h->n_pt_prior > 0)
    launch_pt_prior_blocks(s, h->n_pt_prior, h->NP, h->lz.d_ptp_idx, h->lz.d_ptp_rec, h->d_points, h->d_V, h->d_g,
                           h->lz.d_ptp_part, h->lz.d_ptp_cnt, h->d_scal + S_PPRIOR);
  else if (h->pt_prior_any)
    HIP_OK(hipMemsetAsync(h->d_scal + S_PPRIOR, 0, sizeof(double), s));
  if (with_norms) {
    launch_grad_points_m(s, h->NP, h->d_points, h->d_g, h->d_gpart, h->red_grid, h->d_ptc);
    launch_final_sum(s, h->red_grid, 3, h->d_gpart, h->d_scal + S_GMAX_P, 1u);
    launch_cam_norms_x(s, h->E, h->d_ext_col, h->d_ext, nullptr, h->NC > 0 ? h->ug() : nullptr,
                       h->d_scal + S_CAM0, h->d_exs);
  }
  // cross-rank: sums of cost, bad, gnorm, xnorm; max of gmax
  CHECK_RC(h->allreduce_cost());
  if (h->pt_prior_any) CHECK_RC(h->allreduce(h->d_scal + S_PPRIOR, 1, ncclSum));
  if (with_norms) {
    CHECK_RC(h->allreduce(h->d_scal + S_GMAX_P, 1, ncclMax));
    CHECK_RC(h->allreduce(h->d_scal + S_GNORM_P, 2, ncclSum));
  }
  return 0;
}

// k_eval_bal's error bits: a bounded work-group wait timed out, the pass's results are void
int dab::xerr_fail(unsigned long long e) {
  return set_error(DAB_E_DEVICE, "evaluation pass: a work-group wait timed out (code " + std::to_string(e) + ")");
}
int dab::read_scalars(dab_handle* h) {
  HIP_OK(hipMemcpyAsync(h->h_scal, h->d_scal, sizeof(double) * S_NSLOTS, hipMemcpyDeviceToHost, h->stream));
  HIP_OK(hipMemcpyAsync(h->h_flags, h->d_flags, sizeof(int) * 4, hipMemcpyDeviceToHost, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));
  // a one-shot all-reduce that gave up waiting for a peer poisons its output: stop here,
  // before any decision is taken on it (every rank's next call fails the same way)
  CHECK_RC(p2p_check(h->p2p_main));
  CHECK_RC(p2p_check(h->p2p_comm));
  if (h->cost_fx_pending) {
    // the last evaluation pass left its cost in fixed point (cost_fx_commit): exact
    // integer limb sums, converted once here. Its error bits (kFxErr) were summed over the
    // ranks with the cost (allreduce_cost), so a wait that ran out on any rank fails this
    // call on every rank, before any decision is taken on the pass
    unsigned long long w[kFxWords];
    std::memcpy(w, h->h_scal + S_CFX + (size_t)kFxWords * h->fx_last, sizeof(w));
    h->cost_fx_pending = false;
    if (const unsigned long long e = cost_fx_err(w)) {
      HIP_OK(hipMemsetAsync(h->d_scal + S_XERR, 0, sizeof(double), h->stream));  // reported here
      HIP_OK(hipStreamSynchronize(h->stream));
      return xerr_fail(e);
    }
    cost_fx_total(w, h->h_scal[S_COST], h->h_scal[S_COST_BAD]);
  }
  return 0;
}

// Jacobi scaling s = 1/(1+sqrt(diag(J^T J))), computed once at iteration 0.
__global__ void k_scale_points(int NP, const double* __restrict__ V, double* __restrict__ sp, int on) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 3 * NP) return;
  const int k = i / NP, p = i - k * NP;
  const int vi = k == 0 ? 0 : (k == 1 ? 3 : 5);
  sp[i] = on ? 1.0 / (1.0 + sqrt(V[(size_t)vi * NP + p])) : 1.0;
}
__global__ void k_scale_cams(int NC, const double* __restrict__ ug, double* __restrict__ sc, int on) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 6 * NC) return;
  const int c = i / 6, a = i - 6 * c;
  const int q = a * 6 - (a * (a - 1)) / 2;  // (a,a) in the packed upper layout
  sc[i] = on ? 1.0 / (1.0 + sqrt(ug[27 * (size_t)c + q])) : 1.0;
}
// the scales of the points, the cameras and the nfi free intrinsics from the blocks at x
void dab::launch_jacobi_scale(dab_handle* h, int nfi, int on) {
  hipStream_t s = h->stream;
  const int NP = h->NP, NC = h->NC;
  if (h->d_ptc) launch_scale_points_m(s, NP, h->d_V, h->d_scale_p, on, h->d_ptc);
  else k_scale_points<<<grid_for(3 * NP, 256, 1 << 20), 256, 0, s>>>(NP, h->d_V, h->d_scale_p, on);
  if (h->d_exs) launch_scale_cams_x(s, NC, h->ug(), h->d_scale_c, on, h->d_exs);
  else if (NC > 0) k_scale_cams<<<grid_for(6 * NC, 256, 1 << 20), 256, 0, s>>>(NC, h->ug(), h->d_scale_c, on);
  launch_intr_scale(s, nfi, h->lz.d_zg, h->lz.d_intr_act, h->lz.d_sz, on);
}
DAB_WARM_TU(k_scale_points);

static void print_header() {
  std::printf("iter      cost      cost_change  |gradient|   |step|    tr_ratio  tr_radius  ls_iter  iter_time  total_time\n");
}
static void print_iter(const dab_iteration& it, double total) {
  std::printf("%4d % 3.6e % 3.2e % 3.2e % 3.2e % 3.2e % 3.2e %4d % 3.2e % 3.2e\n", it.iteration, it.cost,
              it.cost_change, it.gradient_max_norm, it.step_norm, it.relative_decrease, it.trust_region_radius,
              it.linear_solver_iterations, it.iteration_time_in_seconds, total);
  std::fflush(stdout);
}

// Wall-clock since solve start, maxed over ranks so every rank takes the
// "Maximum solver time reached" exit on the same iteration. Returns < 0 on error.
static double elapsed_collective(dab_handle* h, double local) {
  if (!h->coll()) return local;
  hipStream_t s = h->stream;
  h->h_scal[S_TIME] = local;
  if (hipMemcpyAsync(h->d_scal + S_TIME, &h->h_scal[S_TIME], sizeof(double), hipMemcpyHostToDevice, s) != hipSuccess)
    return -1.0;
  if (h->allreduce(h->d_scal + S_TIME, 1, ncclMax) != 0) return -1.0;
  if (hipMemcpyAsync(&h->h_scal[S_TIME], h->d_scal + S_TIME, sizeof(double), hipMemcpyDeviceToHost, s) != hipSuccess)
    return -1.0;
  if (hipStreamSynchronize(s) != hipSuccess) return -1.0;
  return h->h_scal[S_TIME];
}

// ------------------------------------------------------------------------------------
// dab_solve: the trust-region LM loop
// ------------------------------------------------------------------------------------
static int solve_impl(dab_handle* h, const dab_options* opt_in, dab_summary* sum);
extern "C" int dab_solve(dab_handle* h, const dab_options* opt_in, dab_summary* sum) {
  const int rc = solve_impl(h, opt_in, sum);
  CHECK_RC(guard_fail(h, "dab_solve"));
  return rc;
}
extern "C" int dab_set_loss(dab_handle* h, int32_t loss_type, double scale) {
  clear_error();
  if (!h) return set_error(DAB_E_INVALID, "null handle");
  if (loss_type != DAB_LOSS_TRIVIAL && loss_type != DAB_LOSS_HUBER && loss_type != DAB_LOSS_SOFT_L1 &&
      loss_type != DAB_LOSS_CAUCHY)
    return set_error(DAB_E_INVALID, "unknown loss type");
  if (loss_type == DAB_LOSS_TRIVIAL) scale = 1.0;  // ignored
  if (!(std::isfinite(scale) && scale > 0.0)) return set_error(DAB_E_INVALID, "loss scale must be finite and > 0");
  // launches copy the view by value: passes already enqueued keep the loss they were launched with
  h->view.loss = loss_type;
  h->view.loss_a = scale;
  h->view.loss_b = scale * scale;
  h->view.loss_c = 1.0 / h->view.loss_b;
  h->loss_scale = scale;
  return 0;
}
extern "C" int dab_get_loss(dab_handle* h, int32_t* loss_type, double* scale) {
  clear_error();
  if (!h) return set_error(DAB_E_INVALID, "null handle");
  if (loss_type) *loss_type = h->view.loss;
  if (scale) *scale = h->view.loss == DAB_LOSS_TRIVIAL ? 0.0 : h->loss_scale;
  return 0;
}

// The system with the block z (nfi > 0): the handle's dense buffer of n' = 6 NC + 6 nfi rows (+
// the rhs row) at ldz, the solution and border-sum buffers, which free intrinsics each point sees
// (k_intr_ptmask) and the border kernels' partials.
static int intr_system_buffers(dab_handle* h, int nfi) {
  if (nfi <= 0) return 0;
  const int n2 = 6 * h->NC + 6 * nfi;
  h->ldz = ((n2 + 1 + 7) / 8) * 8;
  if (h->ldz % 512 == 0) h->ldz += 8;
  const size_t need = (size_t)(n2 + 1) * h->ldz;
  if (need > h->lz.Sz_cap) {
    h->dev.drop(h->lz.d_Sz);
    h->lz.d_Sz = nullptr;
    h->lz.Sz_cap = 0;
    CHECK_RC(h->dev.alloc(&h->lz.d_Sz, need));
    h->lz.Sz_cap = need;
  }
  if (!h->lz.d_yz) {
    CHECK_RC(h->dev.alloc(&h->lz.d_yz, (size_t)6 * h->NC + 6 * kIntrFreeMax));
    CHECK_RC(h->dev.alloc(&h->lz.d_bsum, (size_t)6 * kIntrFreeMax * (6 * (size_t)h->NC + 6 * kIntrFreeMax + 1)));
    CHECK_RC(h->dev.alloc(&h->lz.d_ptmask, (size_t)std::max(1, h->NP)));
  }
  launch_intr_ptmask(h->stream, h->view, h->lz.d_intr_meta, h->lz.d_ptmask);
  int spg = 1;
  const size_t bneed = (size_t)intr_border_groups(h->view.nslice, h->NC, nfi, &spg) * (size_t)(6 * nfi) * (n2 + 1);
  if (bneed > h->lz.bpart_cap) {
    h->dev.drop(h->lz.d_bpart);
    h->lz.d_bpart = nullptr;
    h->lz.bpart_cap = 0;
    CHECK_RC(h->dev.alloc(&h->lz.d_bpart, bneed));
    h->lz.bpart_cap = bneed;
  }
  return 0;
}
// The rows of the block z of S (n' x n' at ld, the leading n x n part and the rhs row n built by
// either assembly): the rhs moves to row n', then the border sums (one point-major pass),
// all-reduced and scattered into S
int dab::intr_border_rows(dab_handle* h, int nfi, const StepScalars& sc, double* S, int ld) {
  if (nfi <= 0) return 0;
  hipStream_t s = h->stream;
  const int n = 6 * h->NC, n2 = n + 6 * nfi;
  HIP_OK(hipMemcpyAsync(S + (size_t)n2 * ld, S + (size_t)n * ld, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice,
                        s));
  launch_intr_border(s, h->view, h->d_points, h->d_camtab, h->d_scale_c, h->d_L, h->d_q, h->lz.d_sz, h->lz.d_intr_meta,
                     h->lz.d_ptmask, nfi, h->lz.d_bpart, h->lz.d_bsum, h->knobs.intr_border_lds != 0);
  CHECK_RC(h->allreduce(h->lz.d_bsum, (size_t)(6 * nfi) * (size_t)(n2 + 1), ncclSum));
  launch_intr_scatter(s, n, nfi, h->lz.d_bsum, h->lz.d_zg, h->lz.d_sz, h->lz.d_intr_act, sc, S, ld);
  return 0;
}

// The free intrinsics that join the camera system (the handle's mask) and the refusals every
// caller shares, before anything on the handle changes. refuse_any: the caller's own reason to
// refuse a non-empty set (null: none).
int dab::cam_system_free_set(dab_handle* h, const char* refuse_any, CamSystem* cs) {
  cs->nfi = cs->nz_scal = 0;
  if (!intr_mask_any(h)) return 0;
  CHECK_RC(intr_free_set(h, true, &cs->nfi, &cs->nz_scal));
  if (cs->nfi > 0 && refuse_any) return set_error(DAB_E_UNSUPPORTED, refuse_any);
  if (cs->nfi > kIntrFreeMax) return set_error(DAB_E_UNSUPPORTED, "more than 16 free intrinsics");
  if (cs->nfi > 0 && h->NC == 0) return set_error(DAB_E_UNSUPPORTED, "free intrinsics need a free extrinsic");
  return 0;
}
// The buffers of the system for cs->nfi free intrinsics (the tables of the step are built):
// with the block z its own dense buffer of n' = 6 NC + 6 nfi rows (+ rhs row). factor: the dense
// factorisation's scratch and captured graph too, which belong to the set-up, not to the first
// step (kept while the camera count and the buffers stay the same)
int dab::cam_system_buffers(dab_handle* h, bool factor, CamSystem* cs) {
  const int nfi = cs->nfi;
  cs->n = 6 * h->NC;
  cs->n2 = cs->n + 6 * nfi;
  CHECK_RC(intr_system_buffers(h, nfi));
  cs->S = nfi > 0 ? h->lz.d_Sz : h->d_S;
  cs->ld = nfi > 0 ? h->ldz : h->lds;
  cs->yc = nfi > 0 ? h->lz.d_yz : h->d_yc;
  if (factor && h->NC > 0 && chol_prepare(h->chol, h->stream, cs->n2, cs->S, cs->ld, cs->yc, h->d_flags + 1) != 0)
    return set_error(DAB_E_DEVICE, "dense Cholesky set-up failed");
  return 0;
}
// S of one step (NC > 0): its leading n x n part and the rhs row n, summed over the ranks; the
// border rows of the block z come after it. x_cost scales the tile path's fixed-point rhs: the
// cost of everything that enters q_p, the observations and the point priors of all ranks.
// with_pm: the point-major Y planes too (the back substitution of dab_solve's pair-table path
// reads them). The Y records are fp64 and go to d_Yrec: fp32 records exist only in the PCG.
int dab::cam_system_assemble(dab_handle* h, const CamSystem& cs, const StepScalars& sc, double x_cost, bool with_pm) {
  hipStream_t s = h->stream;
  const DevView& v = h->view;
  const int NC = h->NC;
  if (h->schur_tiles) {
    // S by register-owned block tiles over the records' Y (re-evaluated once per step)
    SchurTiles a = h->tiles;
    a.kq = 0;
    if (x_cost > 0.0 && std::isfinite(x_cost)) {
      int e2;
      (void)std::frexp(2.0 * x_cost, &e2);  // sum_p |q_p|^2 <= 2 cost (observations + point priors) < 2^e2
      a.kq = (e2 + 1) >> 1;
    }
    launch_schur_scale(s, NC, h->ug(), h->d_scale_c, h->d_kx);
    HIP_OK(hipMemsetAsync(h->d_rfx, 0, sizeof(unsigned long long) * 6 * (size_t)NC, s));
    launch_schur_y(s, v, h->d_points, h->d_camtab, h->d_L, h->d_q, h->d_scale_c, a, h->d_yrec, h->d_rfx);
    launch_schur_tiles(s, h->d_yrec, a, NC);
    launch_schur_sum_tiles(s, a, h->d_sblk);
    CHECK_RC(h->allreduce(h->d_sblk, (size_t)a.nelem, ncclSum));
    CHECK_RC(h->allreduce_u64(reinterpret_cast<uint64_t*>(h->d_rfx), (size_t)6 * NC));
    HIP_OK(hipMemsetAsync(cs.S, 0, sizeof(double) * (size_t)(cs.n + 1) * cs.ld, s));
    launch_schur_unpack(s, NC, h->d_sblk, h->d_rfx, h->d_kx, a.kq, cs.S, cs.ld, h->ybc());
    launch_s_add_u(s, NC, h->ug(), h->ncross, h->d_cross_cam, h->Ux(), h->d_scale_c, sc, h->ybc(), cs.S, cs.ld);
    return 0;
  }
  // the camera-major pass writes the [NE][18] records the S blocks gather (no plane-to-record
  // copy); the slot planes as before
  launch_entry_y(s, v, h->d_points, h->d_camtab, h->d_scale_c, h->d_L, YBufs{h->d_Y, h->d_Yp, false}, with_pm,
                 h->lz.d_Yrec);
  // one rank: the S blocks straight into the dense S (nothing to all-reduce), no zero
  // fill of the whole matrix and no scatter; several: packed, all-reduced, unpacked
  const bool direct = h->world == 1;
  launch_s_blocks(s, h->nblk, h->d_blk_pair_beg, h->d_pairs, nullptr, h->NE, h->packed(), h->lz.d_Yrec,
                  direct ? cs.S : nullptr, cs.ld, h->d_blk_cam, h->nzero, h->d_blk_zero);
  launch_cam_rhs_partial(s, v, h->nchunk, h->d_chunk_beg, h->lz.d_Yrec, h->d_q, h->d_partial, true);
  launch_seg_final(s, NC, 6, h->d_seg_chunk, h->d_partial, h->ybc(), h->max_seg_chunks);
  if (direct) {
    launch_s_add_u(s, NC, h->ug(), h->ncross, h->d_cross_cam, h->Ux(), h->d_scale_c, sc, h->ybc(), cs.S, cs.ld);
  } else {
    CHECK_RC(h->allreduce(h->d_spack, h->spack_count(), ncclSum));
    launch_s_unpack(s, NC, h->nblk, h->d_blk_cam, h->packed(), h->ug(), h->ncross, h->d_cross_cam, h->Ux(),
                    h->d_scale_c, sc, h->ybc(), cs.S, cs.ld);
  }
  return 0;
}

static int solve_impl(dab_handle* h, const dab_options* opt_in, dab_summary* sum) {
  clear_error();
  if (!h || !h->have_problem) return set_error(DAB_E_STATE, "no problem set");
  if (!sum) return set_error(DAB_E_INVALID, "null summary");
  dab_options opt;
  if (opt_in) opt = *opt_in;
  else dab_options_init(&opt);
  // the fp32 matrix-free product (proj_jac32) never forms a residual, and fp32 Y records from
  // an fp32-weighted row are numerics work of their own: refused, never a silent fp64 fall-back
  if (opt.pcg_fp32 != 0 && h->view.loss != DAB_LOSS_TRIVIAL)
    return set_error(DAB_E_UNSUPPORTED, "pcg_fp32 with a robust loss is not supported (set pcg_fp32 = 0 or DAB_LOSS_TRIVIAL)");
  if (opt.linear_solver_type != DAB_LINEAR_SOLVER_EXPLICIT_SCHUR &&
      opt.linear_solver_type != DAB_LINEAR_SOLVER_IMPLICIT_SCHUR_PCG &&
      opt.linear_solver_type != DAB_LINEAR_SOLVER_AUTO)
    return set_error(DAB_E_INVALID, "unknown linear_solver_type");
  HIP_OK(hipSetDevice(h->device));
  // constant points: this rank's set, and whether any rank has a free point left
  CHECK_RC(pt_const_sync(h));
  CHECK_RC(ext_sub_sync(h));  // the effective constant scalars of the free extrinsics (none: no masked kernel)
  CHECK_RC(prior_sync(h));  // the effective extrinsic priors (none: no prior kernel is launched)
  CHECK_RC(pt_prior_sync(h));  // this rank's effective point priors, after pt_const_sync (likewise)
  // whether any rank has a free point left, and whether any has an effective point prior
  int pstate = 2;
  CHECK_RC(call_state(h, &pstate));
  const bool no_free_points = pstate == 1;
  if (opt.linear_solver_type == DAB_LINEAR_SOLVER_AUTO)  // the same choice on every rank (NC is the union's)
    opt.linear_solver_type = h->world <= 1 || h->NC == 0 || mf_schur_fits(h->NC, h->E, h->NI) ||
                                     (no_free_points && h->knobs.points_direct != 0)  // S = U + D^2: nothing to reduce
                                 ? DAB_LINEAR_SOLVER_EXPLICIT_SCHUR
                                 : DAB_LINEAR_SOLVER_IMPLICIT_SCHUR_PCG;
  const bool use_pcg = opt.linear_solver_type == DAB_LINEAR_SOLVER_IMPLICIT_SCHUR_PCG;
  const bool timing = PhaseTimer::on();
  // free intrinsics: the refusals come first, so a refused solve leaves the handle as it was
  CamSystem cs;
  CHECK_RC(cam_system_free_set(
      h, use_pcg ? "free intrinsics need the exact step (DAB_LINEAR_SOLVER_EXPLICIT_SCHUR)" : nullptr, &cs));
  CHECK_RC(zprior_sync(h, cs.nfi));  // the effective intrinsic priors of that free set (none: no prior kernel)
  // no free point on any rank: no Schur complement, the camera system is U + D^2 (block diagonal
  // without cross blocks). Not with free intrinsics, nor for an explicitly requested PCG
  const bool direct = no_free_points && !use_pcg && cs.nfi == 0 && h->NC > 0 && h->knobs.points_direct != 0;
  const bool direct_dense = direct && h->ncross > 0;
  // (or every scalar of every free extrinsic is constant, and no intrinsic is free)
  const bool no_free_params = no_free_points && (h->NC == 0 || (h->n_ext_sub == 6 * h->NC && cs.nfi == 0));
  const double tp0 = now_s();
  if (direct_dense) {
    // the dense buffer as build_schur_tables sizes it (kept when the tables are built later)
    const int nd = 6 * h->NC;
    h->lds = ((nd + 1 + 7) / 8) * 8;
    if (h->lds % 512 == 0) h->lds += 8;
    CHECK_RC(h->sticky(h->st_S, &h->d_S, (size_t)(nd + 1) * h->lds));
    if (!h->lz.d_zero6) {
      CHECK_RC(h->dev.alloc(&h->lz.d_zero6, (size_t)nd));
      HIP_OK(hipMemsetAsync(h->lz.d_zero6, 0, sizeof(double) * (size_t)nd, h->stream));
    }
  }
  if (!direct && !no_free_params) CHECK_RC(use_pcg ? build_pcg_buffers(h) : build_schur_tables(h));
  const double tp1 = now_s();
  CHECK_RC(cam_system_buffers(h, direct ? direct_dense : !use_pcg && !no_free_params, &cs));
  const int nfi = cs.nfi, n2 = cs.n2;
  double* const yc_ = cs.yc;
  if (timing)
    std::fprintf(stderr, "solve prep: %s %.2f ms, Cholesky graph %.2f ms\n", use_pcg ? "pcg buffers" : "schur tables",
                 1e3 * (tp1 - tp0), 1e3 * (now_s() - tp1));
  // Y records of each step: fp64 (both layouts), or fp32 for the mixed-precision PCG
  // (Jacobians, residuals, V/U/g, the CG vectors and scalars stay fp64)
  // (the matrix-free PCG of small camera sets stores no Y and is all fp64)
  const bool y32 = use_pcg && opt.pcg_fp32 != 0 && !h->mf;
  // matrix-free mixed precision: fp32 products, fp64 sums, recurrences and true residuals
  h->mf32 = use_pcg && opt.pcg_fp32 != 0 && h->mf;
  if (y32 && !h->lz.d_Y32c) {
    CHECK_RC(h->dev.alloc(&h->lz.d_Y32c, (size_t)kYRec * std::max(1, h->NE)));
    CHECK_RC(h->dev.alloc(&h->lz.d_Y32p, (size_t)kYRec * std::max(1, h->NS) * (h->any_compose ? 2 : 1)));
  }
  const YBufs yb = y32 ? YBufs{h->lz.d_Y32c, h->lz.d_Y32p, true} : YBufs{h->d_Y, h->d_Yp, false};
  hipStream_t s = h->stream;
  const DevView& v = h->view;
  const int NP = h->NP, NC = h->NC, n = 6 * NC;
  const double t_start = now_s();
  std::memset(sum->message, 0, sizeof(sum->message));
  sum->iterations_written = 0;
  sum->num_successful_steps = sum->num_unsuccessful_steps = 0;
  sum->num_iterations = 0;
  sum->num_residuals = 2 * h->N + 6 * h->n_prior + 3 * h->n_pt_prior + 6 * h->n_zprior;  // this rank's, as 2 N is
  sum->num_parameters = 3 * (NP - h->n_pt_const) + 6 * NC - h->n_ext_sub + cs.nz_scal;
  sum->num_free_points = NP - h->n_pt_const;
  sum->num_free_ext = NC;
  sum->jacobian_evaluation_time_in_seconds = 0;
  sum->residual_evaluation_time_in_seconds = 0;
  sum->linear_solver_time_in_seconds = 0;
  sum->termination_type = DAB_FAILURE;
  sum->linear_solver_type_used = opt.linear_solver_type;
  sum->schur_assembly = use_pcg ? (h->mf ? (h->mf32 ? DAB_PCG_MATRIX_FREE_FP32 : DAB_PCG_MATRIX_FREE) : DAB_PCG_STORED_Y)
                                : (direct ? DAB_SCHUR_DIRECT : h->schur_tiles ? DAB_SCHUR_TILES : DAB_SCHUR_PAIRS);
  const bool verbose = opt.minimizer_progress_to_stdout && h->rank == 0;

  // ---- iteration 0 ----
  // a solve starts with a clean sticky error word (a timed-out wait of an earlier call was
  // reported by that call)
  HIP_OK(hipMemsetAsync(h->d_scal + S_XERR, 0, sizeof(double), s));
  // without free points no back substitution runs: delta_p is zero for the whole solve
  if (direct && NP > 0) HIP_OK(hipMemsetAsync(h->d_dp, 0, sizeof(double) * 3 * (size_t)NP, s));
  double t0 = now_s();
  CHECK_RC(eval_jacobian_and_blocks(h, true));
  // intrinsic sums and norms at x (k_intr_eval after every evaluation pass); hz = their host copy:
  // [0..4] of the candidate, [8..12] at x, as launch_cam_norms orders them
  double hz[16] = {0};
  auto intr_at_x = [&]() -> int {
    if (nfi <= 0) return 0;
    CHECK_RC(intr_eval(h));
    // intrinsic priors: A^T A | A^T r into zg, after the sum over the ranks and before the norms at
    // x, the Jacobi scale and the border rows read it
    zprior_blocks(h);
    launch_intr_candidate(s, h->NI, h->lz.d_intr_meta, h->d_intr, h->lz.d_sz, nullptr, h->lz.d_zg, nullptr, nullptr,
                          h->lz.d_znorm + 8);
    return 0;
  };
  auto read_znorm = [&]() -> int {
    if (nfi <= 0) return 0;
    HIP_OK(hipMemcpyAsync(hz, h->lz.d_znorm, sizeof(hz), hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    return 0;
  };
  CHECK_RC(intr_at_x());
  CHECK_RC(read_znorm());
  CHECK_RC(read_scalars(h));
  if (timing) std::fprintf(stderr, "solve iteration 0: %.2f ms\n", 1e3 * (now_s() - t0));
  launch_jacobi_scale(h, nfi, opt.jacobi_scaling);
  sum->jacobian_evaluation_time_in_seconds += now_s() - t0;
  // x_rhs: the observations' cost and the point priors' (all ranks): both enter q_p, so together
  // they bound the tile assembly's fixed-point rhs. The extrinsic priors' part never enters q_p
  // and stays out of that bound (it could only loosen it), and so does the intrinsic priors'.
  auto cost_at_x = [&](double* rhs) {
    const double obs = 0.5 * h->h_scal[S_COST];
    *rhs = h->pt_prior_any ? obs + pt_prior_cost(h) : obs;
    double c = h->n_prior > 0 ? obs + prior_cost(h) : obs;
    if (h->pt_prior_any) c += pt_prior_cost(h);
    return h->n_zprior > 0 ? c + zprior_cost(h) : c;
  };
  double x_rhs;
  double x_cost = cost_at_x(&x_rhs);
  bool eval_ok = h->h_scal[S_COST_BAD] == 0.0 && std::isfinite(prior_cost(h)) && std::isfinite(pt_prior_cost(h)) &&
                 std::isfinite(zprior_cost(h));
  double gmax = std::max(h->h_scal[S_GMAX_P], h->h_scal[S_CAM0 + 2]);
  double x_norm = std::sqrt(h->h_scal[S_XNORM_P] + h->h_scal[S_CAM0 + 4]);
  if (nfi > 0) {
    gmax = std::max(gmax, hz[8 + 2]);
    x_norm = std::sqrt(h->h_scal[S_XNORM_P] + h->h_scal[S_CAM0 + 4] + hz[8 + 4]);
  }
  sum->initial_cost = x_cost;
  double final_cost = x_cost;
  if (!eval_ok) {
    std::snprintf(sum->message, sizeof(sum->message), "Residual and Jacobian evaluation failed.");
    sum->final_cost = x_cost;
    sum->total_time_in_seconds = now_s() - t_start;
    return 0;
  }
  if (no_free_params) {
    // Ceres' reduced program is empty: nothing to minimise, the parameters stay as they are
    sum->termination_type = DAB_CONVERGENCE;
    sum->final_cost = x_cost;
    std::snprintf(sum->message, sizeof(sum->message),
                  "Function tolerance reached. No non-constant parameter blocks found.");
    sum->total_time_in_seconds = now_s() - t_start;
    return 0;
  }

  int iteration = 0;
  double radius = opt.initial_trust_region_radius, decrease_factor = 2.0;
  int num_invalid = 0;
  int term = -1;
  dab_iteration it{};
  it.iteration = 0;
  it.step_is_successful = 1;
  it.step_is_valid = 1;
  it.cost = x_cost;
  it.gradient_max_norm = gmax;
  double iter_start = t_start;
  if (verbose) print_header();

  for (;;) {
    // FinalizeIterationAndCheckIfMinimizerCanContinue
    if (it.step_is_successful) sum->num_successful_steps++;
    else sum->num_unsuccessful_steps++;
    it.trust_region_radius = radius;
    it.iteration_time_in_seconds = now_s() - iter_start;
    if (it.cost < final_cost) final_cost = it.cost;
    if (sum->iterations && sum->iterations_written < sum->iterations_capacity)
      sum->iterations[sum->iterations_written++] = it;
    if (verbose) print_iter(it, now_s() - t_start);
    sum->num_iterations = iteration;
    const double elapsed = elapsed_collective(h, now_s() - t_start);
    if (elapsed < 0) return set_error(DAB_E_DEVICE, "solver-time all-reduce failed");
    if (elapsed >= opt.max_solver_time_in_seconds) {
      term = DAB_NO_CONVERGENCE;
      std::snprintf(sum->message, sizeof(sum->message), "Maximum solver time reached.");
      break;
    }
    if (iteration >= opt.max_num_iterations) {
      term = DAB_NO_CONVERGENCE;
      std::snprintf(sum->message, sizeof(sum->message),
                    "Maximum number of iterations reached. Number of iterations: %d.", iteration);
      break;
    }
    if (it.step_is_successful && gmax <= opt.gradient_tolerance) {
      term = DAB_CONVERGENCE;
      std::snprintf(sum->message, sizeof(sum->message), "Gradient tolerance reached. Gradient max norm: %e <= %e",
                    gmax, opt.gradient_tolerance);
      break;
    }
    if (radius <= opt.min_trust_region_radius) {
      term = DAB_CONVERGENCE;
      std::snprintf(sum->message, sizeof(sum->message), "Minimum trust region radius reached.");
      break;
    }

    iter_start = now_s();
    iteration++;
    const double prev_gmax = gmax;
    it = dab_iteration{};
    it.iteration = iteration;
    it.linear_solver_iterations = 1;

    // ---- ComputeTrustRegionStep (DENSE_SCHUR) ----
    const double tls = now_s();
    StepScalars sc{radius, opt.min_lm_diagonal, opt.max_lm_diagonal};
    HIP_OK(hipMemsetAsync(h->d_flags, 0, sizeof(int) * 4, s));
    if (!direct) launch_point_factor_m(s, v, h->d_V, h->d_g, h->d_scale_p, sc, h->d_L, h->d_q, h->d_flags, h->d_ptc);
    bool pcg_fail = false;
    if (direct && !direct_dense) {
      launch_cam_block_solve_x(s, NC, h->ug(), h->d_scale_c, sc, yc_, h->d_flags + 1, h->d_exs);
    } else if (direct) {
      HIP_OK(hipMemsetAsync(cs.S, 0, sizeof(double) * (size_t)(n + 1) * cs.ld, s));
      launch_s_add_u(s, NC, h->ug(), h->ncross, h->d_cross_cam, h->Ux(), h->d_scale_c, sc, h->lz.d_zero6, cs.S, cs.ld);
      launch_ext_unit_diag(s, NC, h->d_exs, cs.S, cs.ld);
      if (chol_factor_solve(h->chol, s, n, cs.S, cs.ld, yc_, h->d_flags + 1) != 0)
        return set_error(DAB_E_DEVICE, "dense Cholesky launch failed");
    } else if (NC > 0 && use_pcg) {
      if (!h->mf) launch_entry_y(s, v, h->d_points, h->d_camtab, h->d_scale_c, h->d_L, yb, true);
      int cg_iters = 0, cg_status = 0;
      CHECK_RC(pcg_solve(h, opt, sc, yb, &cg_iters, &cg_status));
      it.linear_solver_iterations = cg_iters;
      pcg_fail = cg_status == kPcgFailure;
    } else if (NC > 0) {
      CHECK_RC(cam_system_assemble(h, cs, sc, x_rhs, true));
      CHECK_RC(intr_border_rows(h, nfi, sc, cs.S, cs.ld));
      launch_ext_unit_diag(s, NC, h->d_exs, cs.S, cs.ld);  // constant scalars: unit rows for the factor
      if (chol_factor_solve(h->chol, s, n2, cs.S, cs.ld, yc_, h->d_flags + 1) != 0)
        return set_error(DAB_E_DEVICE, "dense Cholesky launch failed");
    }
    // (the direct step has no back substitution: delta_p stays the zeros written before iteration 0)
    if (!direct && ((use_pcg && h->mf) || (!use_pcg && h->schur_tiles)))
      launch_mf_backsub(s, v, h->d_points, h->d_camtab, h->d_scale_c, h->d_L, h->d_q, yc_, h->d_dp, h->mf_grid_n);
    else if (!direct)
      launch_backsub(s, v, h->d_L, h->d_q, yb, NC > 0 ? yc_ : nullptr, h->d_dp);
    // the y_z term of the point step, whichever back substitution ran
    if (nfi > 0)
      launch_intr_backsub(s, v, h->d_points, h->d_camtab, h->d_L, h->lz.d_sz, yc_ + n, h->lz.d_intr_meta, h->d_dp);
    // candidate x + delta and the model / candidate cost in one observation pass
    launch_axpy_points_m(s, NP, h->d_points, h->d_dp, h->d_points_c, h->d_gpart, h->red_grid, h->d_ptc);
    launch_final_sum(s, h->red_grid, 2, h->d_gpart, h->d_scal + S_STEP_P);
    launch_cam_candidate_x(s, h->E, h->d_ext_col, h->d_ext, NC > 0 ? yc_ : nullptr, h->d_scale_c, h->d_ext_c,
                           h->d_dc, h->d_exs);
    launch_cam_norms_x(s, h->E, h->d_ext_col, h->d_ext, h->d_ext_c, nullptr, h->d_scal + S_CAM0, h->d_exs);
    launch_cam_tables(s, h->E, h->d_ext_c, h->d_camtab_c);
    const double tre = now_s();
    if (nfi > 0) {
      // candidate intrinsics, delta_z and their norms; the candidate pass with the z term
      launch_intr_candidate(s, h->NI, h->lz.d_intr_meta, h->d_intr, h->lz.d_sz, yc_ + n, nullptr, h->lz.d_intr_c, h->lz.d_dz,
                            h->lz.d_znorm);
      launch_candidate_z(s, v, h->d_points, h->d_camtab, h->d_dp, h->d_dc, h->d_camtab_c, h->lz.d_intr_meta, h->lz.d_dz,
                         h->lz.d_intr_c, h->d_gpart, h->red_grid);
    } else {
      launch_candidate(s, v, h->d_points, h->d_camtab, h->d_dp, h->d_dc, h->d_camtab_c, h->d_gpart, h->red_grid);
    }
    launch_final_sum(s, h->red_grid, 3, h->d_gpart, h->d_scal + S_MODEL);
    // the point priors' part of the model cost change and of the candidate's cost: this rank's,
    // after the final sum that writes those slots (same stream) and before the sum over the ranks
    launch_pt_prior_candidate(s, h->n_pt_prior, NP, h->lz.d_ptp_idx, h->lz.d_ptp_rec, h->d_points, h->d_points_c,
                              h->d_dp, h->lz.d_ptp_part, h->lz.d_ptp_cnt, h->d_scal + S_MODEL);
    CHECK_RC(h->allreduce(h->d_scal + S_MODEL, 5, ncclSum));
    // the priors' part of the model cost change and of the candidate's cost, once, after the sum
    launch_prior_candidate(s, h->n_prior, h->lz.d_prior_idx, h->lz.d_prior_rec, h->d_ext, h->d_ext_c, h->d_dc,
                           h->lz.d_prior_part, h->lz.d_prior_cnt, h->d_scal + S_MODEL);
    launch_zprior_candidate(s, h->n_zprior, h->lz.d_zp_idx, h->lz.d_zp_rec, h->d_intr, h->lz.d_intr_c, h->lz.d_dz,
                            h->d_scal + S_MODEL);
    CHECK_RC(h->allreduce_max_i32(h->d_flags, 4));
    CHECK_RC(read_znorm());
    CHECK_RC(read_scalars(h));
    // bit 2 of the Cholesky flag: a bounded wait inside the factorisation gave up (a
    // scheduling / residency fault, not a property of the matrix): an error, not a
    // rejected step (bit 1 = not positive definite)
    if (!use_pcg && NC > 0 && (h->h_flags[1] & 2))
      return set_error(DAB_E_DEVICE, "dense Cholesky: a bounded wait between work-groups timed out");
    const double tdone = now_s();
    sum->linear_solver_time_in_seconds += tre - tls;
    sum->residual_evaluation_time_in_seconds += tdone - tre;

    const bool solve_fail = pcg_fail || h->h_flags[0] != 0 || h->h_flags[1] != 0 || h->h_flags[2] != 0 ||
                            h->h_flags[3] != 0;
    const double model_cost_change = h->h_scal[S_MODEL];
    it.step_is_valid = !solve_fail && std::isfinite(model_cost_change) && model_cost_change > 0.0;
    if (!it.step_is_valid) {
      num_invalid++;
      if (num_invalid >= opt.max_num_consecutive_invalid_steps) {
        term = DAB_FAILURE;
        std::snprintf(sum->message, sizeof(sum->message),
                      "Number of consecutive invalid steps more than Solver::Options::max_num_consecutive_invalid_steps: %d",
                      opt.max_num_consecutive_invalid_steps);
        break;
      }
      radius = radius / decrease_factor;
      decrease_factor *= 2.0;
      it.cost = x_cost;
      it.gradient_max_norm = prev_gmax;
      it.step_is_successful = 0;
      continue;
    }
    num_invalid = 0;
    const double candidate_cost = h->h_scal[S_CAND_BAD] != 0.0 ? 1.7976931348623157e308 : 0.5 * h->h_scal[S_CAND];
    // ParameterToleranceReached
    it.step_norm = nfi > 0 ? std::sqrt(h->h_scal[S_STEP_P] + h->h_scal[S_CAM0 + 0] + hz[0])
                           : std::sqrt(h->h_scal[S_STEP_P] + h->h_scal[S_CAM0 + 0]);
    if (it.step_norm <= opt.parameter_tolerance * (x_norm + opt.parameter_tolerance)) {
      term = DAB_CONVERGENCE;
      std::snprintf(sum->message, sizeof(sum->message), "Parameter tolerance reached. Relative step_norm: %e <= %e.",
                    it.step_norm / (x_norm + opt.parameter_tolerance), opt.parameter_tolerance);
      break;
    }
    // FunctionToleranceReached
    it.cost_change = x_cost - candidate_cost;
    if (std::fabs(it.cost_change) <= opt.function_tolerance * x_cost) {
      term = DAB_CONVERGENCE;
      std::snprintf(sum->message, sizeof(sum->message), "Function tolerance reached. |cost_change|/cost: %e <= %e",
                    std::fabs(it.cost_change) / x_cost, opt.function_tolerance);
      break;
    }
    it.relative_decrease = (x_cost - candidate_cost) / model_cost_change;
    if (it.relative_decrease > opt.min_relative_decrease) {
      // HandleSuccessfulStep: x <- candidate, re-evaluate J at the new point
      const double xc_norm = nfi > 0 ? std::sqrt(h->h_scal[S_XCNORM_P] + h->h_scal[S_CAM0 + 1] + hz[1])
                                     : std::sqrt(h->h_scal[S_XCNORM_P] + h->h_scal[S_CAM0 + 1]);
      std::swap(h->d_points, h->d_points_c);
      std::swap(h->d_ext, h->d_ext_c);
      std::swap(h->d_camtab, h->d_camtab_c);  // the candidate pass built the tables of x + delta
      if (nfi > 0) {  // every kernel reads the intrinsics through the view
        std::swap(h->d_intr, h->lz.d_intr_c);
        h->view.intr = h->d_intr;
      }
      x_norm = xc_norm;
      const double tj = now_s();
      CHECK_RC(eval_jacobian_and_blocks(h, true, true));
      CHECK_RC(intr_at_x());
      CHECK_RC(read_znorm());
      CHECK_RC(read_scalars(h));
      sum->jacobian_evaluation_time_in_seconds += now_s() - tj;
      if (h->h_scal[S_COST_BAD] != 0.0 || !std::isfinite(prior_cost(h)) || !std::isfinite(pt_prior_cost(h)) ||
          !std::isfinite(zprior_cost(h))) {
        term = DAB_FAILURE;
        std::snprintf(sum->message, sizeof(sum->message), "Residual and Jacobian evaluation failed.");
        break;
      }
      x_cost = cost_at_x(&x_rhs);
      gmax = std::max(h->h_scal[S_GMAX_P], h->h_scal[S_CAM0 + 2]);
      if (nfi > 0) gmax = std::max(gmax, hz[8 + 2]);
      it.step_is_successful = 1;
      it.cost = x_cost;
      it.gradient_max_norm = gmax;
      radius = radius / std::max(1.0 / 3.0, 1.0 - std::pow(2.0 * it.relative_decrease - 1.0, 3));
      radius = std::min(opt.max_trust_region_radius, radius);
      decrease_factor = 2.0;
    } else {
      it.step_is_successful = 0;
      it.cost = candidate_cost;
      it.gradient_max_norm = prev_gmax;
      radius = radius / decrease_factor;
      decrease_factor *= 2.0;
    }
  }

  sum->termination_type = term;
  sum->final_cost = final_cost;
  // the accepted iterate is always the lowest-cost one (steps are monotone), so the
  // device-resident x is Ceres' parameters_; write it back (sfm.cc:47-48 semantics)
  HIP_OK(hipStreamSynchronize(s));
  CHECK_RC(p2p_check(h->p2p_main));  // fail closed: the caller's arrays stay untouched
  CHECK_RC(p2p_check(h->p2p_comm));
  CHECK_RC(dab_get_parameters(h, h->prob.points, h->prob.ext));
  sum->total_time_in_seconds = now_s() - t_start;
  return 0;
}
