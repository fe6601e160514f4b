// dab_api_eval.hip — the entry points beside the solve: residual / Jacobian evaluation and
// the point filter (filterPoint3d, parity), the dense SPD solve, the benchmark hooks.
#include "dab_handle.h"

using namespace dab;

// ------------------------------------------------------------------------------------
// evaluation entry points (filterPoint3d residual pass, parity)
// ------------------------------------------------------------------------------------
extern "C" int dab_eval_residuals(dab_handle* h, double* residuals, double* cost) {
  clear_error();
  if (!h || !h->have_problem) return set_error(DAB_E_STATE, "no problem set");
  HIP_OK(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  launch_cam_tables(s, h->E, h->d_ext, h->d_camtab);
  launch_residual(s, h->view, h->d_points, h->d_camtab, h->d_r, h->d_gpart, h->red_grid);
  launch_final_sum(s, h->red_grid, 2, h->d_gpart, h->d_scal + S_COST);
  h->cost_fx_pending = false;
  CHECK_RC(read_scalars(h));
  if (cost) *cost = 0.5 * h->h_scal[S_COST];
  if (residuals) {
    std::vector<double> r((size_t)2 * h->NS);
    HIP_OK(hipMemcpyAsync(r.data(), h->d_r, r.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    for (int s2 = 0; s2 < h->NS; ++s2) {
      const int o = h->perm[s2];
      if (o < 0) continue;
      residuals[2 * (size_t)o] = r[2 * (size_t)s2];
      residuals[2 * (size_t)o + 1] = r[2 * (size_t)s2 + 1];
    }
  }
  return 0;
}

extern "C" int dab_eval_jacobians(dab_handle* h, double* residuals, double* jacobians) {
  clear_error();
  if (!h || !h->have_problem) return set_error(DAB_E_STATE, "no problem set");
  HIP_OK(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  if (!h->lz.d_Jfull) CHECK_RC(h->dev.alloc(&h->lz.d_Jfull, (size_t)30 * h->NS));
  launch_cam_tables(s, h->E, h->d_ext, h->d_camtab);
  launch_jacobian_full(s, h->view, h->d_points, h->d_camtab, h->d_r, h->lz.d_Jfull);
  std::vector<double> r((size_t)2 * h->NS), J((size_t)30 * h->NS);
  HIP_OK(hipMemcpyAsync(r.data(), h->d_r, r.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(J.data(), h->lz.d_Jfull, J.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  for (int s2 = 0; s2 < h->NS; ++s2) {
    const int o = h->perm[s2];
    if (o < 0) continue;
    if (residuals) {
      residuals[2 * (size_t)o] = r[2 * (size_t)s2];
      residuals[2 * (size_t)o + 1] = r[2 * (size_t)s2 + 1];
    }
    if (jacobians) {
      double* out = jacobians + (size_t)o * 30;
      const bool comp = h->prob.obs_ext1[o] >= 0;
      for (int col = 0; col < 15; ++col)
        for (int row = 0; row < 2; ++row) {
          double val = 0.0;
          if (col < 9 || comp) val = J[(size_t)(2 * col + row) * h->NS + s2];
          out[row * 15 + col] = val;
        }
    }
  }
  return 0;
}

extern "C" int dab_filter(dab_handle* h, double error_boundary, const double center[3], double radius,
                          uint8_t* obs_keep, uint8_t* point_keep, int32_t* n_obs_kept, int32_t* n_points_kept) {
  clear_error();
  if (!h || !h->have_problem) return set_error(DAB_E_STATE, "no problem set");
  if (!center) return set_error(DAB_E_INVALID, "null hemisphere center");
  HIP_OK(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  Dev tmp{"entry-point temporaries"};
  unsigned char *d_slot = nullptr, *d_pt = nullptr;
  CHECK_RC(tmp.alloc(&d_slot, (size_t)std::max(1, h->NS)));
  CHECK_RC(tmp.alloc(&d_pt, (size_t)std::max(1, h->NP)));
  launch_cam_tables(s, h->E, h->d_ext, h->d_camtab);
  launch_filter(s, h->view, h->d_points, h->d_camtab, error_boundary, center, radius, d_slot, d_pt);
  std::vector<unsigned char> slot((size_t)h->NS), pt((size_t)h->NP);
  if (h->NS > 0) HIP_OK(hipMemcpyAsync(slot.data(), d_slot, slot.size(), hipMemcpyDeviceToHost, s));
  if (h->NP > 0) HIP_OK(hipMemcpyAsync(pt.data(), d_pt, pt.size(), hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  CHECK_RC(guard_fail(h, "dab_filter", &tmp));
  int32_t no = 0, np = 0;
  if (obs_keep) std::memset(obs_keep, 0, (size_t)h->N);
  for (int s2 = 0; s2 < h->NS; ++s2) {
    const int o = h->perm[s2];
    if (o < 0) continue;
    if (obs_keep) obs_keep[o] = slot[s2];
    no += slot[s2];
  }
  if (point_keep) std::memset(point_keep, 0, (size_t)h->prob.num_points);
  for (int i = 0; i < h->NP; ++i) {
    if (point_keep) point_keep[h->pt_of[i]] = pt[i];
    np += pt[i];
  }
  if (n_obs_kept) *n_obs_kept = no;
  if (n_points_kept) *n_points_kept = np;
  return 0;
}

extern "C" int dab_dense_spd_solve(dab_handle* h, int n, const double* A, const double* b, double* x,
                                   double* factor_ms) {
  clear_error();
  if (!h) return set_error(DAB_E_INVALID, "null handle");
  if (n < 0 || (n > 0 && (!A || !b || !x))) return set_error(DAB_E_INVALID, "bad dense solve arguments");
  if (n == 0) return 0;
  HIP_OK(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  int lds = ((n + 1 + 7) / 8) * 8;
  if (lds % 512 == 0) lds += 8;
  Dev tmp{"entry-point temporaries"};
  double *dA = nullptr, *dy = nullptr;
  int* dflag = nullptr;
  CHECK_RC(tmp.alloc(&dA, (size_t)(n + 1) * lds));
  CHECK_RC(tmp.alloc(&dy, (size_t)n));
  CHECK_RC(tmp.alloc(&dflag, 1));
  HIP_OK(hipMemsetAsync(dA, 0, sizeof(double) * (size_t)(n + 1) * lds, s));
  HIP_OK(hipMemsetAsync(dflag, 0, sizeof(int), s));
  HIP_OK(hipMemcpy2DAsync(dA, lds * sizeof(double), A, n * sizeof(double), n * sizeof(double), n,
                          hipMemcpyHostToDevice, s));
  HIP_OK(hipMemcpyAsync(dA + (size_t)n * lds, b, n * sizeof(double), hipMemcpyHostToDevice, s));
  HIP_OK(hipEventRecord(h->ev0, s));
  if (chol_factor_solve(h->chol, s, n, dA, lds, dy, dflag) != 0)
    return set_error(DAB_E_DEVICE, "dense factorisation launch failed");
  HIP_OK(hipEventRecord(h->ev1, s));
  int flag = 0;
  HIP_OK(hipMemcpyAsync(x, dy, n * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(&flag, dflag, sizeof(int), hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  CHECK_RC(guard_fail(h, "dab_dense_spd_solve", &tmp));
  float ms = 0.f;
  HIP_OK(hipEventElapsedTime(&ms, h->ev0, h->ev1));
  if (factor_ms) *factor_ms = ms;
  return flag ? 1 : 0;
}

// ------------------------------------------------------------------------------------
// benchmark hooks
// ------------------------------------------------------------------------------------
// accumulate the timings of the recorded bench steps (waits for the last one)
static int collect_bench_events(dab_handle* h) {
  if (h->bench_pending == 0) return 0;
  HIP_OK(hipEventSynchronize(h->bench_ev[h->bench_pending - 1][3]));
  for (int i = 0; i < h->bench_pending; ++i) {
    const auto& ev = h->bench_ev[i];
    float a = 0.f, b = 0.f, c = 0.f;
    HIP_OK(hipEventElapsedTime(&a, ev[0], ev[1]));  // camera side (+ all-reduce issue)
    HIP_OK(hipEventElapsedTime(&b, ev[1], ev[2]));  // point kernel
    HIP_OK(hipEventElapsedTime(&c, ev[2], ev[3]));  // cost sum + all-reduce join
    h->bench_jac_ms += b;
    h->bench_asm_ms += a + c;
    h->bench_count++;
    if (h->bench_pair_rec[i]) {
      float d = 0.f;
      HIP_OK(hipEventElapsedTime(&d, ev[4], ev[5]));  // pair-major camera kernel
      h->bench_pair_ms += d;
      h->bench_pair_count++;
    }
  }
  h->bench_pending = 0;
  return 0;
}

extern "C" int dab_bench_eval_pass(dab_handle* h, int with_assembly, int count) {
  clear_error();
  if (!h || !h->have_problem) return set_error(DAB_E_STATE, "no problem set");
  if (count < 0) return set_error(DAB_E_INVALID, "negative pass count");
  HIP_OK(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  // Timing events bracket every 8th pass (Knobs::bench_sample) of the batch (the first one always):
  // even fence-free, four event records add ~10 us to a ~40 us pass, so timing every pass
  // would distort the throughput it measures. DAB_BENCH_SAMPLE overrides (0 = no events).
  const int sample = h->knobs.bench_sample;
  // a non-empty free set: the intrinsic sums of each pass too (dab_get_intrinsic_blocks)
  int bench_nfi = 0;
  if (intr_mask_any(h)) CHECK_RC(intr_free_set(h, true, &bench_nfi));
  if (bench_nfi > kIntrFreeMax) return set_error(DAB_E_UNSUPPORTED, "more than 16 free intrinsics");
  auto intr_pass = [&]() -> int {
    if (bench_nfi <= 0) return 0;
    launch_cam_tables(s, h->E, h->d_ext, h->d_camtab);
    return intr_eval(h);
  };
  for (int step = 0; step < count; ++step) {
    // every bench pass is an evaluation at a NEW linearization point, as in the LM loop
    // after an accepted step (sfm.cc:66-73, Ceres re-linearises each iteration): the pass
    // derives nothing from the points that it could keep between passes (no camera-major
    // point copy; the tables are built inside the launch)
    if (sample <= 0 || step % sample != 0) {
      CHECK_RC(eval_pass(h, false));
      CHECK_RC(h->allreduce_cost());
      CHECK_RC(intr_pass());
      continue;
    }
    // per-step events from a pool: nothing here waits for the device, so back-to-back
    // steps queue like the solver's own passes; dab_bench_kernel_ms reads them afterwards
    if (h->bench_pending >= (int)h->bench_ev.size()) {
      if (h->bench_pending >= 4096) CHECK_RC(collect_bench_events(h));
      while ((int)h->bench_ev.size() <= h->bench_pending) {
        std::array<hipEvent_t, 6> e{};
        // timing-only events: no system-scope fence (it costs several us per record)
        for (auto& x : e) HIP_OK(hipEventCreateWithFlags(&x, hipEventDisableSystemFence));
        h->bench_ev.push_back(e);
      }
    }
    h->bench_pair_rec.resize(h->bench_ev.size());
    const int slot = h->bench_pending++;
    const auto& ev = h->bench_ev[slot];
    h->bench_pair_rec[slot] = 0;
    HIP_OK(hipEventRecord(ev[0], s));
    if (with_assembly) {
      bool prec = false;
      CHECK_RC(eval_pass(h, false, ev[1], ev[2], ev[4], ev[5], &prec));
      h->bench_pair_rec[slot] = prec;
      CHECK_RC(h->allreduce_cost());
      CHECK_RC(intr_pass());
    } else {
      if (eval_points_needs_camtab(h->eval_wps)) launch_cam_tables(s, h->E, h->d_ext, h->d_camtab);
      HIP_OK(hipEventRecord(ev[1], s));
      if (eval_points_fx(h->eval_wps)) h->fx_last ^= 1;
      h->cost_fx_pending = eval_points_fx(h->eval_wps);
      launch_eval_points(s, h->view, h->d_points, h->d_ext, h->d_camtab, h->d_V, h->d_g, h->d_gpart, h->d_arrivals,
                         h->d_scal + S_COST, h->cost_fx(h->fx_last), h->cost_fx(h->fx_last ^ 1), h->eval_grid,
                         h->eval_wps);
      HIP_OK(hipEventRecord(ev[2], s));
    }
    HIP_OK(hipEventRecord(ev[3], s));
  }
  return 0;
}

// the handle's sticky error word (dab_sync after bench passes), cleared once read
static int xerr_check_sticky(dab_handle* h) {
  unsigned e = 0;
  std::memcpy(&e, h->h_scal + S_XERR, sizeof(e));
  if (e == 0) return 0;
  HIP_OK(hipMemsetAsync(h->d_scal + S_XERR, 0, sizeof(double), h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));
  return xerr_fail(e);
}
extern "C" int dab_sync(dab_handle* h) {
  clear_error();
  if (!h) return set_error(DAB_E_INVALID, "null handle");
  HIP_OK(hipSetDevice(h->device));
  HIP_OK(hipStreamSynchronize(h->stream));
  if (h->d_scal) {
    HIP_OK(hipMemcpy(h->h_scal + S_XERR, h->d_scal + S_XERR, sizeof(double), hipMemcpyDeviceToHost));
    CHECK_RC(xerr_check_sticky(h));
  }
  return 0;
}

extern "C" int dab_bench_get_blocks(dab_handle* h, int32_t* num_free_ext, int32_t* num_cross, double* V, double* g,
                                    double* ug, double* ux, double* cost) {
  clear_error();
  if (!h || !h->have_problem) return set_error(DAB_E_STATE, "no problem set");
  HIP_OK(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  if (num_free_ext) *num_free_ext = h->NC;
  if (num_cross) *num_cross = h->ncross;
  const size_t NP = (size_t)h->NP;
  if (V || g) {
    std::vector<double> hv(6 * NP), hg(3 * NP);
    if (NP > 0) {
      HIP_OK(hipMemcpyAsync(hv.data(), h->d_V, hv.size() * sizeof(double), hipMemcpyDeviceToHost, s));
      HIP_OK(hipMemcpyAsync(hg.data(), h->d_g, hg.size() * sizeof(double), hipMemcpyDeviceToHost, s));
      HIP_OK(hipStreamSynchronize(s));
    }
    const size_t npts = (size_t)h->prob.num_points;
    if (V) std::fill(V, V + 6 * npts, 0.0);
    if (g) std::fill(g, g + 3 * npts, 0.0);
    for (size_t i = 0; i < NP; ++i) {
      const size_t p = (size_t)h->pt_of[i];
      if (V)
        for (int k = 0; k < 6; ++k) V[6 * p + k] = hv[k * NP + i];
      if (g)
        for (int k = 0; k < 3; ++k) g[3 * p + k] = hg[k * NP + i];
    }
  }
  if (ug && h->NC > 0)
    HIP_OK(hipMemcpyAsync(ug, h->ug(), sizeof(double) * 27 * (size_t)h->NC, hipMemcpyDeviceToHost, s));
  if (ux && h->NC > 0 && h->ncross > 0)
    HIP_OK(hipMemcpyAsync(ux, h->Ux(), sizeof(double) * 36 * (size_t)h->ncross, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  if (cost) {
    // read_scalars converts a fixed-point cost once and clears the flag: put it back, so
    // that this read leaves the handle as it found it
    const bool pending = h->cost_fx_pending;
    CHECK_RC(read_scalars(h));
    h->cost_fx_pending = pending;
    *cost = 0.5 * h->h_scal[S_COST];
  }
  return 0;
}

extern "C" int dab_bench_kernel_ms(dab_handle* h, double* jac_ms, double* assembly_ms) {
  clear_error();
  if (!h) return set_error(DAB_E_INVALID, "null handle");
  CHECK_RC(collect_bench_events(h));
  const double n = h->bench_count > 0 ? h->bench_count : 1;
  if (jac_ms) *jac_ms = h->bench_jac_ms / n;
  if (assembly_ms) *assembly_ms = h->bench_asm_ms / n;
  h->last_pair_ms = h->bench_pair_count > 0 ? h->bench_pair_ms / h->bench_pair_count : 0.0;
  h->bench_jac_ms = h->bench_asm_ms = h->bench_pair_ms = 0;
  h->bench_count = h->bench_pair_count = 0;
  return 0;
}

extern "C" int dab_bench_pair_ms(dab_handle* h, double* ms, double* bytes) {
  clear_error();
  if (!h || !h->have_problem) return set_error(DAB_E_STATE, "no problem set");
  // Algorithmic bytes of one k_eval_pair launch (the rig's composed observations whose two
  // cameras are free, pair-major): per observation the 16-B pixel and three index words
  // (point, arc, ring; the intrinsic is the arc's), the 24-B point once per distinct point
  // the pass touches, and per chunk its 90 sums out (two camera halves + the cross block).
  // The point array is read, in this order, by random gathers.
  if (ms) *ms = h->last_pair_ms;
  if (bytes) *bytes = h->pair_eval ? h->pair_bytes : 0.0;
  return 0;
}

extern "C" int dab_jacobian_bytes(dab_handle* h, double* bytes) {
  clear_error();
  if (!h || !h->have_problem) return set_error(DAB_E_STATE, "no problem set");
  // Algorithmic bytes of one launch of the point-side evaluation kernel (k_eval_points,
  // matrix-free residual + Jacobian reduced into V, g): the SURVEY §8d input terms
  // (16 xy + 4 n_idx per observation, n_idx = 2 single / 3 arc∘ring; 24 per point,
  // 48 per intrinsic, 48 per extrinsic) plus the outputs V, g per point (72 B). The
  // LDS variants build R, t from the 48-B extrinsics; the global-table variants read the
  // 96-B R, t part of the camera tables instead. The Jacobian itself never reaches HBM, so
  // its 16 k bytes per observation are not counted (they are not moved).
  // The fused pass (k_eval_bal) also produces the camera side: it writes U | g_c (216 B
  // per free camera) and reads every entry a second time in camera-major order (20 B:
  // point index + pixel; the chunk's camera and intrinsic are per block). A deterministic
  // matrix-free pass needs both traversal orders (point-major for V, g; camera-major for
  // U, g_c: no atomics, no per-observation partials), so both reads are algorithmic.
  // This is the minimal count whatever the implementation reads: no denormalised copies, no
  // re-gathers of a point, each traversal's index words once.
  double b = (24.0 + 72.0) * h->NP + 48.0 * h->E + 48.0 * h->NI;
  if (h->fused) b += 216.0 * h->NC + 20.0 * h->NE;
  for (int o = 0; o < h->N; ++o) b += 16.0 + 4.0 * (h->prob.obs_ext1[o] >= 0 ? 3 : 2);
  *bytes = b;
  return 0;
}
