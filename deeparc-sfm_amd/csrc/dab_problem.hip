// dab_problem.hip — dab_set_problem: validation, the orderings and reduction tables of a
// problem (on the host, or on the device through dab_setup.hip), its work buffers and the
// device view; and the free-intrinsic state of the handle with its entry points.
#include "dab_handle.h"

using namespace dab;

// Pair-major chunks: a pair of n records is cut into ceil(n / most) equal pieces (the last
// one shorter by less than one per piece), not into full chunks and a ragged remainder:
// every chunk's work-group then runs about the same number of iterations per lane
static size_t pair_piece(size_t n, int most) {
  const size_t m = (size_t)std::max(1, most), parts = std::max<size_t>(1, (n + m - 1) / m);
  return std::max<size_t>(1, (n + parts - 1) / parts);
}

// ------------------------------------------------------------------------------------
// problem setup: orderings and reduction tables (built once)
// ------------------------------------------------------------------------------------
static int validate(const dab_problem* p) {
  if (!p) return set_error(DAB_E_INVALID, "null problem");
  if (p->num_obs < 0 || p->num_points < 0 || p->num_ext < 0 || p->num_intr < 0)
    return set_error(DAB_E_INVALID, "negative size");
  if (p->num_obs > 0 && (!p->obs_xy || !p->obs_point || !p->obs_ext0 || !p->obs_ext1 || !p->obs_intr))
    return set_error(DAB_E_INVALID, "null observation array");
  if ((p->num_points > 0 && !p->points) || (p->num_ext > 0 && !p->ext) ||
      (p->num_intr > 0 && (!p->intr || !p->intr_nf || !p->intr_nk)))
    return set_error(DAB_E_INVALID, "null parameter array");
  for (int i = 0; i < p->num_intr; ++i) {
    if (p->intr_nf[i] < 1 || p->intr_nf[i] > 2) return set_error(DAB_E_INVALID, "intr_nf must be 1 or 2");
    if (p->intr_nk[i] < 0 || p->intr_nk[i] > 2) return set_error(DAB_E_INVALID, "intr_nk must be 0, 1 or 2");
  }
  return 0;
}
// per-observation index ranges (the host path; the device path checks them in su_count)
static int validate_obs(const dab_problem* p) {
  for (int o = 0; o < p->num_obs; ++o) {
    const int pt = p->obs_point[o], e0 = p->obs_ext0[o], e1 = p->obs_ext1[o], ii = p->obs_intr[o];
    if (pt < 0 || pt >= p->num_points || e0 < 0 || e0 >= p->num_ext || e1 < -1 || e1 >= p->num_ext ||
        ii < 0 || ii >= p->num_intr)
      return set_error(DAB_E_INVALID, "observation " + std::to_string(o) + " has an out-of-range index");
  }
  return 0;
}

// The host reference path of the set-up (DAB_SETUP_HOST=1; multi-rank problems and sizes
// setup_device_fits refuses): stable counting sorts and gathers on host threads, then the
// uploads. setup_device builds the same arrays on the GPU.
// whether the camera chunks' (ext, intr) pairs are an affine map of the chunk index (one
// chunk per free camera, both indices offset by a constant): the fused pass then computes them
static void set_uni_affine(dab_handle* h, const std::vector<int2>& cu) {
  h->uni_affine = 0;
  h->uni_ox = h->uni_oi = 0;
  if (cu.empty() || (int)cu.size() != h->NC) return;
  const int ox = cu[0].x, oi = cu[0].y;
  if (ox < 0 || oi < 0) return;
  for (size_t c = 0; c < cu.size(); ++c)
    if (cu[c].x != (int)c + ox || cu[c].y != (int)c + oi) return;
  h->uni_affine = 1;
  h->uni_ox = ox;
  h->uni_oi = oi;
}
// the point kernel's arrival counter and the chunk ids, the uniform ones first (ChunkLists)
static int upload_chunk_lists(dab_handle* h, const std::vector<int2>& chunk_uni) {
  CHECK_RC(h->dev.alloc(&h->d_arrivals, 1));
  HIP_OK(hipMemsetAsync(h->d_arrivals, 0, sizeof(unsigned), h->stream));
  std::vector<int> lists;
  for (int q = 0; q < h->nchunk; ++q)
    if (chunk_uni[q].x >= 0) lists.push_back(q);
  const int nuni = (int)lists.size();
  for (int q = 0; q < h->nchunk; ++q)
    if (chunk_uni[q].x < 0) lists.push_back(q);
  CHECK_RC(upload(&h->d_chunk_lists, h->dev, lists, h->stream));
  h->chunks.nchunk = h->nchunk;
  h->chunks.nuni = nuni;
  h->chunks.ngen = h->nchunk - nuni;
  h->chunks.uni = h->d_chunk_lists;
  h->chunks.gen = h->d_chunk_lists + nuni;
  return 0;
}
// the tables and buffers of the linear solvers are built on first use (dab_schur_tables.hip):
// none yet for a new problem
static void reset_solver_tables(dab_handle* h) {
  h->schur_built = false;
  h->schur_tiles = false;
  h->pcg_built = false;
  h->mf = h->mf32 = false;
  h->cg_wpart = nullptr;  // its buffer went with the previous problem's allocations
  h->fused_grid = 0;      // so did the single-pass product's partials
  h->mf_grid_n = 0;
  h->nblk = 0;
  h->nzero = 0;
  h->npairs = 0;
}
// the device layout of the intrinsics: (cx, cy, fx, fy', k0, k1, 0, 0), unused distortion terms
// zeroed, from the dab_problem layout [NI][6]
static std::vector<double> device_intrinsics(int NI, const double* intr, const int* nf, const int* nk) {
  std::vector<double> K((size_t)kIntr * std::max(1, NI), 0.0);
  for (int i = 0; i < NI; ++i) {
    const double* in = intr + 6 * (size_t)i;
    double* o = &K[(size_t)kIntr * i];
    o[0] = in[0];
    o[1] = in[1];
    o[2] = in[2];
    o[3] = nf[i] == 2 ? in[3] : in[2];
    o[4] = nk[i] >= 1 ? in[4] : 0.0;
    o[5] = nk[i] >= 2 ? in[5] : 0.0;
  }
  return K;
}
static int setup_host(dab_handle* h, const dab_problem* p, PhaseTimer& phase) {
  CHECK_RC(validate_obs(p));
  h->setup_tmp.clear();  // a previous device set-up's scratch (the host path needs none)
  const int N = p->num_obs;
  hipStream_t s = h->stream;
  // referenced points (local compact ids, in id order) and extrinsics
  std::vector<int> pt_local(p->num_points, -1);
  std::vector<char> pref(p->num_points, 0);
  std::vector<double> eref(std::max(1, p->num_ext), 0.0);
  h->any_compose = false;
  for (int o = 0; o < N; ++o) {
    pref[p->obs_point[o]] = 1;
    eref[p->obs_ext0[o]] = 1.0;
    if (p->obs_ext1[o] >= 0) {
      eref[p->obs_ext1[o]] = 1.0;
      h->any_compose = true;
    }
  }
  // device point order: referenced points by observation count, descending (stable by
  // id), so that the 64 points of one wave slice have similar track lengths (SELL-64)
  std::vector<int> pcount(p->num_points, 0);
  int maxcount = 0;
  for (int o = 0; o < N; ++o) maxcount = std::max(maxcount, ++pcount[p->obs_point[o]]);
  {  // counting sort by count, descending, stable by id (linear: set-up recurs per filter round)
    std::vector<int> start(maxcount + 2, 0);
    int npref = 0;
    for (int i = 0; i < p->num_points; ++i)
      if (pref[i]) {
        start[maxcount - pcount[i] + 1]++;
        ++npref;
      }
    for (int k = 0; k <= maxcount; ++k) start[k + 1] += start[k];
    h->pt_of.assign(npref, 0);
    for (int i = 0; i < p->num_points; ++i)
      if (pref[i]) h->pt_of[start[maxcount - pcount[i]]++] = i;
  }
  for (int l = 0; l < (int)h->pt_of.size(); ++l) pt_local[h->pt_of[l]] = l;
  h->NP = (int)h->pt_of.size();
  // the free camera set must agree on every rank
  if (h->world > 1) {
    double* d_tmp = nullptr;
    CHECK_RC(h->dev.alloc(&d_tmp, eref.size() + 1));
    eref.push_back(h->any_compose ? 1.0 : 0.0);
    HIP_OK(hipMemcpyAsync(d_tmp, eref.data(), eref.size() * sizeof(double), hipMemcpyHostToDevice, s));
    CHECK_RC(h->allreduce(d_tmp, eref.size(), ncclMax));
    HIP_OK(hipMemcpyAsync(eref.data(), d_tmp, eref.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    h->any_compose = eref.back() != 0.0;
    eref.pop_back();
  }
  h->ext_col.assign(p->num_ext, -1);
  h->ext_fixed.assign(p->num_ext, 0);
  h->NC = 0;
  for (int e = 0; e < p->num_ext; ++e) {
    const bool is_const = p->freeze_camera || (p->ext_const && p->ext_const[e]);
    h->ext_fixed[e] = is_const;
    if (eref[e] != 0.0 && !is_const) h->ext_col[e] = h->NC++;
  }
  const int NP = h->NP, NC = h->NC;
  h->nplanes = h->any_compose ? 30 : 18;
  phase("points, cameras");

  // Observation slots, SELL-64: slice sl holds local points [64 sl, 64 sl + 64); the k-th
  // observation (caller order) of the slice's lane-l point sits at slice_off[sl] + 64 k + l,
  // slices padded to their longest track (padding slots: point -1). One wave walks a
  // slice with every load coalesced and reduces V, g per lane with no cross-lane work.
  std::vector<int> cnt(NP + 1, 0);
  big_vec<int> by_pt;
  {
    std::vector<long long> st;
    bucket_sort(N, NP, [&](long long o) { return pt_local[p->obs_point[o]]; }, by_pt, st);
    for (int i = 0; i <= NP; ++i) cnt[i] = (int)st[i];
  }
  h->nslice = (NP + 63) / 64;
  std::vector<int> slice_off(h->nslice + 1, 0);
  for (int sl = 0; sl < h->nslice; ++sl) {
    const int p0 = 64 * sl;
    const int len = cnt[p0 + 1] - cnt[p0];  // longest track of the slice (sorted)
    slice_off[sl + 1] = slice_off[sl] + 64 * len;
  }
  const int NS = slice_off[h->nslice];
  h->NS = NS;
  h->perm.resize(NS);
  big_vec<int4> obs_idx(NS);
  big_vec<double2> obs_xy(NS);
  // entries (observation slots on free cameras), point-major: counted per point first
  std::vector<int> pt_ent_ptr(NP + 1, 0);
  par_for(64LL * h->nslice, [&](long long b, long long e, int) {
    for (int pt = (int)b; pt < (int)e; ++pt) {
      const int sl = pt / 64, lane = pt % 64;
      const int len = pt < NP ? cnt[pt + 1] - cnt[pt] : 0;
      for (int k = len; k < (slice_off[sl + 1] - slice_off[sl]) / 64; ++k) {  // padding slots
        const int slot = slice_off[sl] + 64 * k + lane;
        h->perm[slot] = -1;
        obs_idx[slot] = make_int4(-1, 0, -1, 0);
        obs_xy[slot] = make_double2(0.0, 0.0);
      }
      if (pt >= NP) continue;
      int ne = 0;
      for (int k = 0; k < len; ++k) {
        const int slot = slice_off[sl] + 64 * k + lane;
        const int o = by_pt[cnt[pt] + k];
        h->perm[slot] = o;
        obs_idx[slot] = make_int4(pt, p->obs_ext0[o], p->obs_ext1[o], p->obs_intr[o]);
        obs_xy[slot] = make_double2(p->obs_xy[2 * (size_t)o], p->obs_xy[2 * (size_t)o + 1]);
        ne += p->obs_ext0[o] >= 0 && h->ext_col[p->obs_ext0[o]] >= 0;
        ne += p->obs_ext1[o] >= 0 && h->ext_col[p->obs_ext1[o]] >= 0;
      }
      pt_ent_ptr[pt + 1] = ne;
    }
  });
  for (int pt = 0; pt < NP; ++pt) pt_ent_ptr[pt + 1] += pt_ent_ptr[pt];
  h->NE = pt_ent_ptr[NP];
  big_vec<int> ent_os(h->NE), ent_cam(h->NE), ent_pt(h->NE);
  par_for(NP, [&](long long b, long long e, int) {
    for (int pt = (int)b; pt < (int)e; ++pt) {
      const int sl = pt / 64, lane = pt % 64;
      int q = pt_ent_ptr[pt];
      for (int k = 0; k < cnt[pt + 1] - cnt[pt]; ++k) {
        const int s2 = slice_off[sl] + 64 * k + lane;
        for (int slot = 0; slot < 2; ++slot) {
          const int ex = slot ? obs_idx[s2].z : obs_idx[s2].y;
          if (ex < 0 || h->ext_col[ex] < 0) continue;
          ent_os[q] = 2 * s2 + slot;
          ent_cam[q] = h->ext_col[ex];
          ent_pt[q] = pt;
          ++q;
        }
      }
    }
  });
  phase("slots, entries");
  const int NE = h->NE;

  // camera-major entry lists, chunked (deterministic two-level reductions)
  big_vec<int> cam_ent;
  std::vector<int> cam_cnt(NC + 1, 0);
  {
    std::vector<long long> st;
    bucket_sort(NE, NC, [&](long long e) { return ent_cam[e]; }, cam_ent, st);
    for (int c = 0; c <= NC; ++c) cam_cnt[c] = (int)st[c];
  }
  // entries per reduction chunk (one block each); DAB_CHUNK is a tuning knob
  const int chunk = std::max(64, h->knobs.chunk > 0 ? h->knobs.chunk : kChunk);
  std::vector<int> chunk_beg, seg_chunk(NC + 1, 0);
  for (int c = 0; c < NC; ++c) {
    seg_chunk[c] = (int)chunk_beg.size();
    for (int b = cam_cnt[c]; b < cam_cnt[c + 1]; b += chunk) chunk_beg.push_back(b);
  }
  seg_chunk[NC] = (int)chunk_beg.size();
  h->nchunk = (int)chunk_beg.size();
  h->max_seg_chunks = 1;
  for (int c = 0; c < NC; ++c) h->max_seg_chunks = std::max(h->max_seg_chunks, seg_chunk[c + 1] - seg_chunk[c]);
  chunk_beg.push_back(NE);
  // camera-major record positions of the entries, and per observation
  big_vec<int> ent_pos(NE), cm_pt(NE);
  par_for(NE, [&](long long b, long long e, int) {
    for (long long i = b; i < e; ++i) {
      ent_pos[cam_ent[i]] = (int)i;
      cm_pt[i] = ent_pt[cam_ent[i]];
    }
  });
  // runs of one point inside one camera's positions (rig: a point seen by one arc through
  // several rings has several entries of that camera); run[i] = run length at its first
  // position, 0 elsewhere. The diagonal S block needs (sum_run Y)(sum_run Y)^T.
  std::vector<int> run(NE, 0);
  par_for(NC, [&](long long b, long long e, int) {
    for (int c = (int)b; c < (int)e; ++c) {
      int i = cam_cnt[c];
      while (i < cam_cnt[c + 1]) {
        int j = i + 1;
        while (j < cam_cnt[c + 1] && cm_pt[j] == cm_pt[i]) ++j;
        run[i] = j - i;
        i = j;
      }
    }
  }, 1);
  // static camera-major copy of the entries' observation inputs (matrix-free camera passes)
  big_vec<int4> cm_idx(NE);
  // the runs of each chunk as records {first position, length, point, camera} in position
  // order (k_mf_diag_frame: its loads need no dependent index load; run_beg[nchunk + 1])
  std::vector<int> run_beg(h->nchunk + 1, 0);
  par_for(h->nchunk, [&](long long b, long long e, int) {
    for (int c = (int)b; c < (int)e; ++c) {
      int n = 0;
      for (int i = chunk_beg[c]; i < chunk_beg[c + 1]; ++i) n += run[i] > 0;
      run_beg[c + 1] = n;
    }
  }, 64);
  for (int c = 0; c < h->nchunk; ++c) run_beg[c + 1] += run_beg[c];
  big_vec<int4> run_rec(std::max(1, run_beg[h->nchunk]));
  big_vec<double2> cm_xy(NE);
  par_for(NE, [&](long long b, long long en, int) {
    for (long long i = b; i < en; ++i) {
      const int e = cam_ent[i], s2 = ent_os[e] >> 1;
      int4 id = obs_idx[s2];
      if (ent_os[e] & 1) id.w |= kSlotBit;
      cm_idx[i] = id;
      cm_xy[i] = obs_xy[s2];
    }
  });
  par_for(NC, [&](long long b, long long e, int) {
    for (int c = (int)b; c < (int)e; ++c)
      for (int q = seg_chunk[c]; q < seg_chunk[c + 1]; ++q) {
        int k = run_beg[q];
        for (int i = chunk_beg[q]; i < chunk_beg[q + 1]; ++i)
          if (run[i] > 0) run_rec[k++] = make_int4(i, run[i], cm_pt[i], c);
      }
  }, 1);
  // chunks whose entries all see one camera through one intrinsic (single-extrinsic
  // observations): the camera passes read that camera's tables once per block
  std::vector<int2> chunk_uni(h->nchunk, make_int2(-1, -1));
  par_for(h->nchunk, [&](long long b, long long e, int) {
    for (int q = (int)b; q < (int)e; ++q) {
      const int4 first = cm_idx[chunk_beg[q]];
      bool uni = first.z < 0 && !(first.w & kSlotBit);
      for (int i = chunk_beg[q]; uni && i < chunk_beg[q + 1]; ++i)
        uni = cm_idx[i].z < 0 && cm_idx[i].y == first.y && cm_idx[i].w == first.w;
      if (uni) chunk_uni[q] = make_int2(first.y, first.w);
    }
  }, 16);
  phase("camera-major");
  // arc∘ring cross blocks: composed observations whose two cameras are both free.
  // The pair table is the union over ranks so the all-reduced layout matches.
  // keys (c0 NC + c1) NS + s2 in increasing order: a counting sort by camera pair over the
  // slots in increasing order (linear; the comparison sort of 9M keys took ~1 s at C5)
  big_vec<long long> xkeys;
  if (h->any_compose && NC > 0) {
    // the two free cameras of a composed slot (-1: not a cross observation)
    auto cams_of = [&](long long s2) -> int2 {
      const int e1 = obs_idx[s2].z;
      if (e1 < 0 || obs_idx[s2].x < 0) return make_int2(-1, -1);
      const int c0 = h->ext_col[obs_idx[s2].y], c1 = h->ext_col[e1];
      if (c0 < 0 || c1 < 0) return make_int2(-1, -1);
      return make_int2(c0, c1);
    };
    // (c0, c1, slot) order by two stable NC-bucket passes (by c1, then by c0): counters of
    // NC per thread, not NC^2, and the 64-bit key below does not overflow
    big_vec<int> o1, o2;
    std::vector<long long> st1, st2;
    bucket_sort(NS, NC, [&](long long s2) { return cams_of(s2).y; }, o1, st1);
    bucket_sort((long long)o1.size(), NC, [&](long long j) { return cams_of(o1[j]).x; }, o2, st2);
    xkeys.resize(o2.size());
    par_for((long long)o2.size(), [&](long long b, long long e, int) {
      for (long long i = b; i < e; ++i) {
        const int s2 = o1[o2[i]];
        const int2 c = cams_of(s2);
        xkeys[i] = ((long long)c.x * NC + c.y) * (long long)NS + s2;
      }
    });
  }
  std::vector<long long> pairkeys;  // unique (c0*NC+c1)
  for (long long k : xkeys) {
    const long long pk = k / NS;
    if (pairkeys.empty() || pairkeys.back() != pk) pairkeys.push_back(pk);
  }
  if (h->world > 1 && h->any_compose && NC > 0) {
    // union of pair keys via an NC x NC bitmap all-reduce(max)
    std::vector<double> bm((size_t)NC * NC, 0.0);
    for (long long pk : pairkeys) bm[(size_t)pk] = 1.0;
    double* d_bm = nullptr;
    CHECK_RC(h->dev.alloc(&d_bm, bm.size()));
    HIP_OK(hipMemcpyAsync(d_bm, bm.data(), bm.size() * sizeof(double), hipMemcpyHostToDevice, s));
    CHECK_RC(h->allreduce(d_bm, bm.size(), ncclMax));
    HIP_OK(hipMemcpyAsync(bm.data(), d_bm, bm.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    pairkeys.clear();
    for (size_t i = 0; i < bm.size(); ++i)
      if (bm[i] != 0.0) pairkeys.push_back((long long)i);
  }
  h->ncross = (int)pairkeys.size();
  std::vector<int2> cross_cam(h->ncross);
  for (int k = 0; k < h->ncross; ++k) cross_cam[k] = make_int2((int)(pairkeys[k] / NC), (int)(pairkeys[k] % NC));
  std::vector<int> xchunk_beg, xseg_chunk(h->ncross + 1, 0);
  big_vec<int4> x_idx(xkeys.size());
  big_vec<double2> x_xy(xkeys.size());
  {
    par_for((long long)xkeys.size(), [&](long long b, long long e, int) {
      for (long long i = b; i < e; ++i) {
        const int s2 = (int)(xkeys[i] % NS);
        x_idx[i] = obs_idx[s2];
        x_xy[i] = obs_xy[s2];
      }
    });
    std::vector<size_t> pbeg(h->ncross + 1, 0);
    std::vector<long long> pcnt(h->ncross, 0);
    size_t i = 0;
    for (int k = 0; k < h->ncross; ++k) {
      pbeg[k] = i;
      while (i < xkeys.size() && xkeys[i] / NS == pairkeys[k]) ++i;
      pcnt[k] = (long long)(i - pbeg[k]);
    }
    const int xchunk = std::max(64, h->knobs.xchunk > 0 ? h->knobs.xchunk : kPairChunk);
    for (int k = 0; k < h->ncross; ++k) {
      xseg_chunk[k] = (int)xchunk_beg.size();
      const size_t b = pbeg[k], piece = pair_piece((size_t)pcnt[k], xchunk);
      for (size_t q = b; q < b + (size_t)pcnt[k]; q += piece) xchunk_beg.push_back((int)q);
    }
    xseg_chunk[h->ncross] = (int)xchunk_beg.size();
    h->nxchunk = (int)xchunk_beg.size();
    h->max_xseg_chunks = 1;
    for (int k = 0; k < h->ncross; ++k)
      h->max_xseg_chunks = std::max(h->max_xseg_chunks, xseg_chunk[k + 1] - xseg_chunk[k]);
    xchunk_beg.push_back((int)xkeys.size());
  }

  // per-camera CSR of cross blocks for the implicit operator: code = 2 k + (camera is c1)
  std::vector<int> xptr(NC + 1, 0), xlist;
  {
    std::vector<std::vector<int>> per(NC);
    for (int k = 0; k < h->ncross; ++k) {
      per[cross_cam[k].x].push_back(2 * k);
      per[cross_cam[k].y].push_back(2 * k + 1);
    }
    for (int c = 0; c < NC; ++c) {
      xptr[c] = (int)xlist.size();
      xlist.insert(xlist.end(), per[c].begin(), per[c].end());
    }
    if (NC > 0) xptr[NC] = (int)xlist.size();
    h->nxlist = (int)xlist.size();
  }

  // pair-major evaluation (rig): the composed observations with both cameras free are
  // evaluated per (arc, ring) pair chunk; the remaining camera-major entries keep chunks
  // of their own, and every camera lists its halves of the pair chunks (increasing chunk)
  big_vec<int4> cm2_idx;
  big_vec<double2> cm2_xy;
  std::vector<int> chunk2_beg, seg2_chunk(NC + 1, 0), xcam_ptr(NC + 1, 0), xcam_list;
  h->pair_eval = h->nxchunk > 0 && pair_eval_fits(h->E, h->NI) && h->knobs.pair_eval != 0;
  if (h->pair_eval) {
    {  // algorithmic bytes of one k_eval_pair launch (dab_bench_pair_ms)
      std::vector<char> touched(NP, 0);
      long long npt = 0;
      for (long long k : xkeys) {
        const int p = obs_idx[(int)(k % NS)].x;
        if (p >= 0 && !touched[p]) {
          touched[p] = 1;
          ++npt;
        }
      }
      h->pair_bytes = (16.0 + 12.0) * (double)xkeys.size() + 24.0 * (double)npt + 90.0 * 8.0 * h->nxchunk;
      h->pair_uni_intr = true;
      for (size_t i = 1; i < x_idx.size() && h->pair_uni_intr; ++i)
        if (x_idx[i].y == x_idx[i - 1].y && x_idx[i].z == x_idx[i - 1].z && x_idx[i].w != x_idx[i - 1].w)
          h->pair_uni_intr = false;
    }
    // the entries that are not paired, per camera (counted, then filled in parallel)
    auto unpaired = [&](int i) {
      const int4 id = cm_idx[i];
      return !(id.z >= 0 && h->ext_col[id.y] >= 0 && h->ext_col[id.z] >= 0);
    };
    std::vector<int> c2cnt(NC + 1, 0);
    par_for(NC, [&](long long b, long long e, int) {
      for (int c = (int)b; c < (int)e; ++c) {
        int n2 = 0;
        for (int i = cam_cnt[c]; i < cam_cnt[c + 1]; ++i) n2 += unpaired(i);
        c2cnt[c + 1] = n2;
      }
    }, 1);
    for (int c = 0; c < NC; ++c) c2cnt[c + 1] += c2cnt[c];
    cm2_idx.resize(c2cnt[NC]);
    cm2_xy.resize(c2cnt[NC]);
    par_for(NC, [&](long long b, long long e, int) {
      for (int c = (int)b; c < (int)e; ++c) {
        int q = c2cnt[c];
        for (int i = cam_cnt[c]; i < cam_cnt[c + 1]; ++i)
          if (unpaired(i)) {
            cm2_idx[q] = cm_idx[i];
            cm2_xy[q] = cm_xy[i];
            ++q;
          }
      }
    }, 1);
    for (int c = 0; c < NC; ++c) {
      seg2_chunk[c] = (int)chunk2_beg.size();
      for (int q = c2cnt[c]; q < c2cnt[c + 1]; q += chunk) chunk2_beg.push_back(q);
    }
    seg2_chunk[NC] = (int)chunk2_beg.size();
    h->nchunk2 = (int)chunk2_beg.size();
    chunk2_beg.push_back((int)cm2_idx.size());
    std::vector<std::vector<int>> per(NC);
    for (int k = 0; k < h->ncross; ++k)
      for (int q = xseg_chunk[k]; q < xseg_chunk[k + 1]; ++q) {
        per[cross_cam[k].x].push_back(2 * q);
        per[cross_cam[k].y].push_back(2 * q + 1);
      }
    for (int c = 0; c < NC; ++c) {
      std::sort(per[c].begin(), per[c].end());
      xcam_ptr[c] = (int)xcam_list.size();
      xcam_list.insert(xcam_list.end(), per[c].begin(), per[c].end());
    }
    xcam_ptr[NC] = (int)xcam_list.size();
  }

  phase("pair-major");
  reset_solver_tables(h);

  const std::vector<double> intr = device_intrinsics(h->NI, p->intr, p->intr_nf, p->intr_nk);
  std::vector<double> points((size_t)3 * NP);
  for (int i = 0; i < NP; ++i)
    for (int k = 0; k < 3; ++k) points[3 * (size_t)i + k] = p->points[3 * (size_t)h->pt_of[i] + k];
  std::vector<double> ext(p->ext, p->ext + 6 * (size_t)h->E);

  phase("host copies");
  // ---- upload ----
  Dev& d = h->dev;
  CHECK_RC(upload(&h->d_obs_idx, d, obs_idx, s));
  CHECK_RC(upload(&h->d_obs_xy, d, obs_xy, s));
  CHECK_RC(upload(&h->d_slice_off, d, slice_off, s));
  CHECK_RC(upload(&h->d_pt_ent_ptr, d, pt_ent_ptr, s));
  CHECK_RC(upload(&h->d_ent_os, d, ent_os, s));
  CHECK_RC(upload(&h->d_ent_cam, d, ent_cam, s));
  CHECK_RC(upload(&h->d_ent_pt, d, ent_pt, s));
  CHECK_RC(upload(&h->d_ext_col, d, h->ext_col, s));
  CHECK_RC(upload(&h->d_ent_pos, d, ent_pos, s));
  CHECK_RC(upload(&h->d_cm_pt, d, cm_pt, s));
  CHECK_RC(upload(&h->d_cm_idx, d, cm_idx, s));
  CHECK_RC(upload(&h->d_cm_xy, d, cm_xy, s));
  CHECK_RC(upload(&h->d_chunk_beg, d, chunk_beg, s));
  CHECK_RC(upload(&h->d_chunk_uni, d, chunk_uni, s));
  set_uni_affine(h, chunk_uni);
  CHECK_RC(upload_chunk_lists(h, chunk_uni));
  CHECK_RC(upload(&h->d_seg_chunk, d, seg_chunk, s));
  CHECK_RC(upload(&h->d_x_idx, d, x_idx, s));
  CHECK_RC(upload(&h->d_x_xy, d, x_xy, s));
  CHECK_RC(upload(&h->d_xchunk_beg, d, xchunk_beg, s));
  CHECK_RC(upload(&h->d_xseg_chunk, d, xseg_chunk, s));
  CHECK_RC(upload(&h->d_cross_cam, d, cross_cam, s));
  CHECK_RC(upload(&h->d_xptr, d, xptr, s));
  CHECK_RC(upload(&h->d_run, d, run, s));
  CHECK_RC(upload(&h->d_run_beg, d, run_beg, s));
  CHECK_RC(upload(&h->d_run_rec, d, run_rec, s));
  CHECK_RC(upload(&h->d_xlist, d, xlist, s));
  if (h->pair_eval) {
    if (!cm2_idx.empty()) {
      CHECK_RC(upload(&h->d_cm2_idx, d, cm2_idx, s));
      CHECK_RC(upload(&h->d_cm2_xy, d, cm2_xy, s));
    }
    CHECK_RC(upload(&h->d_chunk2_beg, d, chunk2_beg, s));
    CHECK_RC(upload(&h->d_seg2_chunk, d, seg2_chunk, s));
    CHECK_RC(upload(&h->d_xcam_ptr, d, xcam_ptr, s));
    if (!xcam_list.empty()) CHECK_RC(upload(&h->d_xcam_list, d, xcam_list, s));
    CHECK_RC(d.alloc(&h->d_partial2, (size_t)std::max(1, h->nchunk2) * 27));
    CHECK_RC(d.alloc(&h->d_xcpart, (size_t)h->nxchunk * 54));
  }
  CHECK_RC(upload(&h->d_intr, d, intr, s));
  CHECK_RC(upload(&h->d_points, d, points, s));
  CHECK_RC(upload(&h->d_ext, d, ext, s));
  h->local_compose = false;
  for (int o = 0; o < N && !h->local_compose; ++o) h->local_compose = p->obs_ext1[o] >= 0;
  h->h_pt_ent_ptr = std::move(pt_ent_ptr);
  h->h_ent_cam = std::move(ent_cam);
  h->h_ent_pos = std::move(ent_pos);
  h->h_ent_os = std::move(ent_os);
  h->host_entries = true;
  return 0;
}

// Work buffers, launch geometry and the device view, common to both set-up paths.
static int setup_buffers(dab_handle* h, PhaseTimer& phase) {
  hipStream_t s = h->stream;
  Dev& d = h->dev;
  const int NP = h->NP, NC = h->NC, NS = h->NS, NE = h->NE;
  CHECK_RC(d.alloc(&h->d_points_c, (size_t)3 * NP));
  CHECK_RC(d.alloc(&h->d_ext_c, (size_t)6 * h->E));
  CHECK_RC(d.alloc(&h->d_camtab, (size_t)kCamTab * h->E));
  CHECK_RC(d.alloc(&h->d_camtab_c, (size_t)kCamTab * h->E));
  CHECK_RC(d.alloc(&h->d_r, (size_t)2 * NS));
  CHECK_RC(d.alloc(&h->d_V, (size_t)6 * NP));
  CHECK_RC(d.alloc(&h->d_g, (size_t)3 * NP));
  CHECK_RC(d.alloc(&h->d_scale_p, (size_t)3 * NP));
  CHECK_RC(d.alloc(&h->d_scale_c, (size_t)6 * NC));
  CHECK_RC(d.alloc(&h->d_L, (size_t)6 * NP));
  CHECK_RC(d.alloc(&h->d_q, (size_t)4 * NP));
  CHECK_RC(d.alloc(&h->d_Y, (size_t)kYRec * NE));
  const size_t npm = (size_t)kYRec * std::max(1, h->NS) * (h->any_compose ? 2 : 1);
  CHECK_RC(d.alloc(&h->d_Yp, npm));
  CHECK_RC(d.alloc(&h->d_camred, h->camred_count()));
  const size_t npart = std::max<size_t>({(size_t)h->nchunk * 27, (size_t)h->nxchunk * 36, (size_t)h->nchunk * 6, 16});
  CHECK_RC(d.alloc(&h->d_partial, npart));
  CHECK_RC(d.alloc(&h->d_xpartial, (size_t)std::max(1, h->nxchunk) * 36));
  CHECK_RC(h->sticky(h->st_yc, &h->d_yc, (size_t)6 * NC));
  CHECK_RC(d.alloc(&h->d_dp, (size_t)3 * NP));
  CHECK_RC(d.alloc(&h->d_dc, (size_t)6 * NC));
  h->red_grid = grid_for(std::max(h->NS, 3 * NP), 256, 1024);
  {
    // point-side kernel: LDS-staged camera tables when they fit (persistent grid, one
    // 1024-thread work-group per CU), else global tables (one block per slice).
    h->eval_wps = h->knobs.eval_wps != INT_MIN ? h->knobs.eval_wps : (eval_points_lds_fits(h->E) ? -2 : 4);
    int ncu = 256;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, h->device) == hipSuccess && prop.multiProcessorCount > 0)
      ncu = prop.multiProcessorCount;
    h->ncu = ncu;
    // LDS variants: one persistent work-group per CU (at most one per slice)
    // On several ranks the camera blocks' RCCL all-reduce runs during the point kernel. The
    // persistent point kernel (one 1024-thread, ~147-KB-LDS work-group per CU) would fill
    // every CU and hold the RCCL kernels off until it ends, so it leaves one CU per XCD
    // free for them (its slices are dealt round robin over whatever grid it gets).
    int pcus = ncu;
    // (a one-rank RCCL handle keeps the full grid: the same work-group partition, hence
    // bitwise the same sums, as dab_create)
    if (h->world > 1 && h->eval_wps <= 0) pcus = std::max(1, ncu - 8);
    h->eval_grid = h->eval_wps <= 0 ? std::max(1, std::min(pcus, h->nslice)) : std::max(1, h->nslice);
    h->fused = h->knobs.eval_fused != 0;
    h->fused_split = h->coll() || h->knobs.eval_split != 0;  // the split schedule on one rank too (tests)
  }
  CHECK_RC(d.alloc(&h->d_gpart, (size_t)std::max(h->red_grid, h->eval_grid) * 4));
  CHECK_RC(d.alloc(&h->d_scal, S_NSLOTS));
  CHECK_RC(h->sticky(h->st_flags, &h->d_flags, 4));
  HIP_OK(hipMemsetAsync(h->d_scal, 0, sizeof(double) * S_NSLOTS, s));  // both fixed-point cost sets start zeroed
  h->fx_last = 1;
  h->cost_fx_pending = false;
  HIP_OK(hipMemsetAsync(h->d_dc, 0, sizeof(double) * std::max(1, 6 * NC), s));
  HIP_OK(hipStreamSynchronize(s));

  DevView& v = h->view;
  v.N = h->NS;
  v.NP = NP;
  v.E = h->E;
  v.NC = NC;
  v.NI = h->NI;
  v.NE = NE;
  v.nslice = h->nslice;
  v.any_comp = h->local_compose ? 1 : 0;
  v.uni_affine = h->uni_affine;
  v.uni_ox = h->uni_ox;
  v.uni_oi = h->uni_oi;
  v.obs_idx = h->d_obs_idx;
  v.obs_xy = h->d_obs_xy;
  v.cm_idx = h->d_cm_idx;
  v.cm_xy = h->d_cm_xy;
  v.chunk_uni = h->d_chunk_uni;
  v.slice_off = h->d_slice_off;
  v.pt_ent_ptr = h->d_pt_ent_ptr;
  v.ent_os = h->d_ent_os;
  v.ent_cam = h->d_ent_cam;
  v.ent_pt = h->d_ent_pt;
  v.ent_pos = h->d_ent_pos;
  v.cm_pt = h->d_cm_pt;
  v.ext_col = h->d_ext_col;
  v.intr = h->d_intr;
  h->fused = h->fused && fused_eval_fits(v, h->nchunk, h->chunks.ngen, h->ncross, h->ncu);
  v.obs_e = nullptr;
  h->d_obs_e = nullptr;
  if (h->fused) {
    // packed 4-B slot records for the point waves (ext | intr << 16: fused_eval_fits keeps
    // E, NI <= kLdsCams)
    CHECK_RC(d.alloc(&h->d_obs_e, (size_t)std::max(1, NS)));
    su_obs_e(s, NS, h->d_obs_idx, h->d_obs_e);
    HIP_OK(hipStreamSynchronize(s));
    v.obs_e = h->d_obs_e;
  }
  HIP_OK(hipStreamSynchronize(s));
  phase("upload");
  h->have_problem = true;
  return 0;
}
// ---- set-up on the device (dab_setup.hip) ------------------------------------------------
// The same arrays as setup_host, built by rocPRIM radix sorts (stable: ties keep input
// order, exactly as the host's counting sorts) and gather / scatter kernels; only the
// camera-sized tables (chunks, cross pairs) are finished on the host. Multi-rank handles
// keep the host path: their free-camera and pair sets are unions over the ranks.
static bool setup_device_fits(dab_handle* h, const dab_problem* p) {
  if (h->world > 1) return false;
  const long long ncam = p->num_ext;  // NC <= num_ext; the pair key c0 NC + c1 must fit an int
  return ncam * ncam + 1 < (1LL << 30) && (long long)p->num_obs * 2 < (1LL << 30);
}
static int setup_device(dab_handle* h, const dab_problem* p, PhaseTimer& phase) {
  hipStream_t s = h->stream;
  Dev& d = h->dev;
  // set-up scratch: kept until the next set-up (freeing it here stalled the solve's first
  // kernels by 10-25 ms)
  Dev& tmp = h->setup_tmp;
  tmp.release();
  const int N = p->num_obs, NPT = p->num_points, E = p->num_ext;
  // scratch for rocPRIM: sized by the largest query
  void* rtmp = nullptr;
  size_t rtmp_cap = 0;
  auto rp = [&](auto call) -> int {  // query the bytes, grow the scratch, run
    size_t bytes = 0;
    if (call(nullptr, &bytes) != 0) return set_error(DAB_E_DEVICE, "rocPRIM size query failed");
    if (bytes > rtmp_cap) {
      void* q = nullptr;
      CHECK_RC(tmp.alloc(reinterpret_cast<unsigned char**>(&q), bytes));
      rtmp = q;
      rtmp_cap = bytes;
    }
    if (call(rtmp, &bytes) != 0) return set_error(DAB_E_DEVICE, "rocPRIM pass failed");
    return 0;
  };
  auto d2h = [&](void* dst, const void* src, size_t bytes) -> int {
    if (bytes) HIP_OK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s));
    return 0;
  };
  auto h2d = [&](void* dst, const void* src, size_t bytes) -> int {
    if (bytes) HIP_OK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s));
    return 0;
  };

  // ---- the caller's observation arrays ----
  int *r_pt = nullptr, *r_e0 = nullptr, *r_e1 = nullptr, *r_in = nullptr;
  double *r_xy = nullptr, *r_points = nullptr;
  CHECK_RC(tmp.alloc(&r_pt, N));
  CHECK_RC(tmp.alloc(&r_e0, N));
  CHECK_RC(tmp.alloc(&r_e1, N));
  CHECK_RC(tmp.alloc(&r_in, N));
  CHECK_RC(tmp.alloc(&r_xy, (size_t)2 * N));
  CHECK_RC(tmp.alloc(&r_points, (size_t)3 * std::max(1, NPT)));
  CHECK_RC(h2d(r_pt, p->obs_point, sizeof(int) * (size_t)N));
  CHECK_RC(h2d(r_e0, p->obs_ext0, sizeof(int) * (size_t)N));
  CHECK_RC(h2d(r_e1, p->obs_ext1, sizeof(int) * (size_t)N));
  CHECK_RC(h2d(r_in, p->obs_intr, sizeof(int) * (size_t)N));
  CHECK_RC(h2d(r_xy, p->obs_xy, sizeof(double) * 2 * (size_t)N));
  CHECK_RC(h2d(r_points, p->points, sizeof(double) * 3 * (size_t)NPT));
  phase("device: upload");

  // ---- counts, validation, referenced extrinsics ----
  int *pcount = nullptr, *eref_d = nullptr, *small = nullptr;  // small: [flags, maxcount, nref, nvalid, count, ...]
  CHECK_RC(tmp.alloc(&pcount, std::max(1, NPT)));
  CHECK_RC(tmp.alloc(&eref_d, std::max(1, E)));
  CHECK_RC(tmp.alloc(&small, 16));
  HIP_OK(hipMemsetAsync(pcount, 0, sizeof(int) * std::max(1, NPT), s));
  HIP_OK(hipMemsetAsync(eref_d, 0, sizeof(int) * std::max(1, E), s));
  HIP_OK(hipMemsetAsync(small, 0, sizeof(int) * 16, s));
  su_count(s, N, r_pt, r_e0, r_e1, r_in, NPT, E, p->num_intr, pcount, eref_d, small);
  if (NPT > 0)
    CHECK_RC(rp([&](void* t, size_t* b) { return su_max(t, b, pcount, small + 1, NPT, s); }));
  int hs[4] = {0, 0, 0, 0};
  std::vector<int> eref(std::max(1, E), 0);
  CHECK_RC(d2h(hs, small, sizeof(int) * 2));
  CHECK_RC(d2h(eref.data(), eref_d, sizeof(int) * (size_t)E));
  HIP_OK(hipStreamSynchronize(s));
  if (hs[0] & 1) {
    // the host check names the first offending observation
    CHECK_RC(validate_obs(p));
    return set_error(DAB_E_INVALID, "an observation has an out-of-range index");
  }
  h->local_compose = h->any_compose = (hs[0] & 2) != 0;
  const int maxcount = hs[1];

  // ---- device point order (count descending, stable by id) ----
  int *pk = nullptr, *pv = nullptr, *pk2 = nullptr, *pv2 = nullptr;
  CHECK_RC(tmp.alloc(&pk, std::max(1, NPT)));
  CHECK_RC(tmp.alloc(&pv, std::max(1, NPT)));
  CHECK_RC(tmp.alloc(&pk2, std::max(1, NPT)));
  CHECK_RC(tmp.alloc(&pv2, std::max(1, NPT)));
  su_point_keys(s, NPT, pcount, small + 1, pk, pv, small + 2);
  if (NPT > 0)
    CHECK_RC(rp([&](void* t, size_t* b) { return su_sort_pairs(t, b, pk, pk2, pv, pv2, NPT, bits_for(maxcount + 1), s); }));
  CHECK_RC(d2h(hs + 2, small + 2, sizeof(int)));
  HIP_OK(hipStreamSynchronize(s));
  const int NP = hs[2];
  h->NP = NP;
  h->pt_of.resize(NP);
  const int* pt_of_d = pv2;  // first NP sorted ids
  CHECK_RC(d2h(h->pt_of.data(), pt_of_d, sizeof(int) * (size_t)NP));
  int *pt_local = nullptr, *lcount = nullptr;
  CHECK_RC(tmp.alloc(&pt_local, std::max(1, NPT)));
  CHECK_RC(tmp.alloc(&lcount, NP + 1));
  su_point_local(s, NP, pt_of_d, pcount, pt_local, lcount);

  // ---- free cameras (host: E is small) ----
  h->ext_col.assign(E, -1);
  h->ext_fixed.assign(E, 0);
  h->NC = 0;
  for (int e = 0; e < E; ++e) {
    const bool is_const = p->freeze_camera || (p->ext_const && p->ext_const[e]);
    h->ext_fixed[e] = is_const;
    if (eref[e] != 0 && !is_const) h->ext_col[e] = h->NC++;
  }
  const int NC = h->NC;
  h->nplanes = h->any_compose ? 30 : 18;
  CHECK_RC(upload(&h->d_ext_col, d, h->ext_col, s));
  phase("device: points, cameras");

  // ---- observations by point (stable), SELL-64 slots ----
  int *ok = nullptr, *ov = nullptr, *ok2 = nullptr, *by_pt = nullptr, *cnt = nullptr;
  CHECK_RC(tmp.alloc(&ok, std::max(1, N)));
  CHECK_RC(tmp.alloc(&ov, std::max(1, N)));
  CHECK_RC(tmp.alloc(&ok2, std::max(1, N)));
  CHECK_RC(tmp.alloc(&by_pt, std::max(1, N)));
  CHECK_RC(tmp.alloc(&cnt, NP + 1));
  su_obs_keys(s, N, r_pt, pt_local, ok, ov);
  if (N > 0)
    CHECK_RC(rp([&](void* t, size_t* b) { return su_sort_pairs(t, b, ok, ok2, ov, by_pt, N, bits_for(NP), s); }));
  CHECK_RC(rp([&](void* t, size_t* b) { return su_exclusive_scan(t, b, lcount, cnt, NP + 1, s); }));
  h->nslice = (NP + 63) / 64;
  const int nslice = h->nslice;
  int* slen = nullptr;
  CHECK_RC(tmp.alloc(&slen, nslice + 1));
  CHECK_RC(d.alloc(&h->d_slice_off, nslice + 1));
  su_slice_len(s, nslice, NP, lcount, slen);
  CHECK_RC(rp([&](void* t, size_t* b) { return su_exclusive_scan(t, b, slen, h->d_slice_off, nslice + 1, s); }));
  int NS = 0;
  CHECK_RC(d2h(&NS, h->d_slice_off + nslice, sizeof(int)));
  HIP_OK(hipStreamSynchronize(s));
  h->NS = NS;
  int *perm_d = nullptr, *ne = nullptr;
  CHECK_RC(d.alloc(&h->d_obs_idx, (size_t)std::max(1, NS)));
  CHECK_RC(d.alloc(&h->d_obs_xy, (size_t)std::max(1, NS)));
  CHECK_RC(tmp.alloc(&perm_d, std::max(1, NS)));
  CHECK_RC(tmp.alloc(&ne, NP + 1));
  su_slots(s, NP, nslice, h->d_slice_off, cnt, lcount, by_pt, r_e0, r_e1, r_in, r_xy, h->d_ext_col, h->d_obs_idx,
           h->d_obs_xy, perm_d, ne);
  h->perm.resize(NS);
  CHECK_RC(d2h(h->perm.data(), perm_d, sizeof(int) * (size_t)NS));
  // entries (free-camera slots), point-major
  CHECK_RC(d.alloc(&h->d_pt_ent_ptr, NP + 1));
  CHECK_RC(rp([&](void* t, size_t* b) { return su_exclusive_scan(t, b, ne, h->d_pt_ent_ptr, NP + 1, s); }));
  int NE = 0;
  CHECK_RC(d2h(&NE, h->d_pt_ent_ptr + NP, sizeof(int)));
  HIP_OK(hipStreamSynchronize(s));
  h->NE = NE;
  CHECK_RC(d.alloc(&h->d_ent_os, std::max(1, NE)));
  CHECK_RC(d.alloc(&h->d_ent_cam, std::max(1, NE)));
  CHECK_RC(d.alloc(&h->d_ent_pt, std::max(1, NE)));
  su_entries(s, NP, h->d_slice_off, lcount, h->d_obs_idx, h->d_ext_col, h->d_pt_ent_ptr, h->d_ent_os, h->d_ent_cam,
             h->d_ent_pt);
  phase("device: slots, entries");

  // ---- camera-major order (entries by camera, stable) ----
  int *ek = nullptr, *ev = nullptr, *pos_cam = nullptr, *cam_ent = nullptr, *cam_cnt_d = nullptr;
  CHECK_RC(tmp.alloc(&ev, std::max(1, NE)));
  CHECK_RC(tmp.alloc(&pos_cam, std::max(1, NE)));
  CHECK_RC(tmp.alloc(&cam_ent, std::max(1, NE)));
  CHECK_RC(tmp.alloc(&cam_cnt_d, NC + 1));
  ek = h->d_ent_cam;
  su_iota(s, NE, ev);
  if (NE > 0)
    CHECK_RC(rp([&](void* t, size_t* b) { return su_sort_pairs(t, b, ek, pos_cam, ev, cam_ent, NE, bits_for(NC), s); }));
  HIP_OK(hipMemsetAsync(cam_cnt_d, 0, sizeof(int) * (NC + 1), s));
  su_bounds(s, NE, pos_cam, NC, cam_cnt_d);
  std::vector<int> cam_cnt(NC + 1, 0);
  CHECK_RC(d2h(cam_cnt.data(), cam_cnt_d, sizeof(int) * (NC + 1)));
  HIP_OK(hipStreamSynchronize(s));
  // chunks (host: NC is small)
  const int chunk = std::max(64, h->knobs.chunk > 0 ? h->knobs.chunk : kChunk);
  std::vector<int> chunk_beg, seg_chunk(NC + 1, 0);
  for (int c = 0; c < NC; ++c) {
    seg_chunk[c] = (int)chunk_beg.size();
    for (int b = cam_cnt[c]; b < cam_cnt[c + 1]; b += chunk) chunk_beg.push_back(b);
  }
  seg_chunk[NC] = (int)chunk_beg.size();
  h->nchunk = (int)chunk_beg.size();
  h->max_seg_chunks = 1;
  for (int c = 0; c < NC; ++c) h->max_seg_chunks = std::max(h->max_seg_chunks, seg_chunk[c + 1] - seg_chunk[c]);
  chunk_beg.push_back(NE);
  const int nchunk = h->nchunk;
  CHECK_RC(upload(&h->d_chunk_beg, d, chunk_beg, s));
  CHECK_RC(upload(&h->d_seg_chunk, d, seg_chunk, s));
  CHECK_RC(d.alloc(&h->d_ent_pos, std::max(1, NE)));
  CHECK_RC(d.alloc(&h->d_cm_pt, std::max(1, NE)));
  CHECK_RC(d.alloc(&h->d_cm_idx, (size_t)std::max(1, NE)));
  CHECK_RC(d.alloc(&h->d_cm_xy, (size_t)std::max(1, NE)));
  su_camera_major(s, NE, cam_ent, h->d_ent_pt, h->d_ent_os, h->d_obs_idx, h->d_obs_xy, h->d_ent_pos, h->d_cm_pt,
                  h->d_cm_idx, h->d_cm_xy);
  CHECK_RC(d.alloc(&h->d_run, std::max(1, NE)));
  su_runs(s, NE, pos_cam, h->d_cm_pt, h->d_run);
  int* run_cnt = nullptr;
  CHECK_RC(tmp.alloc(&run_cnt, nchunk + 1));
  CHECK_RC(d.alloc(&h->d_run_beg, nchunk + 1));
  HIP_OK(hipMemsetAsync(run_cnt, 0, sizeof(int) * (nchunk + 1), s));
  su_chunk_runs(s, nchunk, h->d_chunk_beg, h->d_run, run_cnt);
  CHECK_RC(rp([&](void* t, size_t* b) { return su_exclusive_scan(t, b, run_cnt, h->d_run_beg, nchunk + 1, s); }));
  int nrun = 0;
  CHECK_RC(d2h(&nrun, h->d_run_beg + nchunk, sizeof(int)));
  HIP_OK(hipStreamSynchronize(s));
  CHECK_RC(d.alloc(&h->d_run_rec, (size_t)std::max(1, nrun)));
  su_chunk_run_rec(s, nchunk, h->d_chunk_beg, h->d_run, h->d_cm_pt, pos_cam, h->d_run_beg, h->d_run_rec);
  CHECK_RC(d.alloc(&h->d_chunk_uni, (size_t)std::max(1, nchunk)));
  su_chunk_uni(s, nchunk, h->d_chunk_beg, h->d_cm_idx, kSlotBit, h->d_chunk_uni);
  std::vector<int2> chunk_uni(nchunk);
  CHECK_RC(d2h(chunk_uni.data(), h->d_chunk_uni, sizeof(int2) * (size_t)nchunk));
  HIP_OK(hipStreamSynchronize(s));
  set_uni_affine(h, chunk_uni);
  phase("device: camera-major");

  // ---- pair-major copy of the composed observations (rig) ----
  std::vector<long long> pairkeys;
  std::vector<int> pair_cnt;
  int nx = 0;
  int* xslots = nullptr;
  if (h->any_compose && NC > 0) {
    // the (c0, c1) sort key c0 * NC + c1 (and its sentinel NC * NC) is a 32-bit int
    if ((long long)NC * NC > (long long)INT_MAX)
      return set_error(DAB_E_UNSUPPORTED, "composed observations with more than 46340 free cameras");
    int *xk = nullptr, *xv = nullptr, *xk2 = nullptr;
    CHECK_RC(tmp.alloc(&xk, std::max(1, NS)));
    CHECK_RC(tmp.alloc(&xv, std::max(1, NS)));
    CHECK_RC(tmp.alloc(&xk2, std::max(1, NS)));
    CHECK_RC(tmp.alloc(&xslots, std::max(1, NS)));
    su_cross_keys(s, NS, h->d_obs_idx, h->d_ext_col, NC, xk, xv, small + 3);
    CHECK_RC(rp([&](void* t, size_t* b) { return su_sort_pairs(t, b, xk, xk2, xv, xslots, NS, bits_for((long long)NC * NC), s); }));
    CHECK_RC(d2h(hs + 3, small + 3, sizeof(int)));
    HIP_OK(hipStreamSynchronize(s));
    nx = hs[3];
    if (nx > 0) {
      int *uk = nullptr, *uc = nullptr;
      CHECK_RC(tmp.alloc(&uk, nx));
      CHECK_RC(tmp.alloc(&uc, nx));
      CHECK_RC(rp([&](void* t, size_t* b) { return su_rle(t, b, xk2, uk, uc, small + 4, nx, s); }));
      int nr = 0;
      CHECK_RC(d2h(&nr, small + 4, sizeof(int)));
      HIP_OK(hipStreamSynchronize(s));
      std::vector<int> ukh(nr), uch(nr);
      CHECK_RC(d2h(ukh.data(), uk, sizeof(int) * (size_t)nr));
      CHECK_RC(d2h(uch.data(), uc, sizeof(int) * (size_t)nr));
      HIP_OK(hipStreamSynchronize(s));
      for (int k = 0; k < nr; ++k) {
        pairkeys.push_back(ukh[k]);
        pair_cnt.push_back(uch[k]);
      }
    }
  }
  h->ncross = (int)pairkeys.size();
  std::vector<int2> cross_cam(h->ncross);
  for (int k = 0; k < h->ncross; ++k) cross_cam[k] = make_int2((int)(pairkeys[k] / NC), (int)(pairkeys[k] % NC));
  std::vector<int> xchunk_beg, xseg_chunk(h->ncross + 1, 0);
  {
    int b = 0;
    const int xchunk = std::max(64, h->knobs.xchunk > 0 ? h->knobs.xchunk : kPairChunk);
    if (PhaseTimer::on()) {  // the pair sizes the chunk plan saw
      fprintf(stderr, "pair chunks: %d pairs, most %d records per chunk, counts", h->ncross, xchunk);
      for (int k = 0; k < h->ncross; ++k) fprintf(stderr, " %d", pair_cnt[k]);
      fprintf(stderr, "\n");
    }
    for (int k = 0; k < h->ncross; ++k) {
      xseg_chunk[k] = (int)xchunk_beg.size();
      const int piece = (int)pair_piece((size_t)pair_cnt[k], xchunk);
      for (int q = b; q < b + pair_cnt[k]; q += piece) xchunk_beg.push_back(q);
      b += pair_cnt[k];
    }
    xseg_chunk[h->ncross] = (int)xchunk_beg.size();
    h->nxchunk = (int)xchunk_beg.size();
    h->max_xseg_chunks = 1;
    for (int k = 0; k < h->ncross; ++k)
      h->max_xseg_chunks = std::max(h->max_xseg_chunks, xseg_chunk[k + 1] - xseg_chunk[k]);
    xchunk_beg.push_back(nx);
  }
  CHECK_RC(d.alloc(&h->d_x_idx, (size_t)std::max(1, nx)));
  CHECK_RC(d.alloc(&h->d_x_xy, (size_t)std::max(1, nx)));
  h->pair_eval = h->nxchunk > 0 && pair_eval_fits(h->E, h->NI) && h->knobs.pair_eval != 0;
  unsigned char* touched = nullptr;
  if (h->pair_eval) {
    CHECK_RC(tmp.alloc(&touched, std::max(1, NP)));
    HIP_OK(hipMemsetAsync(touched, 0, (size_t)std::max(1, NP), s));
  }
  su_cross_copy(s, nx, xslots, h->d_obs_idx, h->d_obs_xy, h->d_x_idx, h->d_x_xy, touched);
  // per-camera CSR of cross blocks for the implicit operator: code = 2 k + (camera is c1)
  std::vector<int> xptr(NC + 1, 0), xlist;
  {
    std::vector<std::vector<int>> per(NC);
    for (int k = 0; k < h->ncross; ++k) {
      per[cross_cam[k].x].push_back(2 * k);
      per[cross_cam[k].y].push_back(2 * k + 1);
    }
    for (int c = 0; c < NC; ++c) {
      xptr[c] = (int)xlist.size();
      xlist.insert(xlist.end(), per[c].begin(), per[c].end());
    }
    if (NC > 0) xptr[NC] = (int)xlist.size();
    h->nxlist = (int)xlist.size();
  }
  std::vector<int> chunk2_beg, seg2_chunk(NC + 1, 0), xcam_ptr(NC + 1, 0), xcam_list;
  int n2 = 0;
  int* sel2 = nullptr;
  if (h->pair_eval) {
    HIP_OK(hipMemsetAsync(small + 5, 0, sizeof(int) * 3, s));
    su_count_flags(s, NP, touched, small + 5);
    su_pair_intr(s, nx, h->d_x_idx, small + 7);
    // the entries that are not paired, per camera, in camera-major order
    unsigned char* uf = nullptr;
    int *ufi = nullptr, *uscan = nullptr, *iota = nullptr, *c2cnt_d = nullptr;
    CHECK_RC(tmp.alloc(&uf, std::max(1, NE)));
    CHECK_RC(tmp.alloc(&ufi, NE + 1));
    CHECK_RC(tmp.alloc(&uscan, NE + 1));
    CHECK_RC(tmp.alloc(&iota, std::max(1, NE)));
    CHECK_RC(tmp.alloc(&sel2, std::max(1, NE)));
    CHECK_RC(tmp.alloc(&c2cnt_d, NC + 1));
    su_unpaired_flags(s, NE, h->d_cm_idx, h->d_ext_col, uf, ufi);
    CHECK_RC(rp([&](void* t, size_t* b) { return su_exclusive_scan(t, b, ufi, uscan, NE + 1, s); }));
    su_gather_at(s, NC + 1, cam_cnt_d, uscan, c2cnt_d);
    su_iota(s, NE, iota);
    if (NE > 0)
      CHECK_RC(rp([&](void* t, size_t* b) { return su_select_flagged_i(t, b, iota, uf, sel2, small + 6, NE, s); }));
    std::vector<int> c2cnt(NC + 1, 0);
    CHECK_RC(d2h(c2cnt.data(), c2cnt_d, sizeof(int) * (NC + 1)));
    int pb[3] = {0, 0, 0};
    CHECK_RC(d2h(pb, small + 5, sizeof(int) * 3));
    HIP_OK(hipStreamSynchronize(s));
    h->pair_uni_intr = pb[2] == 0;
    h->pair_bytes = (16.0 + 12.0) * (double)nx + 24.0 * (double)pb[0] + 90.0 * 8.0 * h->nxchunk;
    n2 = pb[1];
    for (int c = 0; c < NC; ++c) {
      seg2_chunk[c] = (int)chunk2_beg.size();
      for (int q = c2cnt[c]; q < c2cnt[c + 1]; q += chunk) chunk2_beg.push_back(q);
    }
    seg2_chunk[NC] = (int)chunk2_beg.size();
    h->nchunk2 = (int)chunk2_beg.size();
    chunk2_beg.push_back(n2);
    std::vector<std::vector<int>> per(NC);
    for (int k = 0; k < h->ncross; ++k)
      for (int q = xseg_chunk[k]; q < xseg_chunk[k + 1]; ++q) {
        per[cross_cam[k].x].push_back(2 * q);
        per[cross_cam[k].y].push_back(2 * q + 1);
      }
    for (int c = 0; c < NC; ++c) {
      std::sort(per[c].begin(), per[c].end());
      xcam_ptr[c] = (int)xcam_list.size();
      xcam_list.insert(xcam_list.end(), per[c].begin(), per[c].end());
    }
    xcam_ptr[NC] = (int)xcam_list.size();
  }
  phase("device: pair-major");
  reset_solver_tables(h);

  const std::vector<double> intr = device_intrinsics(h->NI, p->intr, p->intr_nf, p->intr_nk);
  std::vector<double> ext(p->ext, p->ext + 6 * (size_t)h->E);
  CHECK_RC(upload_chunk_lists(h, chunk_uni));
  CHECK_RC(upload(&h->d_xchunk_beg, d, xchunk_beg, s));
  CHECK_RC(upload(&h->d_xseg_chunk, d, xseg_chunk, s));
  CHECK_RC(upload(&h->d_cross_cam, d, cross_cam, s));
  CHECK_RC(upload(&h->d_xptr, d, xptr, s));
  CHECK_RC(upload(&h->d_xlist, d, xlist, s));
  if (h->pair_eval) {
    if (n2 > 0) {
      CHECK_RC(d.alloc(&h->d_cm2_idx, (size_t)n2));
      CHECK_RC(d.alloc(&h->d_cm2_xy, (size_t)n2));
      su_gather_cm(s, n2, sel2, h->d_cm_idx, h->d_cm_xy, h->d_cm2_idx, h->d_cm2_xy);
    }
    CHECK_RC(upload(&h->d_chunk2_beg, d, chunk2_beg, s));
    CHECK_RC(upload(&h->d_seg2_chunk, d, seg2_chunk, s));
    CHECK_RC(upload(&h->d_xcam_ptr, d, xcam_ptr, s));
    if (!xcam_list.empty()) CHECK_RC(upload(&h->d_xcam_list, d, xcam_list, s));
    CHECK_RC(d.alloc(&h->d_partial2, (size_t)std::max(1, h->nchunk2) * 27));
    CHECK_RC(d.alloc(&h->d_xcpart, (size_t)h->nxchunk * 54));
  }
  CHECK_RC(upload(&h->d_intr, d, intr, s));
  CHECK_RC(d.alloc(&h->d_points, (size_t)3 * NP));
  su_points(s, NP, pt_of_d, r_points, h->d_points);
  CHECK_RC(upload(&h->d_ext, d, ext, s));
  h->host_entries = false;  // build_schur_* fetch the entry lists from the device on first use
  HIP_OK(hipStreamSynchronize(s));
  HIP_OK(hipGetLastError());
  phase("device: tables");
  return 0;
}

static int set_problem_impl(dab_handle* h, const dab_problem* p);
// ------------------------------------------------------------------------------------
// free intrinsics: host state
// ------------------------------------------------------------------------------------
// dab_set_problem: keep the problem's intrinsics, nf / nk and which are referenced here; the
// mask goes back to all-constant (num_intr may have changed); the device buffers are lazy
// (Handle::Lazy)
static int intr_setup(dab_handle* h, const dab_problem* p) {
  const int NI = p->num_intr;
  h->intr_mask.assign((size_t)NI, 0);
  h->intr_ref.assign((size_t)NI, 0);
  h->intr_ref_union = false;
  for (int o = 0; o < p->num_obs; ++o) h->intr_ref[(size_t)p->obs_intr[o]] = 1;
  h->intr_host.assign(p->intr, p->intr + 6 * (size_t)NI);
  h->intr_nf.assign(p->intr_nf, p->intr_nf + NI);
  h->intr_nk.assign(p->intr_nk, p->intr_nk + NI);
  h->intr_meta.clear();
  h->nfi = 0;
  return 0;
}
bool dab::intr_mask_any(const dab_handle* h) {  // some group requested (and not overridden by freeze_camera)
  if (h->prob.freeze_camera) return false;
  for (uint8_t m : h->intr_mask)
    if (m) return true;
  return false;
}
static int intr_struct_bits(const dab_handle* h, int i) {  // scalars the model of intrinsic i has
  return 0x07 | (h->intr_nf[i] == 2 ? 0x08 : 0) | (h->intr_nk[i] >= 1 ? 0x10 : 0) | (h->intr_nk[i] >= 2 ? 0x20 : 0);
}
static int intr_group_bits(int groups) {
  return ((groups & DAB_INTR_CENTER) ? 0x03 : 0) | ((groups & DAB_INTR_FOCAL) ? 0x0c : 0) |
         ((groups & DAB_INTR_DISTORTION) ? 0x30 : 0);
}
// The free set of the mask now on the handle -> d_intr_meta / d_intr_act / h->nfi (uploaded
// when it changed). Collective on a multi-rank handle with a non-empty mask (the referenced
// union, once per problem). with_mask = false: the all-constant meta (parity calls).
int dab::intr_free_set(dab_handle* h, bool with_mask, int* nfi_out, int* nscal_out) {
  const int NI = h->NI;
  bool any = false;
  for (int i = 0; i < NI; ++i) any = any || h->intr_mask[(size_t)i] != 0;
  any = any && with_mask && !h->prob.freeze_camera;
  if (any && h->coll() && !h->intr_ref_union) {
    double* d_ref = nullptr;
    CHECK_RC(h->dev.alloc(&d_ref, (size_t)std::max(1, NI)));
    std::vector<double> ref((size_t)NI);
    for (int i = 0; i < NI; ++i) ref[(size_t)i] = h->intr_ref[(size_t)i];
    HIP_OK(hipMemcpyAsync(d_ref, ref.data(), sizeof(double) * NI, hipMemcpyHostToDevice, h->stream));
    HIP_OK(hipStreamSynchronize(h->stream));
    CHECK_RC(h->allreduce(d_ref, (size_t)NI, ncclMax));
    HIP_OK(hipMemcpyAsync(ref.data(), d_ref, sizeof(double) * NI, hipMemcpyDeviceToHost, h->stream));
    HIP_OK(hipStreamSynchronize(h->stream));
    for (int i = 0; i < NI; ++i) h->intr_ref[(size_t)i] = ref[(size_t)i] != 0.0;
    h->intr_ref_union = true;
    h->dev.drop(d_ref);
  }
  std::vector<int2> meta((size_t)std::max(1, NI), make_int2(-1, 0));
  int act[kIntrFreeMax] = {0};
  int nfi = 0, nscal = 0;
  for (int i = 0; i < NI; ++i) {
    const int sb = intr_struct_bits(h, i);
    const int ab = any && h->intr_ref[(size_t)i] ? (sb & intr_group_bits(h->intr_mask[(size_t)i])) : 0;
    meta[(size_t)i].y = (sb << 8) | (h->intr_nf[i] == 1 ? 1 << 16 : 0);
    if (ab == 0) continue;
    meta[(size_t)i].x = nfi;
    meta[(size_t)i].y |= ab;
    if (nfi < kIntrFreeMax) act[nfi] = ab;
    ++nfi;
    nscal += __builtin_popcount((unsigned)ab);
  }
  if (nfi_out) *nfi_out = nfi;
  if (nscal_out) *nscal_out = nscal;
  if (nfi > kIntrFreeMax) return 0;  // the caller refuses; nothing uploaded
  if (!h->lz.d_intr_meta) {
    Dev& d = h->dev;
    CHECK_RC(d.alloc(&h->lz.d_intr_meta, (size_t)std::max(1, NI)));
    CHECK_RC(d.alloc(&h->lz.d_intr_act, (size_t)kIntrFreeMax));
    CHECK_RC(d.alloc(&h->lz.d_intr_c, (size_t)kIntr * std::max(1, NI)));
    CHECK_RC(d.alloc(&h->lz.d_zg, (size_t)kIntrFreeMax * kIntrRec));
    CHECK_RC(d.alloc(&h->lz.d_sz, (size_t)6 * kIntrFreeMax));
    CHECK_RC(d.alloc(&h->lz.d_dz, (size_t)6 * kIntrFreeMax));
    CHECK_RC(d.alloc(&h->lz.d_znorm, (size_t)16));
    CHECK_RC(d.alloc(&h->lz.d_zpart, (size_t)intr_eval_grid(h->view.N) * kIntrFreeMax * kIntrRec));
    h->intr_meta.clear();
  }
  bool same = h->intr_meta.size() == meta.size();
  for (size_t i = 0; same && i < meta.size(); ++i) same = meta[i].x == h->intr_meta[i].x && meta[i].y == h->intr_meta[i].y;
  if (!same) {
    HIP_OK(hipMemcpyAsync(h->lz.d_intr_meta, meta.data(), sizeof(int2) * meta.size(), hipMemcpyHostToDevice, h->stream));
    HIP_OK(hipMemcpyAsync(h->lz.d_intr_act, act, sizeof(act), hipMemcpyHostToDevice, h->stream));
    HIP_OK(hipStreamSynchronize(h->stream));
    h->intr_meta = meta;
  }
  h->nfi = nfi;
  return 0;
}
// [U_zz | g_z | count] of the free intrinsics at the x on the handle (tables in d_camtab), all-reduced
int dab::intr_eval(dab_handle* h) {
  if (h->nfi <= 0) return 0;
  launch_intr_eval(h->stream, h->view, h->d_points, h->d_camtab, h->lz.d_intr_meta, h->nfi, h->lz.d_zpart, h->lz.d_zg);
  return h->allreduce(h->lz.d_zg, (size_t)h->nfi * kIntrRec, ncclSum);
}

extern "C" int dab_set_intrinsics_free(dab_handle* h, const uint8_t* groups) {
  clear_error();
  if (!h) return set_error(DAB_E_INVALID, "null handle");
  if (!h->have_problem) return set_error(DAB_E_STATE, "no problem set");
  if (groups)
    for (int i = 0; i < h->NI; ++i)
      if (groups[i] > 7) return set_error(DAB_E_INVALID, "intrinsic group bits above 7");
  for (int i = 0; i < h->NI; ++i) h->intr_mask[(size_t)i] = groups ? groups[i] : 0;
  return 0;
}
extern "C" int dab_get_intrinsics_free(dab_handle* h, uint8_t* groups, int32_t* num_free_intr,
                                       int32_t* num_free_scalars) {
  clear_error();
  if (!h) return set_error(DAB_E_INVALID, "null handle");
  if (!h->have_problem) return set_error(DAB_E_STATE, "no problem set");
  if (groups)
    for (int i = 0; i < h->NI; ++i) groups[i] = h->intr_mask[(size_t)i];
  if (num_free_intr || num_free_scalars) {
    int nfi = 0, nscal = 0;
    if (!intr_mask_any(h)) {
      // nothing requested (or freeze_camera): empty, no device use
    } else if (!h->coll() || h->intr_ref_union) {
      // the referenced set is known on the host: count there, the device and h->nfi untouched
      for (int i = 0; i < h->NI; ++i) {
        if (!h->intr_ref[(size_t)i]) continue;
        const int ab = intr_struct_bits(h, i) & intr_group_bits(h->intr_mask[(size_t)i]);
        nfi += ab != 0;
        nscal += __builtin_popcount((unsigned)ab);
      }
    } else {
      // several ranks, the referenced union not formed yet: the one collective of this call
      HIP_OK(hipSetDevice(h->device));
      CHECK_RC(intr_free_set(h, true, &nfi, &nscal));
    }
    if (num_free_intr) *num_free_intr = nfi;
    if (num_free_scalars) *num_free_scalars = nscal;
  }
  return 0;
}
extern "C" int dab_get_intrinsics(dab_handle* h, double* intr) {
  clear_error();
  if (!h) return set_error(DAB_E_INVALID, "null handle");
  if (!h->have_problem) return set_error(DAB_E_STATE, "no problem set");
  if (!intr) return set_error(DAB_E_INVALID, "null intrinsics array");
  HIP_OK(hipSetDevice(h->device));
  std::vector<double> K((size_t)kIntr * std::max(1, h->NI));
  HIP_OK(hipMemcpyAsync(K.data(), h->d_intr, sizeof(double) * K.size(), hipMemcpyDeviceToHost, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));
  for (int i = 0; i < h->NI; ++i) {
    const int sb = intr_struct_bits(h, i);
    for (int k = 0; k < 6; ++k)
      intr[6 * (size_t)i + k] = ((sb >> k) & 1) ? K[(size_t)kIntr * i + k] : h->intr_host[6 * (size_t)i + k];
  }
  return 0;
}
extern "C" int dab_update_intrinsics(dab_handle* h, const double* intr) {
  clear_error();
  if (!h) return set_error(DAB_E_INVALID, "null handle");
  if (!h->have_problem) return set_error(DAB_E_STATE, "no problem set");
  if (!intr) return set_error(DAB_E_INVALID, "null intrinsics array");
  HIP_OK(hipSetDevice(h->device));
  const std::vector<double> K = device_intrinsics(h->NI, intr, h->intr_nf.data(), h->intr_nk.data());
  HIP_OK(hipMemcpyAsync(h->d_intr, K.data(), sizeof(double) * K.size(), hipMemcpyHostToDevice, h->stream));
  HIP_OK(hipStreamSynchronize(h->stream));
  h->intr_host.assign(intr, intr + 6 * (size_t)h->NI);
  return 0;
}
extern "C" int dab_eval_intrinsic_jacobians(dab_handle* h, double* J) {
  clear_error();
  if (!h) return set_error(DAB_E_INVALID, "null handle");
  if (!h->have_problem) return set_error(DAB_E_STATE, "no problem set");
  if (!J) return set_error(DAB_E_INVALID, "null Jacobian array");
  HIP_OK(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  // the kernel reads only which scalars each model has: its own table, the handle's free set
  // (mask, meta, nfi) is neither read nor touched, and no rank waits for another
  std::vector<int2> meta((size_t)std::max(1, h->NI), make_int2(-1, 0));
  for (int i = 0; i < h->NI; ++i) meta[(size_t)i].y = (intr_struct_bits(h, i) << 8) | (h->intr_nf[i] == 1 ? 1 << 16 : 0);
  int2* d_meta = nullptr;
  double* d_J = nullptr;
  CHECK_RC(h->dev.alloc(&d_meta, meta.size()));
  CHECK_RC(h->dev.alloc(&d_J, (size_t)12 * std::max(1, h->NS)));
  HIP_OK(hipMemcpyAsync(d_meta, meta.data(), sizeof(int2) * meta.size(), hipMemcpyHostToDevice, s));
  launch_cam_tables(s, h->E, h->d_ext, h->d_camtab);
  launch_intr_jac(s, h->view, h->d_points, h->d_camtab, d_meta, d_J);
  std::vector<double> Jh((size_t)12 * h->NS);
  HIP_OK(hipMemcpyAsync(Jh.data(), d_J, Jh.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  h->dev.drop(d_J);
  h->dev.drop(d_meta);
  for (int s2 = 0; s2 < h->NS; ++s2) {
    const int o = h->perm[s2];
    if (o < 0) continue;
    std::memcpy(J + 12 * (size_t)o, Jh.data() + 12 * (size_t)s2, 12 * sizeof(double));
  }
  return 0;
}
extern "C" int dab_get_intrinsic_blocks(dab_handle* h, int32_t* num_free_intr, double* zg) {
  clear_error();
  if (!h) return set_error(DAB_E_INVALID, "null handle");
  if (!h->have_problem) return set_error(DAB_E_STATE, "no problem set");
  HIP_OK(hipSetDevice(h->device));
  int nfi = 0;
  CHECK_RC(intr_free_set(h, true, &nfi));
  if (nfi > kIntrFreeMax) return set_error(DAB_E_UNSUPPORTED, "more than 16 free intrinsics");
  if (num_free_intr) *num_free_intr = nfi;
  if (zg && nfi > 0) {
    std::vector<double> z((size_t)nfi * kIntrRec);
    HIP_OK(hipMemcpyAsync(z.data(), h->lz.d_zg, z.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_OK(hipStreamSynchronize(h->stream));
    for (int i = 0; i < nfi; ++i) std::memcpy(zg + 27 * (size_t)i, z.data() + (size_t)kIntrRec * i, 27 * sizeof(double));
  }
  return 0;
}

// ------------------------------------------------------------------------------------
// constant points: host state
// ------------------------------------------------------------------------------------
// The constant set of the mask on the handle (referenced here and flagged), in device point
// order, for the calls that honour it. Empty: d_ptc stays null and nothing touches the device.
int dab::pt_const_sync(dab_handle* h) {
  h->d_ptc = nullptr;
  h->n_pt_const = 0;
  if (h->pt_const.empty() || h->NP <= 0) return 0;
  std::vector<uint8_t> m((size_t)h->NP);
  int n = 0;
  for (int i = 0; i < h->NP; ++i) n += (m[(size_t)i] = h->pt_const[(size_t)h->pt_of[(size_t)i]] != 0);
  if (n == 0) return 0;
  if (!h->lz.d_pt_const) {
    CHECK_RC(h->dev.alloc(&h->lz.d_pt_const, (size_t)h->NP));
    h->pt_const_dirty = true;
  }
  if (h->pt_const_dirty) {
    HIP_OK(hipMemcpyAsync(h->lz.d_pt_const, m.data(), m.size(), hipMemcpyHostToDevice, h->stream));
    HIP_OK(hipStreamSynchronize(h->stream));  // m goes out of scope
    h->pt_const_dirty = false;
  }
  h->d_ptc = h->lz.d_pt_const;
  h->n_pt_const = n;
  return 0;
}
extern "C" int dab_set_points_constant(dab_handle* h, const uint8_t* mask) {
  clear_error();
  if (!h) return set_error(DAB_E_INVALID, "null handle");
  if (!h->have_problem) return set_error(DAB_E_STATE, "no problem set");
  const size_t n = (size_t)h->prob.num_points;
  if (mask) h->pt_const.assign(mask, mask + n);
  else h->pt_const.clear();
  h->pt_const_dirty = true;
  h->pt_prior_dirty = true;  // the effective point priors are those on non-constant points
  return 0;
}
extern "C" int dab_get_points_constant(dab_handle* h, uint8_t* mask, int32_t* num_constant) {
  clear_error();
  if (!h) return set_error(DAB_E_INVALID, "null handle");
  if (!h->have_problem) return set_error(DAB_E_STATE, "no problem set");
  const size_t n = (size_t)h->prob.num_points;
  if (mask)
    for (size_t i = 0; i < n; ++i) mask[i] = h->pt_const.empty() ? 0 : h->pt_const[i];
  if (num_constant) {
    int c = 0;
    if (!h->pt_const.empty())
      for (int i = 0; i < h->NP; ++i) c += h->pt_const[(size_t)h->pt_of[(size_t)i]] != 0;
    *num_constant = c;
  }
  return 0;
}

// ------------------------------------------------------------------------------------
// constant scalars of an extrinsic: host state
// ------------------------------------------------------------------------------------
// The effective set of the mask on the handle (bits on an extrinsic with a camera column:
// referenced on some rank, not constant, no freeze_camera), by camera column, for the calls that
// honour it. Empty: d_exs stays null and nothing touches the device.
static int ext_sub_effective(const dab_handle* h, std::vector<uint8_t>* by_col) {
  int n = 0;
  if (h->ext_sub.empty()) return 0;
  for (int e = 0; e < h->E; ++e) {
    const int c = h->ext_col[(size_t)e];
    if (c < 0) continue;
    const uint8_t b = h->ext_sub[(size_t)e] & 63;
    n += __builtin_popcount(b);
    if (by_col) (*by_col)[(size_t)c] = b;
  }
  return n;
}
int dab::ext_sub_sync(dab_handle* h) {
  h->d_exs = nullptr;
  h->n_ext_sub = 0;
  if (h->ext_sub.empty() || h->NC <= 0) return 0;
  std::vector<uint8_t> m((size_t)h->NC, 0);
  const int n = ext_sub_effective(h, &m);
  if (n == 0) return 0;
  if (!h->lz.d_ext_sub) {
    CHECK_RC(h->dev.alloc(&h->lz.d_ext_sub, (size_t)h->NC));
    h->ext_sub_dirty = true;
  }
  if (h->ext_sub_dirty) {
    HIP_OK(hipMemcpyAsync(h->lz.d_ext_sub, m.data(), m.size(), hipMemcpyHostToDevice, h->stream));
    HIP_OK(hipStreamSynchronize(h->stream));  // m goes out of scope
    h->ext_sub_dirty = false;
  }
  h->d_exs = h->lz.d_ext_sub;
  h->n_ext_sub = n;
  return 0;
}
extern "C" int dab_set_ext_scalars_constant(dab_handle* h, const uint8_t* bits) {
  clear_error();
  if (!h) return set_error(DAB_E_INVALID, "null handle");
  if (!h->have_problem) return set_error(DAB_E_STATE, "no problem set");
  const size_t n = (size_t)h->prob.num_ext;
  if (bits)
    for (size_t e = 0; e < n; ++e)
      if (bits[e] > 63) return set_error(DAB_E_INVALID, "extrinsic scalar bits above 63 (six scalars: bits 0..5)");
  if (bits) h->ext_sub.assign(bits, bits + n);
  else h->ext_sub.clear();
  h->ext_sub_dirty = true;
  return 0;
}
extern "C" int dab_get_ext_scalars_constant(dab_handle* h, uint8_t* bits, int32_t* num_constant_scalars) {
  clear_error();
  if (!h) return set_error(DAB_E_INVALID, "null handle");
  if (!h->have_problem) return set_error(DAB_E_STATE, "no problem set");
  const size_t n = (size_t)h->prob.num_ext;
  if (bits)
    for (size_t e = 0; e < n; ++e) bits[e] = h->ext_sub.empty() ? 0 : h->ext_sub[e];
  if (num_constant_scalars) *num_constant_scalars = ext_sub_effective(h, nullptr);
  return 0;
}

// ------------------------------------------------------------------------------------
// extrinsic priors: host state
// ------------------------------------------------------------------------------------
// The effective set of the priors on the handle (the extrinsic has a camera column: referenced on
// some rank, not constant, no freeze_camera), in the order set, as device records for the calls
// that honour it. Empty: n_prior stays 0 and nothing touches the device.
int dab::prior_sync(dab_handle* h) {
  h->n_prior = 0;
  std::vector<int2> idx;
  for (size_t i = 0; i < h->prior_idx.size(); ++i) {
    const int e = h->prior_idx[i];
    if (h->ext_col[(size_t)e] >= 0) idx.push_back(make_int2(e, h->ext_col[(size_t)e]));
  }
  const int n = (int)idx.size();
  if (n == 0) return 0;
  if (n > h->lz.prior_cap) {
    h->dev.drop(h->lz.d_prior_idx);
    h->dev.drop(h->lz.d_prior_rec);
    h->dev.drop(h->lz.d_prior_res);
    h->dev.drop(h->lz.d_prior_part);
    h->lz.d_prior_idx = nullptr;
    h->lz.d_prior_rec = h->lz.d_prior_res = h->lz.d_prior_part = nullptr;
    h->lz.prior_cap = 0;
    CHECK_RC(h->dev.alloc(&h->lz.d_prior_idx, (size_t)n));
    CHECK_RC(h->dev.alloc(&h->lz.d_prior_rec, (size_t)kPriorRec * n));
    CHECK_RC(h->dev.alloc(&h->lz.d_prior_res, (size_t)6 * n + 1));
    CHECK_RC(h->dev.alloc(&h->lz.d_prior_part, (size_t)2 * n));
    if (!h->lz.d_prior_cnt) CHECK_RC(h->dev.alloc(&h->lz.d_prior_cnt, (size_t)2));
    h->lz.prior_cap = n;
    h->prior_dirty = true;
  }
  if (h->prior_dirty) {
    // mean | A | A^T A (upper-packed as ug packs U), formed once here
    std::vector<double> rec((size_t)kPriorRec * n);
    int j = 0;
    for (size_t i = 0; i < h->prior_idx.size(); ++i) {
      if (h->ext_col[(size_t)h->prior_idx[i]] < 0) continue;
      double* R = rec.data() + (size_t)kPriorRec * j++;
      const double* A = h->prior_A.data() + 36 * i;
      std::memcpy(R, h->prior_mean.data() + 6 * i, 6 * sizeof(double));
      std::memcpy(R + 6, A, 36 * sizeof(double));
      int q = 42;
      for (int a = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b) {
          double t = 0.0;
          for (int r = 0; r < 6; ++r) t += A[6 * r + a] * A[6 * r + b];
          R[q++] = t;
        }
    }
    HIP_OK(hipMemcpyAsync(h->lz.d_prior_idx, idx.data(), sizeof(int2) * (size_t)n, hipMemcpyHostToDevice, h->stream));
    HIP_OK(hipMemcpyAsync(h->lz.d_prior_rec, rec.data(), sizeof(double) * rec.size(), hipMemcpyHostToDevice,
                          h->stream));
    HIP_OK(hipStreamSynchronize(h->stream));  // idx, rec go out of scope
    h->prior_dirty = false;
  }
  // the arrival count starts every call that launches the prior kernels at zero
  HIP_OK(hipMemsetAsync(h->lz.d_prior_cnt, 0, sizeof(unsigned) * 2, h->stream));
  h->n_prior = n;
  return 0;
}
extern "C" int dab_set_ext_priors(dab_handle* h, int32_t count, const int32_t* ext_index, const double* mean,
                                  const double* sqrt_info) {
  clear_error();
  if (!h) return set_error(DAB_E_INVALID, "null handle");
  if (!h->have_problem) return set_error(DAB_E_STATE, "no problem set");
  if (count < 0) return set_error(DAB_E_INVALID, "negative prior count");
  if (count > 0 && (!ext_index || !mean || !sqrt_info)) return set_error(DAB_E_INVALID, "null prior array");
  std::vector<uint8_t> seen((size_t)std::max(1, h->E), 0);
  for (int i = 0; i < count; ++i) {
    const int e = ext_index[i];
    if (e < 0 || e >= h->E) return set_error(DAB_E_INVALID, "prior on an extrinsic index out of range");
    if (seen[(size_t)e]) return set_error(DAB_E_INVALID, "two priors on one extrinsic");
    seen[(size_t)e] = 1;
  }
  for (size_t i = 0; i < (size_t)6 * count; ++i)
    if (!std::isfinite(mean[i])) return set_error(DAB_E_INVALID, "prior mean is not finite");
  for (size_t i = 0; i < (size_t)36 * count; ++i)
    if (!std::isfinite(sqrt_info[i])) return set_error(DAB_E_INVALID, "prior sqrt_info is not finite");
  h->prior_idx.assign(ext_index, ext_index + count);
  h->prior_mean.assign(mean, mean + (size_t)6 * count);
  h->prior_A.assign(sqrt_info, sqrt_info + (size_t)36 * count);
  h->prior_dirty = true;
  h->n_prior = 0;
  return 0;
}
extern "C" int dab_get_ext_priors(dab_handle* h, int32_t* count, int32_t* num_effective, int32_t* ext_index,
                                  double* mean, double* sqrt_info) {
  clear_error();
  if (!h) return set_error(DAB_E_INVALID, "null handle");
  if (!h->have_problem) return set_error(DAB_E_STATE, "no problem set");
  const size_t n = h->prior_idx.size();
  if (count) *count = (int32_t)n;
  if (num_effective) {
    int c = 0;
    for (int e : h->prior_idx) c += h->ext_col[(size_t)e] >= 0;
    *num_effective = c;
  }
  if (ext_index) std::copy(h->prior_idx.begin(), h->prior_idx.end(), ext_index);
  if (mean) std::copy(h->prior_mean.begin(), h->prior_mean.end(), mean);
  if (sqrt_info) std::copy(h->prior_A.begin(), h->prior_A.end(), sqrt_info);
  return 0;
}
extern "C" int dab_eval_ext_priors(dab_handle* h, double* residuals, double* cost) {
  clear_error();
  if (!h) return set_error(DAB_E_INVALID, "null handle");
  if (!h->have_problem) return set_error(DAB_E_STATE, "no problem set");
  HIP_OK(hipSetDevice(h->device));
  CHECK_RC(prior_sync(h));
  const int n = h->n_prior;
  std::vector<double> res((size_t)6 * n + 1, 0.0);
  if (n > 0) {
    launch_prior_eval(h->stream, n, h->lz.d_prior_idx, h->lz.d_prior_rec, h->d_ext, h->lz.d_prior_res);
    HIP_OK(hipMemcpyAsync(res.data(), h->lz.d_prior_res, sizeof(double) * res.size(), hipMemcpyDeviceToHost,
                          h->stream));
    HIP_OK(hipStreamSynchronize(h->stream));
  }
  if (residuals) {  // as set: an ignored prior's row is zero
    int j = 0;
    for (size_t i = 0; i < h->prior_idx.size(); ++i) {
      const bool eff = h->ext_col[(size_t)h->prior_idx[i]] >= 0;
      for (int k = 0; k < 6; ++k) residuals[6 * i + k] = eff ? res[(size_t)6 * j + k] : 0.0;
      j += eff;
    }
  }
  if (cost) *cost = res[(size_t)6 * n];
  return guard_fail(h, "dab_eval_ext_priors");
}

// ------------------------------------------------------------------------------------
// point priors: host state
// ------------------------------------------------------------------------------------
// Per prior as set: its device point when it is effective (the point is referenced on this rank
// and not constant), else -1.
static void pt_prior_device_points(const dab_handle* h, std::vector<int>* dev) {
  dev->assign(h->pt_prior_idx.size(), -1);
  if (h->pt_prior_idx.empty() || h->NP <= 0) return;
  std::vector<int> local((size_t)h->prob.num_points, -1);
  for (int l = 0; l < h->NP; ++l) local[(size_t)h->pt_of[(size_t)l]] = l;
  for (size_t i = 0; i < h->pt_prior_idx.size(); ++i) {
    const size_t p = (size_t)h->pt_prior_idx[i];
    if (local[p] >= 0 && (h->pt_const.empty() || h->pt_const[p] == 0)) (*dev)[i] = local[p];
  }
}
// This rank's effective set in device point order, as device records for the calls that honour
// it: idx and the planar records [kPtPriorRec][n], A^T A formed once here, uploaded only when the
// priors, the constant mask or the problem changed. Empty: n_pt_prior stays 0 and nothing touches
// the device.
int dab::pt_prior_sync(dab_handle* h) {
  h->n_pt_prior = 0;
  if (h->pt_prior_idx.empty() || h->NP <= 0) return 0;
  if (h->pt_prior_dirty) {
    std::vector<int> dev;
    pt_prior_device_points(h, &dev);
    std::vector<std::pair<int, int>> order;  // (device point, prior as set)
    for (size_t i = 0; i < dev.size(); ++i)
      if (dev[i] >= 0) order.emplace_back(dev[i], (int)i);
    std::sort(order.begin(), order.end());
    const int n = (int)order.size();
    h->pt_prior_pos.assign(dev.size(), -1);
    for (int j = 0; j < n; ++j) h->pt_prior_pos[(size_t)order[(size_t)j].second] = j;
    if (n > h->lz.ptp_cap) {
      h->dev.drop(h->lz.d_ptp_idx);
      h->dev.drop(h->lz.d_ptp_rec);
      h->dev.drop(h->lz.d_ptp_res);
      h->dev.drop(h->lz.d_ptp_part);
      h->lz.d_ptp_idx = nullptr;
      h->lz.d_ptp_rec = h->lz.d_ptp_res = h->lz.d_ptp_part = nullptr;
      h->lz.ptp_cap = 0;
      CHECK_RC(h->dev.alloc(&h->lz.d_ptp_idx, (size_t)n));
      CHECK_RC(h->dev.alloc(&h->lz.d_ptp_rec, (size_t)kPtPriorRec * n));
      CHECK_RC(h->dev.alloc(&h->lz.d_ptp_res, (size_t)3 * n + 1));
      CHECK_RC(h->dev.alloc(&h->lz.d_ptp_part, (size_t)2 * pt_prior_groups(n)));
      if (!h->lz.d_ptp_cnt) CHECK_RC(h->dev.alloc(&h->lz.d_ptp_cnt, (size_t)2));
      h->lz.ptp_cap = n;
    }
    if (n > 0) {
      std::vector<int> idx((size_t)n);
      std::vector<double> rec((size_t)kPtPriorRec * n);
      const size_t ns = (size_t)n;
      for (size_t j = 0; j < ns; ++j) {
        idx[j] = order[j].first;
        const size_t i = (size_t)order[j].second;
        const double* A = h->pt_prior_A.data() + 9 * i;
        for (int k = 0; k < 3; ++k) rec[k * ns + j] = h->pt_prior_mean[3 * i + k];
        for (int k = 0; k < 9; ++k) rec[(3 + k) * ns + j] = A[k];
        int q = 12;  // (0,0) (0,1) (0,2) (1,1) (1,2) (2,2), as V
        for (int a = 0; a < 3; ++a)
          for (int b = a; b < 3; ++b) {
            double t = 0.0;
            for (int r = 0; r < 3; ++r) t += A[3 * r + a] * A[3 * r + b];
            rec[(size_t)(q++) * ns + j] = t;
          }
      }
      HIP_OK(hipMemcpyAsync(h->lz.d_ptp_idx, idx.data(), sizeof(int) * ns, hipMemcpyHostToDevice, h->stream));
      HIP_OK(hipMemcpyAsync(h->lz.d_ptp_rec, rec.data(), sizeof(double) * rec.size(), hipMemcpyHostToDevice,
                            h->stream));
      HIP_OK(hipStreamSynchronize(h->stream));  // idx, rec go out of scope
    }
    h->pt_prior_n = n;
    h->pt_prior_dirty = false;
  }
  if (h->pt_prior_n == 0) return 0;
  // the arrival count starts every call that launches the point-prior kernels at zero
  HIP_OK(hipMemsetAsync(h->lz.d_ptp_cnt, 0, sizeof(unsigned) * 2, h->stream));
  h->n_pt_prior = h->pt_prior_n;
  return 0;
}
int dab::call_state(dab_handle* h, int* points_state) {
  double st[2] = {h->NP - h->n_pt_const > 0 ? 2.0 : (h->n_pt_const > 0 ? 1.0 : 0.0), h->n_pt_prior > 0 ? 1.0 : 0.0};
  if (h->coll()) {
    hipStream_t s = h->stream;
    h->h_scal[S_SYNC] = st[0];
    h->h_scal[S_SYNC1] = st[1];
    HIP_OK(hipMemcpyAsync(h->d_scal + S_SYNC, &h->h_scal[S_SYNC], 2 * sizeof(double), hipMemcpyHostToDevice, s));
    CHECK_RC(h->allreduce(h->d_scal + S_SYNC, 2, ncclMax));
    HIP_OK(hipMemcpyAsync(&h->h_scal[S_SYNC], h->d_scal + S_SYNC, 2 * sizeof(double), hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    st[0] = h->h_scal[S_SYNC];
    st[1] = h->h_scal[S_SYNC1];
  }
  if (points_state) *points_state = (int)st[0];
  h->pt_prior_any = st[1] > 0.0;
  return 0;
}
extern "C" int dab_set_point_priors(dab_handle* h, int32_t count, const int32_t* point_index, const double* mean,
                                    const double* sqrt_info) {
  clear_error();
  if (!h) return set_error(DAB_E_INVALID, "null handle");
  if (!h->have_problem) return set_error(DAB_E_STATE, "no problem set");
  if (count < 0) return set_error(DAB_E_INVALID, "negative prior count");
  if (count > 0 && (!point_index || !mean || !sqrt_info)) return set_error(DAB_E_INVALID, "null prior array");
  const int npts = h->prob.num_points;
  std::vector<uint8_t> seen((size_t)std::max(1, npts), 0);
  for (int i = 0; i < count; ++i) {
    const int p = point_index[i];
    if (p < 0 || p >= npts) return set_error(DAB_E_INVALID, "prior on a point index out of range");
    if (seen[(size_t)p]) return set_error(DAB_E_INVALID, "two priors on one point");
    seen[(size_t)p] = 1;
  }
  for (size_t i = 0; i < (size_t)3 * count; ++i)
    if (!std::isfinite(mean[i])) return set_error(DAB_E_INVALID, "prior mean is not finite");
  for (size_t i = 0; i < (size_t)9 * count; ++i)
    if (!std::isfinite(sqrt_info[i])) return set_error(DAB_E_INVALID, "prior sqrt_info is not finite");
  h->pt_prior_idx.assign(point_index, point_index + count);
  h->pt_prior_mean.assign(mean, mean + (size_t)3 * count);
  h->pt_prior_A.assign(sqrt_info, sqrt_info + (size_t)9 * count);
  h->pt_prior_dirty = true;
  h->n_pt_prior = 0;
  h->pt_prior_any = false;
  return 0;
}
extern "C" int dab_get_point_priors(dab_handle* h, int32_t* count, int32_t* num_effective, int32_t* point_index,
                                    double* mean, double* sqrt_info) {
  clear_error();
  if (!h) return set_error(DAB_E_INVALID, "null handle");
  if (!h->have_problem) return set_error(DAB_E_STATE, "no problem set");
  if (count) *count = (int32_t)h->pt_prior_idx.size();
  if (num_effective) {
    std::vector<int> dev;
    pt_prior_device_points(h, &dev);
    int c = 0;
    for (int d : dev) c += d >= 0;
    *num_effective = c;
  }
  if (point_index) std::copy(h->pt_prior_idx.begin(), h->pt_prior_idx.end(), point_index);
  if (mean) std::copy(h->pt_prior_mean.begin(), h->pt_prior_mean.end(), mean);
  if (sqrt_info) std::copy(h->pt_prior_A.begin(), h->pt_prior_A.end(), sqrt_info);
  return 0;
}
extern "C" int dab_eval_point_priors(dab_handle* h, double* residuals, double* cost) {
  clear_error();
  if (!h) return set_error(DAB_E_INVALID, "null handle");
  if (!h->have_problem) return set_error(DAB_E_STATE, "no problem set");
  HIP_OK(hipSetDevice(h->device));
  CHECK_RC(pt_prior_sync(h));  // this rank's: the call is not collective
  const int n = h->n_pt_prior;
  std::vector<double> res((size_t)3 * n + 1, 0.0);
  if (n > 0) {
    launch_pt_prior_eval(h->stream, n, h->lz.d_ptp_idx, h->lz.d_ptp_rec, h->d_points, h->lz.d_ptp_res);
    HIP_OK(hipMemcpyAsync(res.data(), h->lz.d_ptp_res, sizeof(double) * res.size(), hipMemcpyDeviceToHost,
                          h->stream));
    HIP_OK(hipStreamSynchronize(h->stream));
  }
  if (residuals) {  // as set: an ignored prior's row is zero
    for (size_t i = 0; i < h->pt_prior_idx.size(); ++i) {
      const int j = n > 0 ? h->pt_prior_pos[i] : -1;
      for (int k = 0; k < 3; ++k) residuals[3 * i + k] = j >= 0 ? res[(size_t)3 * j + k] : 0.0;
    }
  }
  if (cost) *cost = res[(size_t)3 * n];
  return guard_fail(h, "dab_eval_point_priors");
}

// ------------------------------------------------------------------------------------
// intrinsic priors: host state
// ------------------------------------------------------------------------------------
// The effective set of the priors on the handle for the free set now on it (h->intr_meta, nfi of
// them: the intrinsic is referenced on some rank, has an active scalar, no freeze_camera), sorted
// by free column so that the order of setting cannot show, as device records: the inactive columns
// of A and the inactive entries of the mean are zeroed here, A^T A is formed from the zeroed A.
// Uploaded only when the records differ from the ones on the device. Empty: n_zprior stays 0 and
// nothing touches the device.
int dab::zprior_sync(dab_handle* h, int nfi) {
  h->n_zprior = 0;
  h->zprior_pos.assign(h->zprior_idx.size(), -1);
  if (h->zprior_idx.empty() || nfi <= 0 || nfi > kIntrFreeMax) return 0;
  std::vector<std::pair<int, int>> order;  // (free column, prior as set)
  for (size_t i = 0; i < h->zprior_idx.size(); ++i) {
    const int2 mt = h->intr_meta[(size_t)h->zprior_idx[i]];
    if (mt.x >= 0) order.emplace_back(mt.x, (int)i);
  }
  std::sort(order.begin(), order.end());
  const int n = (int)order.size();
  if (n == 0) return 0;
  std::vector<int2> idx((size_t)n);
  std::vector<double> rec((size_t)kPriorRec * n, 0.0);
  for (int j = 0; j < n; ++j) {
    const size_t i = (size_t)order[(size_t)j].second;
    const int ii = h->zprior_idx[i];
    const int act = h->intr_meta[(size_t)ii].y & 63;
    h->zprior_pos[i] = j;
    idx[(size_t)j] = make_int2(ii, order[(size_t)j].first);
    double* R = rec.data() + (size_t)kPriorRec * j;
    double* A = R + 6;
    for (int k = 0; k < 6; ++k) {
      if (!((act >> k) & 1)) continue;
      R[k] = h->zprior_mean[6 * i + k];
      for (int r = 0; r < 6; ++r) A[6 * r + k] = h->zprior_A[36 * i + 6 * r + k];
    }
    int q = 42;
    for (int a = 0; a < 6; ++a)
      for (int b = a; b < 6; ++b) {
        double t = 0.0;
        for (int r = 0; r < 6; ++r) t += A[6 * r + a] * A[6 * r + b];
        R[q++] = t;
      }
  }
  if (!h->lz.d_zp_idx) {
    CHECK_RC(h->dev.alloc(&h->lz.d_zp_idx, (size_t)kIntrFreeMax));
    CHECK_RC(h->dev.alloc(&h->lz.d_zp_rec, (size_t)kPriorRec * kIntrFreeMax));
    CHECK_RC(h->dev.alloc(&h->lz.d_zp_res, (size_t)6 * kIntrFreeMax + 1));
    h->zprior_dev_idx.clear();
    h->zprior_dev_rec.clear();
  }
  bool same = h->zprior_dev_idx.size() == idx.size() && h->zprior_dev_rec.size() == rec.size() &&
              std::memcmp(h->zprior_dev_rec.data(), rec.data(), sizeof(double) * rec.size()) == 0;
  for (size_t j = 0; same && j < idx.size(); ++j)
    same = idx[j].x == h->zprior_dev_idx[j].x && idx[j].y == h->zprior_dev_idx[j].y;
  if (!same) {
    HIP_OK(hipMemcpyAsync(h->lz.d_zp_idx, idx.data(), sizeof(int2) * idx.size(), hipMemcpyHostToDevice, h->stream));
    HIP_OK(hipMemcpyAsync(h->lz.d_zp_rec, rec.data(), sizeof(double) * rec.size(), hipMemcpyHostToDevice, h->stream));
    HIP_OK(hipStreamSynchronize(h->stream));  // idx, rec are pageable
    h->zprior_dev_idx = idx;
    h->zprior_dev_rec = rec;
  }
  h->n_zprior = n;
  return 0;
}
void dab::zprior_blocks(dab_handle* h) {
  launch_zprior_blocks(h->stream, h->n_zprior, h->lz.d_zp_idx, h->lz.d_zp_rec, h->d_intr, h->lz.d_zg,
                       h->d_scal + S_ZPRIOR);
}
extern "C" int dab_set_intr_priors(dab_handle* h, int32_t count, const int32_t* intr_index, const double* mean,
                                   const double* sqrt_info) {
  clear_error();
  if (!h) return set_error(DAB_E_INVALID, "null handle");
  if (!h->have_problem) return set_error(DAB_E_STATE, "no problem set");
  if (count < 0) return set_error(DAB_E_INVALID, "negative prior count");
  if (count > 0 && (!intr_index || !mean || !sqrt_info)) return set_error(DAB_E_INVALID, "null prior array");
  std::vector<uint8_t> seen((size_t)std::max(1, h->NI), 0);
  for (int i = 0; i < count; ++i) {
    const int k = intr_index[i];
    if (k < 0 || k >= h->NI) return set_error(DAB_E_INVALID, "prior on an intrinsic index out of range");
    if (seen[(size_t)k]) return set_error(DAB_E_INVALID, "two priors on one intrinsic");
    seen[(size_t)k] = 1;
  }
  for (size_t i = 0; i < (size_t)6 * count; ++i)
    if (!std::isfinite(mean[i])) return set_error(DAB_E_INVALID, "prior mean is not finite");
  for (size_t i = 0; i < (size_t)36 * count; ++i)
    if (!std::isfinite(sqrt_info[i])) return set_error(DAB_E_INVALID, "prior sqrt_info is not finite");
  h->zprior_idx.assign(intr_index, intr_index + count);
  h->zprior_mean.assign(mean, mean + (size_t)6 * count);
  h->zprior_A.assign(sqrt_info, sqrt_info + (size_t)36 * count);
  h->zprior_pos.assign((size_t)count, -1);
  h->n_zprior = 0;
  return 0;
}
extern "C" int dab_get_intr_priors(dab_handle* h, int32_t* count, int32_t* num_effective, int32_t* intr_index,
                                   double* mean, double* sqrt_info) {
  clear_error();
  if (!h) return set_error(DAB_E_INVALID, "null handle");
  if (!h->have_problem) return set_error(DAB_E_STATE, "no problem set");
  if (count) *count = (int32_t)h->zprior_idx.size();
  if (num_effective) {
    int c = 0;
    if (h->zprior_idx.empty() || !intr_mask_any(h)) {
      // no prior, or nothing free (freeze_camera too): empty, no device use
    } else {
      if (h->coll() && !h->intr_ref_union) {
        // several ranks, the referenced union not formed yet: the one collective of this call
        HIP_OK(hipSetDevice(h->device));
        CHECK_RC(intr_free_set(h, true, nullptr));
      }
      for (int i : h->zprior_idx)
        c += h->intr_ref[(size_t)i] && (intr_struct_bits(h, i) & intr_group_bits(h->intr_mask[(size_t)i])) != 0;
    }
    *num_effective = c;
  }
  if (intr_index) std::copy(h->zprior_idx.begin(), h->zprior_idx.end(), intr_index);
  if (mean) std::copy(h->zprior_mean.begin(), h->zprior_mean.end(), mean);
  if (sqrt_info) std::copy(h->zprior_A.begin(), h->zprior_A.end(), sqrt_info);
  return 0;
}
extern "C" int dab_eval_intr_priors(dab_handle* h, double* residuals, double* cost) {
  clear_error();
  if (!h) return set_error(DAB_E_INVALID, "null handle");
  if (!h->have_problem) return set_error(DAB_E_STATE, "no problem set");
  HIP_OK(hipSetDevice(h->device));
  int nfi = 0;
  if (!h->zprior_idx.empty() && intr_mask_any(h)) {
    CHECK_RC(intr_free_set(h, true, &nfi));
    if (nfi > kIntrFreeMax) return set_error(DAB_E_UNSUPPORTED, "more than 16 free intrinsics");
  }
  CHECK_RC(zprior_sync(h, nfi));
  const int n = h->n_zprior;
  std::vector<double> res((size_t)6 * n + 1, 0.0);
  if (n > 0) {
    launch_zprior_eval(h->stream, n, h->lz.d_zp_idx, h->lz.d_zp_rec, h->d_intr, h->lz.d_zp_res);
    HIP_OK(hipMemcpyAsync(res.data(), h->lz.d_zp_res, sizeof(double) * res.size(), hipMemcpyDeviceToHost, h->stream));
    HIP_OK(hipStreamSynchronize(h->stream));
  }
  if (residuals) {  // as set: an ignored prior's row is zero
    for (size_t i = 0; i < h->zprior_idx.size(); ++i) {
      const int j = h->zprior_pos[i];
      for (int k = 0; k < 6; ++k) residuals[6 * i + k] = j >= 0 ? res[(size_t)6 * j + k] : 0.0;
    }
  }
  if (cost) *cost = res[(size_t)6 * n];
  return guard_fail(h, "dab_eval_intr_priors");
}

extern "C" int dab_set_problem(dab_handle* h, const dab_problem* p) {
  const int rc = set_problem_impl(h, p);
  CHECK_RC(guard_fail(h, "dab_set_problem"));
  return rc;
}
static int set_problem_impl(dab_handle* h, const dab_problem* p) {
  clear_error();
  if (!h) return set_error(DAB_E_INVALID, "null handle");
  CHECK_RC(validate(p));
  HIP_OK(hipSetDevice(h->device));
  HIP_OK(hipStreamSynchronize(h->stream));
  h->dev.drop(h->lz.d_covZ);  // n x n: back to the device, not into the pool
  h->dev.drop(h->lz.d_covZz);
  h->dev.release();
  // the lazily allocated buffers went with the release: the next use allocates again (a stale
  // pointer would be written after its memory was freed)
  h->lz = dab_handle::Lazy{};
  h->have_problem = false;
  h->prob = *p;
  h->pt_const.clear();  // all free again (num_points may have changed)
  h->pt_const_dirty = true;
  h->d_ptc = nullptr;
  h->n_pt_const = 0;
  h->ext_sub.clear();  // every scalar free again (num_ext may have changed)
  h->ext_sub_dirty = true;
  h->d_exs = nullptr;
  h->n_ext_sub = 0;
  h->prior_idx.clear();  // no priors (num_ext may have changed)
  h->prior_mean.clear();
  h->prior_A.clear();
  h->prior_dirty = true;
  h->n_prior = 0;
  h->pt_prior_idx.clear();  // no point priors (num_points may have changed)
  h->pt_prior_mean.clear();
  h->pt_prior_A.clear();
  h->pt_prior_pos.clear();
  h->pt_prior_dirty = true;
  h->pt_prior_n = h->n_pt_prior = 0;
  h->pt_prior_any = false;
  h->zprior_idx.clear();  // no intrinsic priors (num_intr may have changed)
  h->zprior_mean.clear();
  h->zprior_A.clear();
  h->zprior_pos.clear();
  h->zprior_dev_idx.clear();  // lz went with the release
  h->zprior_dev_rec.clear();
  h->n_zprior = 0;
  PhaseTimer phase{"set_problem %-22s %8.1f ms\n"};  // the host preprocessing's phases
  const int N = p->num_obs;
  h->N = N;
  h->E = p->num_ext;
  h->NI = p->num_intr;

  const bool on_device = h->knobs.setup_host == 0 && setup_device_fits(h, p);
  if (on_device) CHECK_RC(setup_device(h, p, phase));
  else CHECK_RC(setup_host(h, p, phase));
  CHECK_RC(setup_buffers(h, phase));
  return intr_setup(h, p);
}
