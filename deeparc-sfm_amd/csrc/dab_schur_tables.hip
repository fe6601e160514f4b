// dab_schur_tables.hip — what the linear solvers need besides the problem's own tables, built
// on the first solve that asks: the explicit step's tile or pair tables (build_schur_tables)
// and the implicit-Schur PCG's buffers (build_pcg_buffers).
#include <iterator>

#include "dab_handle.h"

using namespace dab;

// Explicit-Schur tables (DAB_LINEAR_SOLVER_EXPLICIT_SCHUR only), built on first use:
// every ordered pair (e, f) of entries of one point with cam(e) >= cam(f) contributes
// -Y_e Y_f^T to lower block (cam(e), cam(f)) of the reduced camera system S. Pairs are
// sorted by block so each block is one deterministic segment. The block table is the
// union over ranks so the all-reduced packed layout matches.
static constexpr long long kMaxExplicitPairs = 200000000LL;
static int max_all_ranks(dab_handle* h, double& x) {  // max over ranks of one host scalar
  if (!h->coll()) return 0;
  hipStream_t s = h->stream;
  double* d_f = nullptr;
  CHECK_RC(h->dev.alloc(&d_f, 1));
  HIP_OK(hipMemcpyAsync(d_f, &x, sizeof(double), hipMemcpyHostToDevice, s));
  CHECK_RC(h->allreduce(d_f, 1, ncclMax));
  HIP_OK(hipMemcpyAsync(&x, d_f, sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  return 0;
}

// Explicit S by block tiles (k_schur_y + k_schur_tiles) when the camera set is small (the
// matrix-free criterion: tables in LDS, NC <= 160) and no point sees more than kTileMaxRec
// free cameras. Tables: each point's entries sorted by camera, records (distinct point-camera
// pairs), batches of whole points (<= 640 records, <= 64 points), tiles of <= 1024 blocks.
static constexpr int kBatchPts = 64, kTileBlocks = 1024;
// the entry lists on the host (the explicit-step table builders read them); the device
// set-up leaves them on the device until a builder asks
// The tile tables (k_schur_y / k_schur_tiles): per point its entries sorted by (camera,
// slot) (sch), one record per distinct (point, camera) ordered (batch, camera, point), batch
// headers, and the blocks' owners. On the device (dab_setup.hip, 19) unless the host entry
// lists are resident (DAB_SETUP_HOST=1: the host reference path); bitwise the same tables.
// d_sch / d_m: the device per-point sort (su_tile_sort) when on the device.
static int build_schur_tiles(dab_handle* h, int2* d_sch, const int* d_m) {
  hipStream_t s = h->stream;
  PhaseTimer phase{"schur_tiles %-22s %8.1f ms\n"};
  const int NP = h->NP, NC = h->NC;
  const bool on_device = d_sch != nullptr;
  Dev& d = h->dev;
  const bool single = h->knobs.tile_single != 0;
  const int cap = schur_tile_batch_cap(NC, single);
  const int hdr_bytes = schur_tile_hdr_bytes(NC);
  const int nb = (int)tri_n(NC);
  std::vector<int> rec_ptr(NP + 1, 0);
  std::vector<int> batch_rec{0}, batch_pt{0};
  // batches of whole points: <= kBatchPts points (one mask word) and <= cap records
  auto cut_batches = [&]() {
    int cur = 0, curp = 0;
    for (int p = 0; p < NP; ++p) {
      const int m = rec_ptr[p + 1] - rec_ptr[p];
      if (curp > 0 && (cur + m > cap || curp + 1 > kBatchPts)) {
        batch_rec.push_back(rec_ptr[p]);
        batch_pt.push_back(p);
        cur = curp = 0;
      }
      cur += m;
      curp += 1;
    }
    batch_rec.push_back(rec_ptr[NP]);
    batch_pt.push_back(NP);
  };
  std::vector<long long> hits(std::max(1, nb), 0);
  int nbatch = 0, nrec = 0;
  int *d_br = nullptr, *d_bp = nullptr;
  unsigned char* d_hdr = nullptr;
  int4 *d_rec = nullptr, *d_robs = nullptr;
  if (on_device) {
    {
      std::vector<int> m(NP);
      if (NP > 0) HIP_OK(hipMemcpyAsync(m.data(), d_m, sizeof(int) * (size_t)NP, hipMemcpyDeviceToHost, s));
      HIP_OK(hipStreamSynchronize(s));
      for (int p = 0; p < NP; ++p) rec_ptr[p + 1] = rec_ptr[p] + m[p];
    }
    cut_batches();
    nbatch = (int)batch_rec.size() - 1;
    nrec = rec_ptr[NP];
    phase("device sort, batches");
    CHECK_RC(upload(&d_br, d, batch_rec, s));
    CHECK_RC(upload(&d_bp, d, batch_pt, s));
    CHECK_RC(d.alloc(&d_hdr, (size_t)std::max(1, nbatch) * hdr_bytes));
    CHECK_RC(d.alloc(&d_rec, (size_t)std::max(1, nrec)));
    CHECK_RC(d.alloc(&d_robs, (size_t)std::max(1, nrec)));
    HIP_OK(hipMemsetAsync(d_hdr, 0, (size_t)std::max(1, nbatch) * hdr_bytes, s));
    su_tile_batch(s, nbatch, NC, d_bp, d_br, h->d_pt_ent_ptr, d_sch, h->d_obs_idx, hdr_bytes, d_hdr, d_rec, d_robs);
    int* d_hits = nullptr;
    CHECK_RC(h->setup_tmp.alloc(&d_hits, (size_t)std::max(1, nb)));
    HIP_OK(hipMemsetAsync(d_hits, 0, sizeof(int) * (size_t)std::max(1, nb), s));
    su_tile_hits(s, NP, nb, h->d_pt_ent_ptr, d_sch, d_hits);
    std::vector<int> hi(std::max(1, nb));
    HIP_OK(hipMemcpyAsync(hi.data(), d_hits, sizeof(int) * (size_t)std::max(1, nb), hipMemcpyDeviceToHost, s));
    HIP_OK(hipStreamSynchronize(s));
    for (int k = 0; k < nb; ++k) hits[k] = hi[k];
    phase("device records, hits");
  } else {
    const std::vector<int>& pt_ent_ptr = h->h_pt_ent_ptr;
    const big_vec<int>& ent_cam = h->h_ent_cam;
    const big_vec<int>& ent_os = h->h_ent_os;
    big_vec<int2> sch(h->NE);
    // per point (threads): entries sorted by (camera, slot), distinct cameras counted
    par_for(NP, [&](long long pb, long long pe, int) {
      for (int p = (int)pb; p < (int)pe; ++p) {
        const int b = pt_ent_ptr[p], e = pt_ent_ptr[p + 1];
        for (int i = b; i < e; ++i) sch[i] = make_int2(ent_os[i], ent_cam[i]);
        std::sort(sch.begin() + b, sch.begin() + e, [](const int2& x, const int2& y) {
          return x.y != y.y ? x.y < y.y : x.x < y.x;
        });
        int m = 0;
        for (int i = b; i < e; ++i) m += (i == b || sch[i].y != sch[i - 1].y);
        rec_ptr[p + 1] = m;
      }
    }, 2048);
    for (int p = 0; p < NP; ++p) rec_ptr[p + 1] += rec_ptr[p];
    nrec = rec_ptr[NP];
    phase("sort entries");
    cut_batches();
    nbatch = (int)batch_rec.size() - 1;
    // records ordered (batch, camera, point) and the batch headers: mask[NC] | off[NC + 1]
    big_vec<int4> rec(nrec), robs(nrec);
    std::vector<unsigned char> hdr((size_t)nbatch * hdr_bytes, 0);
    par_for(nbatch, [&](long long bb, long long be, int) {
      std::vector<int> pos(NC + 1);
      for (int b = (int)bb; b < (int)be; ++b) {
        unsigned long long* mask = reinterpret_cast<unsigned long long*>(&hdr[(size_t)b * hdr_bytes]);
        int* off = reinterpret_cast<int*>(&hdr[(size_t)b * hdr_bytes + 8 * (size_t)NC]);
        for (int p = batch_pt[b]; p < batch_pt[b + 1]; ++p)
          for (int i = pt_ent_ptr[p]; i < pt_ent_ptr[p + 1]; ++i)
            if (i == pt_ent_ptr[p] || sch[i].y != sch[i - 1].y) {
              off[sch[i].y + 1]++;
              mask[sch[i].y] |= 1ull << (p - batch_pt[b]);
            }
        for (int c = 0; c < NC; ++c) off[c + 1] += off[c];
        for (int c = 0; c <= NC; ++c) pos[c] = off[c];
        for (int p = batch_pt[b]; p < batch_pt[b + 1]; ++p) {
          int r = -1;
          for (int i = pt_ent_ptr[p]; i < pt_ent_ptr[p + 1]; ++i) {
            if (i > pt_ent_ptr[p] && sch[i].y == sch[i - 1].y) {
              rec[r].y++;
              continue;
            }
            r = batch_rec[b] + pos[sch[i].y]++;
            rec[r] = make_int4(i, 1, p, sch[i].y);
            const int o = h->perm[sch[i].x >> 1];  // the caller's observation of the slot
            robs[r] = make_int4(sch[i].x, h->prob.obs_ext0[o], h->prob.obs_ext1[o], h->prob.obs_intr[o]);
          }
        }
      }
    }, 16);
    phase("records, headers");
    // hit counts of every block from a sample of the points (every 4th): the points that see
    // both of its cameras
    std::vector<std::vector<long long>> th(setup_threads(), std::vector<long long>(std::max(1, nb), 0));
    par_for(NP, [&](long long pb, long long pe, int t) {
      std::vector<int> cams;
      for (int p = (int)pb; p < (int)pe; ++p) {
        if (p % 4) continue;
        cams.clear();
        for (int i = pt_ent_ptr[p]; i < pt_ent_ptr[p + 1]; ++i)
          if (i == pt_ent_ptr[p] || sch[i].y != sch[i - 1].y) cams.push_back(sch[i].y);
        for (size_t x = 0; x < cams.size(); ++x)  // ascending: block (cams[x], cams[y <= x])
          for (size_t y = 0; y <= x; ++y) th[t][tri_n(cams[x]) + cams[y]]++;
      }
    });
    for (auto& v : th)
      for (int k = 0; k < nb; ++k) hits[k] += v[k];
    CHECK_RC(upload(&d_br, d, batch_rec, s));
    CHECK_RC(upload(&d_hdr, d, hdr, s));
    CHECK_RC(upload(&d_sch, d, sch, s));
    CHECK_RC(upload(&d_rec, d, rec, s));
    CHECK_RC(upload(&d_robs, d, robs, s));
    phase("hits, upload");
  }
  // tiles: equal block ranges of <= kTileBlocks (rows up to the tile's last camera)
  const int ntile = std::max(1, (nb + kTileBlocks - 1) / kTileBlocks);
  std::vector<int> tb(ntile + 1), clast(ntile);
  for (int t = 0; t <= ntile; ++t) tb[t] = (int)((long long)nb * t / ntile);
  // slots: per tile, blocks by hit count (descending); thread i owns the i-th heaviest and
  // the (1023 - i)-th, so the pairs' sums are even and a wave's threads have similar work
  std::vector<int> slot((size_t)ntile * 2 * kTileThreads, -1);
  for (int t = 0; t < ntile; ++t) {
    std::vector<int> bl;
    for (int k = tb[t]; k < tb[t + 1]; ++k) bl.push_back(k);
    std::stable_sort(bl.begin(), bl.end(), [&](int x, int y) { return hits[x] > hits[y]; });
    for (int i = 0; i < (int)bl.size(); ++i) {
      const int th2 = i < kTileThreads ? i : 2 * kTileThreads - 1 - i;
      slot[(size_t)t * 2 * kTileThreads + (i < kTileThreads ? 0 : kTileThreads) + th2] = bl[i];
    }
    int c = 0;
    while (tri_n(c + 1) <= tb[t + 1] - 1) ++c;
    clast[t] = c;
  }
  phase("slots");
  SchurTiles& a = h->tiles;
  a.ntile = ntile;
  a.nbatch = nbatch;
  a.nrec = nrec;
  // load balance: a tile's time is its busiest wave's, summed over its batches, and the
  // tiles differ (C5: the arc rows' tile ~2x the others), so a heavy tile's batches go to
  // several work-groups per group. Parts per tile from the sampled hits (the tile's work):
  // the split that minimises max_t(hits_t / sub_t) / groups, groups = CUs / sum(sub)
  // (multiples of 8: one XCD per group). DAB_TILE_BALANCE=0 keeps one part per tile.
  std::vector<int> sub(ntile, 1);
  {
    std::vector<double> w(ntile, 0.0);
    for (int t = 0; t < ntile; ++t)
      for (int k = tb[t]; k < tb[t + 1]; ++k) w[t] += (double)hits[k] + 1.0;
    auto groups_for = [&](int nsub) {
      int ng = std::max(1, h->ncu / nsub);
      if (ng >= 8) ng -= ng % 8;
      return ng;
    };
    auto cost = [&](const std::vector<int>& sb) {
      int ns = 0;
      double m = 0.0;
      for (int t = 0; t < ntile; ++t) {
        ns += sb[t];
        m = std::max(m, w[t] / sb[t]);
      }
      return m / groups_for(ns);
    };
    if (h->knobs.tile_balance != 0 && ntile > 1 && ntile <= 6) {
      std::vector<int> cur(ntile, 1), best = cur;
      double bc = cost(cur);
      for (;;) {  // odometer over sub_t in 1..4
        int t = 0;
        while (t < ntile && cur[t] == 4) cur[t++] = 1;
        if (t == ntile) break;
        ++cur[t];
        const double c = cost(cur);
        if (c < bc * (1.0 - 1e-12)) {
          bc = c;
          best = cur;
        }
      }
      sub = best;
    }
  }
  std::vector<int> subbeg(ntile + 1, 0);
  for (int t = 0; t < ntile; ++t) subbeg[t + 1] = subbeg[t] + sub[t];
  a.nsub = subbeg[ntile];
  int ng = std::max(1, h->ncu / a.nsub);
  if (ng >= 8) ng -= ng % 8;
  // at least tile_minb batches per work-group (small problems keep few partials for the sum):
  // 2 since round 6 — C1's 313 batches on 156 work-groups instead of 39, k_schur_tiles
  // 153 -> 57 us, its partial sum 7 -> 15 us (scripts/runs/r06h.sh)
  const int smax = *std::max_element(sub.begin(), sub.end());
  a.ngroup = std::max(1, std::min(ng, a.nbatch / (std::max(1, h->knobs.tile_minb) * smax)));
  std::vector<int> blk_nslot(std::max(1, nb), a.ngroup);
  for (int t = 0; t < ntile; ++t)
    for (int k = tb[t]; k < tb[t + 1]; ++k) blk_nslot[k] = a.ngroup * sub[t];
  a.nelem = 36 * nb;
  a.stride = (size_t)a.nelem;
  a.kq = 0;
  a.batch_cap = cap;
  a.single = single ? 1 : 0;
  a.hdr_bytes = hdr_bytes;
  int *d_cl = nullptr, *d_slot = nullptr;
  CHECK_RC(upload(&d_cl, d, clast, s));
  CHECK_RC(upload(&d_slot, d, slot, s));
  a.rec_obs = d_robs;
  a.batch_rec = d_br;
  a.tile_clast = d_cl;
  a.tile_slot = d_slot;
  a.hdr = d_hdr;
  a.sch_ent = d_sch;
  a.rec_info = d_rec;
  CHECK_RC(d.alloc(&h->d_kx, (size_t)6 * NC));
  a.kx = h->d_kx;
  CHECK_RC(d.alloc(&a.partial, (size_t)a.ngroup * smax * a.stride));
  int *d_sub = nullptr, *d_subbeg = nullptr, *d_nslot = nullptr;
  CHECK_RC(upload(&d_sub, d, sub, s));
  CHECK_RC(upload(&d_subbeg, d, subbeg, s));
  CHECK_RC(upload(&d_nslot, d, blk_nslot, s));
  a.tile_sub = d_sub;
  a.tile_subbeg = d_subbeg;
  a.blk_nslot = d_nslot;
  CHECK_RC(d.alloc(&h->d_sblk, a.stride));
  CHECK_RC(d.alloc(&h->d_rfx, (size_t)6 * NC));
  CHECK_RC(d.alloc(&h->d_yrec, (size_t)18 * std::max(1, a.nrec)));
  HIP_OK(hipStreamSynchronize(s));
  phase("upload, alloc");
  return 0;
}

// present block keys: the union over ranks (every rank must all-reduce the same S layout)
static int union_block_keys(dab_handle* h, std::vector<long long>& keys) {
  if (!h->coll()) return 0;
  const int NC = h->NC;
  hipStream_t s = h->stream;
  std::vector<double> bm((size_t)NC * NC, 0.0);
  for (long long k : keys) bm[(size_t)k] = 1.0;
  double* d_bm = nullptr;
  CHECK_RC(h->dev.alloc(&d_bm, bm.size()));
  HIP_OK(hipMemcpyAsync(d_bm, bm.data(), bm.size() * sizeof(double), hipMemcpyHostToDevice, s));
  CHECK_RC(h->allreduce(d_bm, bm.size(), ncclMax));
  HIP_OK(hipMemcpyAsync(bm.data(), d_bm, bm.size() * sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  keys.clear();
  for (size_t i = 0; i < bm.size(); ++i)
    if (bm[i] != 0.0) keys.push_back((long long)i);
  return 0;
}

// Pair tables on the device (dab_setup.hip, 18): h->d_pairs in sorted (key, e, f) order;
// pk / pbeg: the present keys (increasing) and their first pair; np2 pairs
static int build_schur_pairs_device(dab_handle* h, std::vector<long long>& pk, std::vector<int>& pbeg,
                                    long long& np2) {
  hipStream_t s = h->stream;
  const int NP = h->NP, NC = h->NC;
  // block key c0 * NC + c1 is a 32-bit int (a dense S that large would not fit anyway)
  if ((long long)NC * NC > (long long)INT_MAX)
    return set_error(DAB_E_UNSUPPORTED, "explicit Schur pair tables for more than 46340 free cameras");
  Dev& tmp = h->setup_tmp;  // released at the next set-up
  void* rtmp = nullptr;
  size_t rtmp_cap = 0;
  auto rp = [&](auto call) -> int {
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
  int* cnt = nullptr;
  unsigned long long* tot = nullptr;
  CHECK_RC(tmp.alloc(&cnt, (size_t)NP + 1));
  CHECK_RC(tmp.alloc(&tot, 1));
  HIP_OK(hipMemsetAsync(tot, 0, sizeof(unsigned long long), s));
  HIP_OK(hipMemsetAsync(cnt + NP, 0, sizeof(int), s));
  su_pair_count(s, NP, h->d_pt_ent_ptr, h->d_ent_cam, cnt, tot);
  unsigned long long total = 0;
  HIP_OK(hipMemcpyAsync(&total, tot, sizeof(total), hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  double flag = NC > 0 && (long long)total > kMaxExplicitPairs ? 1.0 : 0.0;
  CHECK_RC(max_all_ranks(h, flag));  // every rank must take the same branch
  if (flag != 0.0)
    return set_error(DAB_E_UNSUPPORTED,
                     "reduced camera system too large for explicit Schur pair tables (" + std::to_string(total) +
                         " pairs); use DAB_LINEAR_SOLVER_IMPLICIT_SCHUR_PCG");
  np2 = NC > 0 ? (long long)total : 0;
  const int n = (int)np2;
  pk.clear();
  pbeg.clear();
  CHECK_RC(h->dev.alloc(&h->d_pairs, (size_t)std::max(1, n)));
  if (n == 0) return 0;
  int *poff = nullptr, *k1 = nullptr, *v1 = nullptr, *k2 = nullptr, *v2 = nullptr, *uk = nullptr, *uc = nullptr,
      *nr = nullptr;
  int2* ef = nullptr;
  CHECK_RC(tmp.alloc(&poff, (size_t)NP + 1));
  CHECK_RC(tmp.alloc(&k1, (size_t)n));
  CHECK_RC(tmp.alloc(&v1, (size_t)n));
  CHECK_RC(tmp.alloc(&k2, (size_t)n));
  CHECK_RC(tmp.alloc(&v2, (size_t)n));
  CHECK_RC(tmp.alloc(&ef, (size_t)n));
  CHECK_RC(rp([&](void* t, size_t* b) { return su_exclusive_scan(t, b, cnt, poff, NP + 1, s); }));
  su_pair_gen(s, NP, h->d_pt_ent_ptr, h->d_ent_cam, poff, NC, k1, v1, ef);
  CHECK_RC(rp([&](void* t, size_t* b) { return su_sort_pairs(t, b, k1, k2, v1, v2, n, bits_for(NC * NC), s); }));
  su_pair_gather(s, n, v2, ef, h->d_ent_pos, h->d_pairs);
  // present keys and their run lengths
  uk = k1;  // the unsorted keys are no longer needed
  uc = v1;
  CHECK_RC(tmp.alloc(&nr, 1));
  CHECK_RC(rp([&](void* t, size_t* b) { return su_rle(t, b, k2, uk, uc, nr, n, s); }));
  int nruns = 0;
  HIP_OK(hipMemcpyAsync(&nruns, nr, sizeof(int), hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  std::vector<int> ukh(nruns), uch(nruns);
  HIP_OK(hipMemcpyAsync(ukh.data(), uk, sizeof(int) * (size_t)nruns, hipMemcpyDeviceToHost, s));
  HIP_OK(hipMemcpyAsync(uch.data(), uc, sizeof(int) * (size_t)nruns, hipMemcpyDeviceToHost, s));
  HIP_OK(hipStreamSynchronize(s));
  pk.resize(nruns);
  pbeg.resize(nruns);
  int acc = 0;
  for (int i = 0; i < nruns; ++i) {
    pk[i] = ukh[i];
    pbeg[i] = acc;
    acc += uch[i];
  }
  return 0;
}

int dab::build_schur_tables(dab_handle* h) {
  if (h->schur_built) return 0;
  PhaseTimer phase{"schur_tables %-21s %8.1f ms\n"};
  struct Report {  // the whole build, on every way out
    double t0;
    ~Report() {
      if (PhaseTimer::on()) fprintf(stderr, "build_schur_tables %8.1f ms\n", 1e3 * (now_s() - t0));
    }
  } report{phase.t};
  hipStream_t s = h->stream;
  const int NP = h->NP, NC = h->NC;
  const std::vector<int>& pt_ent_ptr = h->h_pt_ent_ptr;
  const big_vec<int>& ent_cam = h->h_ent_cam;
  const big_vec<int>& ent_pos = h->h_ent_pos;
  int2* tile_sch = nullptr;
  int* tile_m = nullptr;
  int dev_maxm = 0;
  {
    // tile mode: every rank must take the same branch (the all-reduced S layouts differ).
    // The host entry lists are needed by the tile tables (and by the host reference path of
    // the pair tables); large camera sets with device set-up never fetch them.
    const bool tiles_possible = h->knobs.schur_tiles != 0 && NC > 0 && mf_schur_fits(NC, h->E, h->NI);
    if (tiles_possible && !h->host_entries) {
      // device: per point entries sorted by (camera, slot), distinct cameras counted
      CHECK_RC(h->dev.alloc(&tile_sch, (size_t)std::max(1, h->NE)));
      CHECK_RC(h->setup_tmp.alloc(&tile_m, (size_t)std::max(1, NP)));
      su_tile_sort(s, NP, h->d_pt_ent_ptr, h->d_ent_cam, h->d_ent_os, tile_sch, tile_m);
      if (NP > 0) {
        int* d_max = nullptr;
        CHECK_RC(h->setup_tmp.alloc(&d_max, 1));
        size_t bytes = 0;
        if (su_max(nullptr, &bytes, tile_m, d_max, NP, s) != 0) return set_error(DAB_E_DEVICE, "rocPRIM size query failed");
        unsigned char* t = nullptr;
        CHECK_RC(h->setup_tmp.alloc(&t, std::max<size_t>(1, bytes)));
        if (su_max(t, &bytes, tile_m, d_max, NP, s) != 0) return set_error(DAB_E_DEVICE, "rocPRIM pass failed");
        HIP_OK(hipMemcpyAsync(&dev_maxm, d_max, sizeof(int), hipMemcpyDeviceToHost, s));
        HIP_OK(hipStreamSynchronize(s));
      }
    }
    std::vector<int> tmax(setup_threads(), 0);  // distinct free cameras of one point
    if (tiles_possible && h->host_entries) par_for(NP, [&](long long pb, long long pe, int t) {
      std::vector<int> seen(std::max(1, NC), -1);
      for (int pt = (int)pb; pt < (int)pe; ++pt) {
        int m = 0;
        for (int e = pt_ent_ptr[pt]; e < pt_ent_ptr[pt + 1]; ++e)
          if (seen[ent_cam[e]] != pt) {
            seen[ent_cam[e]] = pt;
            ++m;
          }
        tmax[t] = std::max(tmax[t], m);
      }
    });
    const int maxm = std::max(dev_maxm, *std::max_element(tmax.begin(), tmax.end()));
    phase("camera counts");
    double no_tiles = (tiles_possible && maxm <= kTileMaxRec) ? 0.0 : 1.0;
    CHECK_RC(max_all_ranks(h, no_tiles));
    h->schur_tiles = no_tiles == 0.0;
  }
  if (h->schur_tiles) {
    CHECK_RC(build_schur_tiles(h, tile_sch, tile_m));
    phase.t = now_s();
    h->nblk = 0;
    h->nzero = 0;
    h->npairs = 0;
    CHECK_RC(h->dev.alloc(&h->d_spack, h->spack_count()));  // ybc only
    phase("tiles: spack alloc");
    const int n = 6 * NC;
    h->lds = ((n + 1 + 7) / 8) * 8;
    if (h->lds % 512 == 0) h->lds += 8;
    CHECK_RC(h->sticky(h->st_S, &h->d_S, (size_t)(n + 1) * h->lds));
    h->mf_grid_n = mf_grid(h->NP, h->ncu);
    phase("tiles: S alloc");
    h->schur_built = true;
    return 0;
  }
  // reduced-camera-system blocks: ordered entry pairs (e, f) of one point with
  // cam(e) >= cam(f); block (cam(e), cam(f)) of the lower triangle of S.
  std::vector<long long> blkkeys;
  std::vector<int2> pairs;
  std::vector<int> blk_pair_beg;
  const bool on_device = !h->host_entries;
  // the present keys with their first pair, in increasing key order, and the number of pairs
  std::vector<long long> pk;
  std::vector<int> pbeg;
  long long np2 = 0;
  if (on_device) {
    // device: count, scan, generate, stable radix sort by block key, gather (bitwise the
    // host path's tables; the pairs stay on the device)
    CHECK_RC(build_schur_pairs_device(h, pk, pbeg, np2));
    phase("pairs on device");
  } else {
    long long total = 0;
    for (int pt = 0; pt < NP; ++pt) {
      const long long m = pt_ent_ptr[pt + 1] - pt_ent_ptr[pt];
      total += m * (m + 1) / 2 + m;  // upper bound
    }
    double flag = total > kMaxExplicitPairs ? 1.0 : 0.0;
    CHECK_RC(max_all_ranks(h, flag));  // every rank must take the same branch
    if (flag != 0.0)
      return set_error(DAB_E_UNSUPPORTED,
                       "reduced camera system too large for explicit Schur pair tables (" +
                           std::to_string(total) + " pairs); use DAB_LINEAR_SOLVER_IMPLICIT_SCHUR_PCG");
  }
  if (!on_device && NC > 0) {
    // pairs generated per point in parallel, in (e, f) order (entries are point-major, so
    // that is the global (e, f) order), then a stable counting sort by block key: the
    // (key, e, f) order of the former comparison sort (~0.4 s at C3), bitwise the same tables
    std::vector<long long> poff((size_t)NP + 1, 0);
    par_for(NP, [&](long long pb, long long pe, int) {
      for (int pt = (int)pb; pt < (int)pe; ++pt) {
        long long c = 0;
        for (int e = pt_ent_ptr[pt]; e < pt_ent_ptr[pt + 1]; ++e)
          for (int f = pt_ent_ptr[pt]; f < pt_ent_ptr[pt + 1]; ++f) c += ent_cam[e] >= ent_cam[f];
        poff[pt + 1] = c;
      }
    }, 4096);
    for (int pt = 0; pt < NP; ++pt) poff[pt + 1] += poff[pt];
    np2 = poff[NP];
    big_vec<long long> pkey((size_t)np2);  // c0 * NC + c1 in 64 bits
    big_vec<int2> pef((size_t)np2);
    par_for(NP, [&](long long pb, long long pe, int) {
      for (int pt = (int)pb; pt < (int)pe; ++pt) {
        long long o = poff[pt];
        for (int e = pt_ent_ptr[pt]; e < pt_ent_ptr[pt + 1]; ++e)
          for (int f = pt_ent_ptr[pt]; f < pt_ent_ptr[pt + 1]; ++f) {
            const int ce = ent_cam[e], cf = ent_cam[f];
            if (ce < cf) continue;
            pkey[o] = (long long)ce * NC + cf;
            pef[o] = make_int2(e, f);
            ++o;
          }
      }
    }, 4096);
    // two stable counting passes (by cf, then by ce: memory O(threads x NC), not NC^2)
    phase("pairs generated");
    big_vec<int> o1, o2;
    std::vector<long long> st1, st2;
    bucket_sort(np2, NC, [&](long long i) { return (int)(pkey[i] % NC); }, o1, st1);
    bucket_sort(np2, NC, [&](long long j) { return (int)(pkey[o1[j]] / NC); }, o2, st2);
    pairs.resize((size_t)np2);
    big_vec<long long> skey((size_t)np2);
    par_for(np2, [&](long long pb, long long pe, int) {
      for (long long i = pb; i < pe; ++i) {
        const int q = o1[o2[i]];
        const int2 ef = pef[q];
        pairs[i] = make_int2(ent_pos[ef.x], ent_pos[ef.y]);  // Y records are camera-major
        skey[i] = pkey[q];
      }
    });
    phase("pairs sorted");
    pk.reserve((size_t)NC * 64);
    pbeg.reserve((size_t)NC * 64);
    for (long long i = 0; i < np2; ++i)
      if (i == 0 || skey[i] != skey[i - 1]) {
        pk.push_back(skey[i]);
        pbeg.push_back((int)i);
      }
  }
  if (on_device || NC > 0) {
    // diagonal blocks always exist; union across ranks
    std::vector<long long> diag((size_t)NC), keys;
    for (int c = 0; c < NC; ++c) diag[c] = (long long)c * NC + c;
    keys.reserve(pk.size() + diag.size());
    std::merge(pk.begin(), pk.end(), diag.begin(), diag.end(), std::back_inserter(keys));  // both sorted
    keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    CHECK_RC(union_block_keys(h, keys));
    blkkeys = keys;
    blk_pair_beg.assign(blkkeys.size() + 1, 0);
    size_t j = 0;  // blocks without local pairs start where the next present key does
    for (size_t b2 = 0; b2 < blkkeys.size(); ++b2) {
      while (j < pk.size() && pk[j] < blkkeys[b2]) ++j;
      blk_pair_beg[b2] = j < pk.size() ? pbeg[j] : (int)np2;
    }
    blk_pair_beg[blkkeys.size()] = (int)np2;
  } else {
    blk_pair_beg.assign(1, 0);
  }
  phase("block keys");
  h->nblk = (int)blkkeys.size();
  h->npairs = np2;
  std::vector<int2> blk_cam(h->nblk);
  for (int b = 0; b < h->nblk; ++b) blk_cam[b] = make_int2((int)(blkkeys[b] / NC), (int)(blkkeys[b] % NC));

  // the lower blocks no pair reaches (blkkeys is sorted): zeroed per step on one rank, where
  // the blocks are written into S directly
  std::vector<int2> blk_zero;
  {
    size_t j = 0;
    for (int c = 0; c < NC; ++c)
      for (int d2 = 0; d2 <= c; ++d2) {
        const long long key = (long long)c * NC + d2;
        while (j < blkkeys.size() && blkkeys[j] < key) ++j;
        if (j >= blkkeys.size() || blkkeys[j] != key) blk_zero.push_back(make_int2(c, d2));
      }
  }
  h->nzero = (int)blk_zero.size();

  Dev& d = h->dev;
  if (!on_device) CHECK_RC(upload(&h->d_pairs, d, pairs, s));
  CHECK_RC(upload(&h->d_blk_cam, d, blk_cam, s));
  if (h->nzero > 0) CHECK_RC(upload(&h->d_blk_zero, d, blk_zero, s));
  CHECK_RC(upload(&h->d_blk_pair_beg, d, blk_pair_beg, s));
  CHECK_RC(d.alloc(&h->d_spack, h->spack_count()));
  const int n = 6 * NC;
  h->lds = ((n + 1 + 7) / 8) * 8;
  if (h->lds % 512 == 0) h->lds += 8;  // avoid power-of-two row strides
  CHECK_RC(h->sticky(h->st_S, &h->d_S, NC > 0 ? (size_t)(n + 1) * h->lds : 1));
  // Y as [NE][18] records for k_s_blocks (allocated here so that an OOM surfaces before
  // iteration 0, not mid-solve)
  if (NC > 0) CHECK_RC(d.alloc(&h->lz.d_Yrec, (size_t)kYRec * std::max(1, h->NE)));
  HIP_OK(hipStreamSynchronize(s));
  phase("upload, alloc");
  h->schur_built = true;
  return 0;
}

// Implicit-Schur PCG buffers (DAB_LINEAR_SOLVER_IMPLICIT_SCHUR_PCG), allocated on first use.
int dab::build_pcg_buffers(dab_handle* h) {
  if (h->pcg_built) return 0;
  Dev& d = h->dev;
  const size_t n = (size_t)6 * h->NC;
  for (double** b : {&h->d_pcg_b, &h->d_pcg_r, &h->d_pcg_z, &h->d_pcg_p, &h->d_pcg_q, &h->d_pcg_w})
    CHECK_RC(d.alloc(b, n));
  CHECK_RC(d.alloc(&h->d_pcg_Ad, 6 * n));
  CHECK_RC(d.alloc(&h->d_pcg_Minv, 6 * n));
  CHECK_RC(d.alloc(&h->d_pcg_red, (size_t)27 * h->NC));
  CHECK_RC(d.alloc(&h->d_pcg_t, (size_t)4 * h->NP));
  CHECK_RC(d.alloc(&h->d_pcg_state, 1));
  CHECK_RC(d.alloc(&h->d_cg_partial, (size_t)cg_partial_size(h->NC)));
  CHECK_RC(d.alloc(&h->d_cg_cnt, 1));
  HIP_OK(hipMemsetAsync(h->d_cg_cnt, 0, sizeof(unsigned), h->stream));
  // the single-pass matvec when the camera system is small (DAB_PCG_FUSED=0 disables it)
  h->mf = mf_schur_fits(h->NC, h->E, h->NI) && h->NP > 0 && h->knobs.pcg_mf != 0;
  if (h->mf) {
    h->mf_grid_n = mf_grid(h->NP, h->ncu);
    CHECK_RC(d.alloc(&h->d_mf_partial, (size_t)h->mf_grid_n * 6 * h->NC));
  }
  h->fused_grid = 0;
  if (pcg_fused_fits(h->NC) && h->NP > 0 && h->knobs.pcg_fused != 0) {
    h->fused_grid = pcg_fused_grid(h->NP, h->ncu);
    CHECK_RC(d.alloc(&h->d_fused_partial, (size_t)h->fused_grid * 6 * h->NC));
  }
  if (!h->h_pcg_state && !(h->h_pcg_state = static_cast<PcgState*>(pinned_take(sizeof(PcgState)))))
    return set_error(DAB_E_NOMEM, "pinned PCG state allocation failed");
  h->pcg_built = true;
  return 0;
}
