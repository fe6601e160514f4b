// dab_handle.hip — the handle's lifecycle: the stream / pinned-memory caches, dab_create*,
// the peer-to-peer all-reduce set-up, dab_destroy, the device guard's check, the parameter
// upload / download and the schedule queries.
#include <map>
#include <mutex>

#include "dab_handle.h"
#include "dab_warm.h"

using namespace dab;

namespace dab {
namespace {
std::mutex& cache_mu() {
  static std::mutex* m = new std::mutex();  // never destroyed: handles may outlive static teardown
  return *m;
}
std::map<int, std::vector<hipStream_t>>& stream_cache() {
  static auto* c = new std::map<int, std::vector<hipStream_t>>();
  return *c;
}
std::map<size_t, std::vector<void*>>& pinned_cache() {
  static auto* c = new std::map<size_t, std::vector<void*>>();
  return *c;
}
}  // namespace
hipStream_t stream_take(int device) {
  {
    std::lock_guard<std::mutex> lk(cache_mu());
    auto& v = stream_cache()[device];
    while (!v.empty()) {
      hipStream_t s = v.back();
      v.pop_back();
      const hipError_t q = hipStreamQuery(s);  // a stream left in an error state is not reused
      if (q == hipSuccess || q == hipErrorNotReady) return s;
      (void)hipGetLastError();
      (void)hipStreamDestroy(s);
    }
  }
  hipStream_t s = nullptr;
  if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return nullptr;
  return s;
}
void stream_give(int device, hipStream_t s) {
  if (!s) return;
  if (hipStreamSynchronize(s) != hipSuccess) {  // a stream in an error state is not reused
    (void)hipStreamDestroy(s);
    return;
  }
  std::lock_guard<std::mutex> lk(cache_mu());
  stream_cache()[device].push_back(s);
}
void* pinned_take(size_t bytes) {
  {
    std::lock_guard<std::mutex> lk(cache_mu());
    auto& v = pinned_cache()[bytes];
    if (!v.empty()) {
      void* p = v.back();
      v.pop_back();
      return p;
    }
  }
  void* p = nullptr;
  if (hipHostMalloc(&p, bytes) != hipSuccess) return nullptr;
  return p;
}
void pinned_give(void* p, size_t bytes) {
  if (!p) return;
  std::lock_guard<std::mutex> lk(cache_mu());
  pinned_cache()[bytes].push_back(p);
}
WarmTable& warm_table() {
  static WarmTable t = {};
  return t;
}
}  // namespace dab

extern "C" int dab_release_caches(void) {
  std::lock_guard<std::mutex> lk(dab::cache_mu());
  // only idle cached objects live here (a handle takes its streams out of the cache and
  // gives them back on destroy), so live handles are unaffected; each device's streams are
  // destroyed with that device current
  int cur = 0;
  const bool have_cur = hipGetDevice(&cur) == hipSuccess;
  for (auto& kv : dab::stream_cache()) {
    if (kv.second.empty()) continue;
    (void)hipSetDevice(kv.first);
    for (hipStream_t s : kv.second) (void)hipStreamDestroy(s);
  }
  if (have_cur) (void)hipSetDevice(cur);
  dab::stream_cache().clear();
  for (auto& kv : dab::pinned_cache())
    for (void* p : kv.second) (void)hipHostFree(p);
  dab::pinned_cache().clear();
  return 0;
}

// ------------------------------------------------------------------------------------
// lifecycle
// ------------------------------------------------------------------------------------
static int create_common(int device, dab_handle** out) {
  if (!out) return set_error(DAB_E_INVALID, "null handle pointer");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return set_error(DAB_E_DEVICE, "no HIP device available");
  if (device < 0 || device >= ndev) return set_error(DAB_E_INVALID, "device ordinal out of range");
  HIP_OK(hipSetDevice(device));
  // Host waits spin (the solver's host round trips are latency-critical: read_scalars every
  // LM iteration). With the runtime's default the waits after a burst of short kernels
  // (the device set-up) fell back to blocking, and the first synchronisation of the
  // following solve took 10-25 ms for 10 us of device work. DAB_SCHEDULE_BLOCKING=1 keeps
  // the default.
  // The flag is process-wide (every host wait of the embedding process spins): dab.h says so.
  // A runtime that refuses it (flags fixed once the device's context exists) keeps its
  // default; that is reported once on stderr, not as an error.
  if (!getenv("DAB_SCHEDULE_BLOCKING")) {
    const hipError_t fe = hipSetDeviceFlags(hipDeviceScheduleSpin);
    static bool warned = false;
    if (fe != hipSuccess && !warned) {
      warned = true;
      fprintf(stderr, "dab: hipSetDeviceFlags(hipDeviceScheduleSpin) not applied (%s); host waits keep the "
                      "runtime's scheduling\n", hipGetErrorString(fe));
    }
  }
  PhaseTimer phase{"create %-24s %.2f ms\n"};
  dab_handle* h = new dab_handle();
  h->device = device;
  h->knobs.read();
  if (!(h->stream = stream_take(device))) {
    delete h;
    return set_error(DAB_E_DEVICE, "hipStreamCreate failed");
  }
  phase("stream");
  h->chol = chol_create();
  phase("Cholesky context");
  if (!h->chol) {
    delete h;
    return set_error(DAB_E_DEVICE, "Cholesky context creation failed");
  }
  // an allocation that fails in one allocator first empties the others' idle pools
  h->keep_dev.donors = {&h->dev, &h->setup_tmp};
  chol_mem(h->chol)->donors = {&h->dev, &h->setup_tmp};
  h->dev.donors = {&h->setup_tmp};
  if (hipEventCreate(&h->ev0) != hipSuccess || hipEventCreate(&h->ev1) != hipSuccess ||
      hipEventCreate(&h->ev2) != hipSuccess || hipEventCreate(&h->ev3) != hipSuccess ||
      hipEventCreateWithFlags(&h->ev_cam, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&h->ev_comm, hipEventDisableTiming) != hipSuccess ||
      !(h->comm_stream = stream_take(device))) {
    delete h;
    return set_error(DAB_E_DEVICE, "hipEventCreate failed");
  }
  if (!(h->h_scal = static_cast<double*>(pinned_take(sizeof(double) * S_NSLOTS))) ||
      !(h->h_flags = static_cast<int*>(pinned_take(sizeof(int) * 4)))) {
    delete h;
    return set_error(DAB_E_NOMEM, "hipHostMalloc failed");
  }
  phase("events, pinned");
  // every code object of the library loaded on this device now, once per process (the first
  // kernel launch of a translation unit would otherwise pay for it mid-solve)
  static bool warmed[64] = {};
  if (device < 64 && !warmed[device]) {
    const WarmTable& t = warm_table();
    if (t.n > kWarmMax) {
      delete h;
      return set_error(DAB_E_STATE, "code-object warm-up table full: raise kWarmMax (dab_warm.h)");
    }
    for (int i = 0; i < t.n; ++i) {
      hipFuncAttributes a;
      (void)hipFuncGetAttributes(&a, t.fn[i]);
    }
    warmed[device] = true;
    phase("code objects");
  }
  *out = h;
  return 0;
}

// DAB_DEV_GUARD=1: after an entry point's device work, every canary of the handle's
// allocators (problem buffers, set-up scratch, kept buffers, Cholesky scratch, and `extra`,
// an entry point's own temporaries) is read back; an overwritten one fails the call closed
// (DAB_E_DEVICE, the first block named in dab_last_error) instead of returning its result
int dab::guard_fail(dab_handle* h, const char* where, Dev* extra) {
  if (!Dev::guard_on() || !h) return 0;
  (void)hipDeviceSynchronize();
  if (Dev::guard_mode() == 2 && std::strcmp(where, "dab_set_problem") == 0 && !h->dev.guards.empty()) {
    const unsigned char one = 1;  // the net's self-test: one byte past the first block
    (void)hipMemcpy(h->dev.guards.front().p, &one, 1, hipMemcpyHostToDevice);
  }
  std::string first;
  int bad = h->dev.guard_check(where, &first) + h->setup_tmp.guard_check(where, &first) +
            h->keep_dev.guard_check(where, &first) + chol_guard_check(h->chol, where, &first);
  if (extra) bad += extra->guard_check(where, &first);
  if (bad == 0) return 0;
  return set_error(DAB_E_DEVICE, "device guard: " + first +
                                     (bad > 1 ? " (and " + std::to_string(bad - 1) + " more)" : std::string()));
}

extern "C" int dab_create(int device, dab_handle** out) {
  clear_error();
  return create_common(device, out);
}

extern "C" int dab_comm_unique_id(uint8_t out_id[128]) {
  clear_error();
  if (!out_id) return set_error(DAB_E_INVALID, "null id buffer");
  ncclUniqueId id;
  NCCL_OK(ncclGetUniqueId(&id));
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
  std::memcpy(out_id, &id, 128);
  return 0;
}

// The one-shot all-reduce contexts: every rank maps every peer's region (IPC handles
// gathered through the handle's own collective). Needs every pair of devices to be
// peer-accessible (one xGMI node); otherwise the sums stay on RCCL.
static int setup_p2p(dab_handle* h) {
  const bool want = h->knobs.p2p > 0 || (h->knobs.p2p < 0 && !h->host_cb);
  if (!want || h->world < 2 || h->world > kP2pMaxRanks) return 0;
  P2pAllgather gather;
  if (h->host_cb) {
    gather = [h](unsigned char* buf) -> int {
      const size_t n = (size_t)h->world * kP2pHandleBytes;
      if (h->stage(n) != 0) return -1;
      for (size_t i = 0; i < n; ++i) h->h_stage[i] = buf[i];
      if (h->host_cb(h->h_stage, (int64_t)n, 0, h->host_user) != 0) return -1;
      for (size_t i = 0; i < n; ++i) buf[i] = (unsigned char)h->h_stage[i];
      return 0;
    };
  } else {
    int ok = 1;  // peer access between this device and every other one of the node
    int ndev = 0;
    (void)hipGetDeviceCount(&ndev);
    for (int d = 0; d < ndev; ++d) {
      int a = 1;
      if (d != h->device && hipDeviceCanAccessPeer(&a, h->device, d) == hipSuccess && !a) ok = 0;
    }
    double f = ok ? 0.0 : 1.0;  // every rank must take the same branch
    double* d_f = nullptr;
    HIP_OK(hipMalloc(&d_f, sizeof(double)));
    HIP_OK(hipMemcpy(d_f, &f, sizeof(double), hipMemcpyHostToDevice));
    NCCL_OK(ncclAllReduce(d_f, d_f, 1, ncclDouble, ncclMax, h->comm, h->stream));
    HIP_OK(hipMemcpyAsync(&f, d_f, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_OK(hipStreamSynchronize(h->stream));
    (void)hipFree(d_f);
    if (f != 0.0) return 0;
    gather = [h](unsigned char* buf) -> int {
      const size_t n = (size_t)h->world * kP2pHandleBytes;
      unsigned char* d = nullptr;
      if (hipMalloc(&d, n) != hipSuccess) return -1;
      int rc = 0;
      if (hipMemcpy(d, buf, n, hipMemcpyHostToDevice) != hipSuccess ||
          ncclAllGather(d + (size_t)h->rank * kP2pHandleBytes, d, kP2pHandleBytes, ncclUint8, h->comm, h->stream) !=
              ncclSuccess ||
          hipMemcpyAsync(buf, d, n, hipMemcpyDeviceToHost, h->stream) != hipSuccess ||
          hipStreamSynchronize(h->stream) != hipSuccess)
        rc = -1;
      (void)hipFree(d);
      return rc;
    };
  }
  P2pComm* ctx[2] = {nullptr, nullptr};
  int rc = p2p_create_group(h->rank, h->world, dab_handle::kP2pWords, 2, gather, ctx);
  // a verified exchange on both contexts before the path is trusted (every rank runs it:
  // the calls are collective)
  for (int k = 0; k < 2 && rc == 0; ++k) rc = p2p_selftest(ctx[k], h->stream);
  // every rank must agree: if the contexts could not be set up or did not verify anywhere,
  // all ranks keep their sums on RCCL (or the host path) instead
  double bad = rc != 0 ? 1.0 : 0.0;
  if (h->host_cb) {
    CHECK_RC(h->stage(1));
    h->h_stage[0] = bad;
    if (h->host_cb(h->h_stage, 1, 1, h->host_user) != 0) return set_error(DAB_E_COMM, "host all-reduce failed");
    bad = h->h_stage[0];
  } else {
    double* d_f = nullptr;
    HIP_OK(hipMalloc(&d_f, sizeof(double)));
    HIP_OK(hipMemcpy(d_f, &bad, sizeof(double), hipMemcpyHostToDevice));
    NCCL_OK(ncclAllReduce(d_f, d_f, 1, ncclDouble, ncclMax, h->comm, h->stream));
    HIP_OK(hipMemcpyAsync(&bad, d_f, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_OK(hipStreamSynchronize(h->stream));
    (void)hipFree(d_f);
  }
  if (bad != 0.0) {
    // one line on stderr: a silent fallback would hide a platform whose peer mappings fail
    fprintf(stderr, "dab: rank %d: peer-to-peer all-reduce not verified (%s); sums stay on %s\n", h->rank,
            rc != 0 ? dab_last_error() : "a peer failed", h->host_cb ? "the host collective" : "RCCL");
    p2p_destroy(ctx[0]);
    p2p_destroy(ctx[1]);
    clear_error();
    return 0;
  }
  h->p2p_main = ctx[0];
  h->p2p_comm = ctx[1];
  return 0;
}

extern "C" int dab_create_dist(int device, int rank, int world_size, const uint8_t unique_id[128],
                               dab_handle** out) {
  clear_error();
  if (world_size < 1 || rank < 0 || rank >= world_size) return set_error(DAB_E_INVALID, "bad rank/world");
  if (world_size > 1 && !unique_id) return set_error(DAB_E_INVALID, "null unique id");
  CHECK_RC(create_common(device, out));
  dab_handle* h = *out;
  h->rank = rank;
  h->world = world_size;
  if (world_size == 1 && unique_id) {
    // one-rank RCCL communicator: the collectives execute (on one GPU) instead of returning
    ncclUniqueId id;
    std::memcpy(&id, unique_id, 128);
    ncclResult_t r = ncclCommInitRank(&h->comm, 1, id, 0);
    if (r != ncclSuccess) {
      std::string msg = std::string("ncclCommInitRank (one rank): ") + ncclGetErrorString(r);
      delete h;
      *out = nullptr;
      return set_error(DAB_E_COMM, msg);
    }
    h->rccl1 = true;
  }
  if (world_size > 1) {
    ncclUniqueId id;
    std::memcpy(&id, unique_id, 128);
    ncclResult_t r = ncclCommInitRank(&h->comm, world_size, id, rank);
    if (r != ncclSuccess) {
      std::string msg = std::string("ncclCommInitRank: ") + ncclGetErrorString(r);
      delete h;
      *out = nullptr;
      return set_error(DAB_E_COMM, msg);
    }
    if (setup_p2p(h) != 0) {
      delete h;
      *out = nullptr;
      return -1;
    }
  }
  return 0;
}

extern "C" int dab_create_dist_host(int device, int rank, int world_size, dab_host_allreduce_fn cb, void* user,
                                    dab_handle** out) {
  clear_error();
  if (world_size < 1 || rank < 0 || rank >= world_size) return set_error(DAB_E_INVALID, "bad rank/world");
  if (world_size > 1 && !cb) return set_error(DAB_E_INVALID, "null all-reduce callback");
  CHECK_RC(create_common(device, out));
  dab_handle* h = *out;
  h->rank = rank;
  h->world = world_size;
  h->host_cb = cb;
  h->host_user = user;
  if (world_size > 1 && setup_p2p(h) != 0) {
    delete h;
    *out = nullptr;
    return -1;
  }
  return 0;
}

extern "C" int dab_destroy(dab_handle* h) {
  clear_error();
  if (!h) return 0;
  (void)hipSetDevice(h->device);
  (void)hipStreamSynchronize(h->stream);
  const double t0 = now_s();
  delete h;
  if (PhaseTimer::on()) std::fprintf(stderr, "destroy %.2f ms\n", 1e3 * (now_s() - t0));
  return 0;
}

extern "C" int dab_update_parameters(dab_handle* h, const double* points, const double* ext) {
  clear_error();
  if (!h || !h->have_problem) return set_error(DAB_E_STATE, "no problem set");
  HIP_OK(hipSetDevice(h->device));
  if (points) {
    std::vector<double> pts((size_t)3 * h->NP);
    for (int i = 0; i < h->NP; ++i)
      for (int k = 0; k < 3; ++k) pts[3 * (size_t)i + k] = points[3 * (size_t)h->pt_of[i] + k];
    HIP_OK(hipMemcpyAsync(h->d_points, pts.data(), pts.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIP_OK(hipStreamSynchronize(h->stream));
  }
  if (ext) {
    HIP_OK(hipMemcpyAsync(h->d_ext, ext, sizeof(double) * 6 * (size_t)h->E, hipMemcpyHostToDevice, h->stream));
    HIP_OK(hipStreamSynchronize(h->stream));
  }
  return 0;
}

extern "C" int dab_get_parameters(dab_handle* h, double* points, double* ext) {
  clear_error();
  if (!h || !h->have_problem) return set_error(DAB_E_STATE, "no problem set");
  HIP_OK(hipSetDevice(h->device));
  if (points) {
    std::vector<double> pts((size_t)3 * h->NP);
    HIP_OK(hipMemcpyAsync(pts.data(), h->d_points, pts.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIP_OK(hipStreamSynchronize(h->stream));
    for (int i = 0; i < h->NP; ++i)
      for (int k = 0; k < 3; ++k) points[3 * (size_t)h->pt_of[i] + k] = pts[3 * (size_t)i + k];
  }
  if (ext) {
    HIP_OK(hipMemcpyAsync(ext, h->d_ext, sizeof(double) * 6 * (size_t)h->E, hipMemcpyDeviceToHost, h->stream));
    HIP_OK(hipStreamSynchronize(h->stream));
  }
  return 0;
}

extern "C" int dab_comm_schedule(dab_handle* h, int32_t* p2p) {
  clear_error();
  if (!h || !p2p) return set_error(DAB_E_INVALID, "null argument");
  *p2p = (h->p2p_main || h->p2p_comm) ? 1 : 0;
  return 0;
}

extern "C" int dab_pcg_schedule(dab_handle* h, int32_t* matrix_free) {
  clear_error();
  if (!h || !h->have_problem || !matrix_free) return set_error(DAB_E_STATE, "no problem set");
  *matrix_free = h->pcg_built && h->mf ? (h->mf32 ? 2 : 1) : 0;
  return 0;
}

extern "C" int dab_eval_schedule(dab_handle* h, int32_t* fused) {
  clear_error();
  if (!h || !h->have_problem || !fused) return set_error(DAB_E_STATE, "no problem set");
  *fused = h->fused ? (h->fused_split ? 2 : 1) : 0;
  return 0;
}
