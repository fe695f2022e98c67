// C ABI of libdsge_hip.so (declared in include/dsge_hip.h): argument checking, kernel
// dispatch on the tile size BS = ceil(n/8), library-owned scratch.  The *_host twins are in api_host.hip.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "dsge_host.hpp"

namespace {
thread_local std::string g_last_error;
}

namespace dsge_host {
int fail(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}
// Compiled-in defaults (never written after load).  One process-level override, read once when the library is loaded: the
// environment variable DSGE_GENSYS_DOUBLING = 0 | 1 | 2 | 3 replaces the default of dsge_options.gensys_doubling (a site that wants the
// ordered QZ for every draw everywhere without touching its callers; the test suite runs its gensys tests under both values).
static Options defaults_from_environment() {
  Options o;
  if (const char* e = std::getenv("DSGE_GENSYS_DOUBLING"))
    if ((e[0] >= '0' && e[0] <= '3') && e[1] == '\0') o.gensys_doubling = e[0] - '0';
  // (A/B switch of the round-6 fused assembly + adjoint launch of the gradient pipeline; not part of dsge_options)
  if (const char* e = std::getenv("DSGE_GRAD_FUSED_ADJOINT"))
    if ((e[0] == '0' || e[0] == '1') && e[1] == '\0') o.grad_fused_adjoint = e[0] - '0';
  return o;
}
const Options g_defaults = defaults_from_environment();
thread_local const Options* t_call_options = nullptr;  // options of the call running on this thread

namespace {
bool g_device_checked = false;
int g_device_ok = 0;
std::mutex g_mutex;
}  // namespace

// Lazy device check (fork-aware: nothing touches HIP before the first call).
int ensure_device() {
  std::lock_guard<std::mutex> lk(g_mutex);
  if (g_device_checked) return g_device_ok ? DSGE_SUCCESS : fail(DSGE_ERR_HIP, "no gfx950 device available");
  g_device_checked = true;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count == 0) {
    (void)hipGetLastError();
    return fail(DSGE_ERR_HIP, "no HIP device visible: libdsge_hip has no CPU fallback");
  }
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, dev));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(DSGE_ERR_HIP, std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only");
  g_device_ok = 1;
  return DSGE_SUCCESS;
}
}  // namespace dsge_host

using namespace dsge_host;

namespace {

// Installs the options of one call on the calling thread (see dsge_host.hpp); nests.
struct OptionsGuard {
  Options local;
  const Options* prev;
  // (grad_fused_adjoint is an internal switch, not in dsge_options: it keeps the process-level value)
  explicit OptionsGuard(const dsge_options* o) : local(g_defaults), prev(t_call_options) {
    if (!o) return;
    static_cast<dsge_options&>(local) = *o;
    t_call_options = &local;
  }
  ~OptionsGuard() { t_call_options = prev; }
};

int check_options(const dsge_options* o) {
  if (!o) return DSGE_SUCCESS;
  if (o->struct_size != sizeof(dsge_options)) return fail(DSGE_ERR_INVALID, "dsge_options.struct_size mismatch (call dsge_options_init)");
  if (!(o->kalman_steady_tol >= 0.0) || o->kalman_steady_tol > 1e-6)
    return fail(DSGE_ERR_INVALID, "kalman_steady_tol must be in [0, 1e-6]");
  if (o->kalman_order < 0 || o->kalman_order > 2) return fail(DSGE_ERR_INVALID, "kalman_order must be 0, 1 or 2");
  if (o->kalman_block < 0 || o->kalman_block > 2) return fail(DSGE_ERR_INVALID, "kalman_block must be 0, 1 or 2");
  if (o->kalman_mfma < 0 || o->kalman_mfma > 2) return fail(DSGE_ERR_INVALID, "kalman_mfma must be 0, 1 or 2");
  if (o->pipeline_chunks < 0 || o->pipeline_chunks > 64) return fail(DSGE_ERR_INVALID, "pipeline_chunks must be in 0..64");
  if (o->gensys_split < 0 || o->gensys_split > 2) return fail(DSGE_ERR_INVALID, "gensys_split must be 0, 1 or 2");
  if (o->gensys_doubling < 0 || o->gensys_doubling > 3) return fail(DSGE_ERR_INVALID, "gensys_doubling must be 0, 1, 2 or 3");
  if (o->kalman_grad_split < 0 || o->kalman_grad_split > 2) return fail(DSGE_ERR_INVALID, "kalman_grad_split must be 0, 1 or 2");
  if (o->n_static_hint < -1 || o->n_static_hint > DSGE_MAX_N) return fail(DSGE_ERR_INVALID, "n_static_hint out of range");
  if (o->ll_constant < DSGE_LL_CONST_P || o->ll_constant > DSGE_LL_CONST_ONE)
    return fail(DSGE_ERR_INVALID, "ll_constant must be DSGE_LL_CONST_P, _OBSERVED or _ONE");
  if (o->jitter_F != o->jitter_F || o->jitter_P != o->jitter_P) return fail(DSGE_ERR_INVALID, "jitter_F / jitter_P must not be NaN");
  return DSGE_SUCCESS;
}

}  // namespace

// ---- StreamArenaPool (dsge_host.hpp) ------------------------------------------------------------------------------------------
namespace dsge_host {
namespace {
std::mutex& pool_registry_mutex() {
  static std::mutex m;
  return m;
}
std::vector<StreamArenaPool*>& pool_registry() {
  static std::vector<StreamArenaPool*> v;
  return v;
}
}  // namespace

StreamArenaPool::StreamArenaPool() {
  std::lock_guard<std::mutex> lk(pool_registry_mutex());
  pool_registry().push_back(this);
}

int StreamArenaPool::reserve(size_t bytes, hipStream_t st, void** out) {
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(mu_);
  Slot* a = nullptr;
  for (auto& slot : slots_)
    if (slot.used && slot.dev == dev && slot.stream == st) a = &slot;
  if (!a)
    for (auto& slot : slots_)
      if (!slot.used && (slot.dev == dev || slot.dev < 0) && (!a || slot.cap > a->cap)) a = &slot;  // the largest free one
  if (!a && slots_.size() < MAX_SLOTS) {
    slots_.emplace_back();
    a = &slots_.back();
  }
  if (!a) {  // every slot is owned by a live stream: take the least recently used one over, once nothing is in flight
    HIP_TRY(hipDeviceSynchronize());
    for (auto& slot : slots_)
      if (slot.dev == dev && (!a || slot.stamp < a->stamp)) a = &slot;
    if (!a) return fail(DSGE_ERR_HIP, "scratch arenas exhausted");
  }
  a->used = true;
  a->dev = dev;
  a->stream = st;
  a->stamp = ++clock_;
  if (a->cap < bytes) {
    if (a->ptr) {
      HIP_TRY(hipDeviceSynchronize());
      HIP_TRY(hipFree(a->ptr));
      a->ptr = nullptr;
      a->cap = 0;
    }
    const size_t cap = bytes + bytes / 4 + 4096;
    HIP_TRY(hipMalloc(&a->ptr, cap));
    a->cap = cap;
  }
  *out = a->ptr;
  return DSGE_SUCCESS;
}

void StreamArenaPool::release(hipStream_t st) {
  std::lock_guard<std::mutex> lk(mu_);
  for (auto& slot : slots_)
    if (slot.used && slot.stream == st) slot.used = false;  // (the memory stays with the slot for its next owner)
}

void stream_arenas_release(hipStream_t st) {
  std::lock_guard<std::mutex> lk(pool_registry_mutex());
  for (StreamArenaPool* p : pool_registry()) p->release(st);
}

// ---- ScratchLayout (dsge_host.hpp) ----
size_t ScratchLayout::bytes() const {
  size_t b = PAD;
  for (int i = 0; i < n_ && i < MAX_BUFS; ++i) b += align256(bufs_[i].bytes);
  return b;
}

int ScratchLayout::reserve(StreamArenaPool& pool, hipStream_t st, void* slice) {
  if (n_ > MAX_BUFS) return fail(DSGE_ERR_INVALID, "ScratchLayout: more buffers declared than MAX_BUFS");
  void* base = slice;
  if (!base) {
    int rc = pool.reserve(bytes(), st, &base);
    if (rc) return rc;
  }
  char* p = (char*)base;
  for (int i = 0; i < n_; ++i) {
    std::memcpy(bufs_[i].slot, &p, sizeof(p));  // (the slot is some T*: every object pointer has this representation)
    p += align256(bufs_[i].bytes);
  }
  return DSGE_SUCCESS;
}

// ---- ThreadStream (dsge_host.hpp) ----
int ThreadStream::ensure() {
  int dev = 0;
  HIP_TRY(hipGetDevice(&dev));
  if (dev_ == dev && s_ && ev_[0] && ev_[1]) return DSGE_SUCCESS;
  // another device than last time, or a creation that failed half-way: drop what exists, then create all three -- a failure
  // leaves a partially filled record behind that the next call (or the destructor) drops
  drop();
  dev_ = dev;
  HIP_TRY(hipStreamCreateWithFlags(&s_, hipStreamNonBlocking));
  for (auto& e : ev_) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  return DSGE_SUCCESS;
}

void ThreadStream::drop() {  // (idempotent; the owning device is made current for the destroy calls and the caller's restored)
  if (!s_ && !ev_[0] && !ev_[1]) return;
  int cur = 0;
  const bool have_cur = hipGetDevice(&cur) == hipSuccess;
  if (dev_ >= 0) (void)hipSetDevice(dev_);
  if (s_) {
    (void)hipStreamSynchronize(s_);
    stream_arenas_release(s_);
    (void)hipStreamDestroy(s_);
    s_ = nullptr;
  }
  for (auto& e : ev_) {
    if (e) (void)hipEventDestroy(e);
    e = nullptr;
  }
  open_ = false;
  if (have_cur) (void)hipSetDevice(cur);
  (void)hipGetLastError();
}

int ThreadStream::fork(hipStream_t from) {
  int rc = ensure();
  if (rc) return rc;
  HIP_TRY(hipEventRecord(ev_[0], from));
  HIP_TRY(hipStreamWaitEvent(s_, ev_[0], 0));
  open_ = true;
  return DSGE_SUCCESS;
}

int ThreadStream::join(hipStream_t into) {
  HIP_TRY(hipEventRecord(ev_[1], s_));
  HIP_TRY(hipStreamWaitEvent(into, ev_[1], 0));
  open_ = false;
  return DSGE_SUCCESS;
}

void ThreadStream::close(hipStream_t into) {
  if (!open_) return;
  if (hipEventRecord(ev_[1], s_) != hipSuccess || hipStreamWaitEvent(into, ev_[1], 0) != hipSuccess)
    (void)hipStreamSynchronize(s_);
  (void)hipGetLastError();
  open_ = false;
}

int twin_streams(hipStream_t* s0, hipStream_t* s1) {
  static thread_local ThreadStream t_twin[2];
  for (auto& t : t_twin) {
    int rc = t.ensure();
    if (rc) return rc;
  }
  *s0 = t_twin[0].stream();
  if (s1) *s1 = t_twin[1].stream();
  return DSGE_SUCCESS;
}

}  // namespace dsge_host

namespace {
// The stream the verdict of gensys by spectral division runs on, next to the filter on the caller's stream (pipeline_unchunked(),
// round 6), and the streams the chunks of dsge_options.pipeline_chunks alternate over
thread_local ThreadStream t_verdict;
constexpr int MAX_CHUNK_STREAMS = 8;
thread_local ThreadStream t_chunk[MAX_CHUNK_STREAMS];

// Scratch of the device entry points (one arena per (device, stream), StreamArenaPool)
StreamArenaPool g_scratch_pool;
StreamArenaPool g_aug_big_pool;  // the gathered model of the augmented route beyond 64 states

// The chain every entry across dated breaks (dsge_kalman_seg.hpp) runs up to P0, on the caller's stream: sym(R Q R') of every (draw,
// segment) by the launch dsge_lyapunov_batched uses (the layouts flatten to batch * S draws; a shared Q is first repeated per draw),
// P0 of segment 0 by the Lyapunov launch on T_0 and sym(R_0 Q_0 R_0') (gathered when S > 1) unless the caller gave P0.
//
//   SegmentChain ch;
//   if ((rc = ch.declare(s, chunk, "segmented ...", other_lds_bytes))) return rc;  // the refusals; the chain's scratch at the head of ch.lay
//   ch.lay.add(...);                                                               // the entry's own scratch behind it
//   if ((rc = ch.reserve(s, st))) return rc;
//   per chunk c = s.at(c0, nb):  if ((rc = ch.run(c, status_io + c0, st))) return rc;  then the filter on ch.RQR, ch.P0 (and ch.qe)
struct SegmentChain {
  ScratchLayout lay;
  double* RQR = nullptr;     // [chunk][S][m][m]
  const double* P0 = nullptr;  // after run(): the caller's P0 of the chunk, or the chain's
  ShockCov qe;               // after run(): the chunk's Q in a *_BATCHED layout over its (draw, segment) problems

  // `name` prefixes the refusals (DSGE_ERR_TOO_LARGE); other_lds_bytes: the LDS image of the entry's own kernel behind the filter
  int declare(const SegmentedProblem& s, int chunk, const char* name, size_t other_lds_bytes) {
    unsigned flat_all = 0;
    if (int rc = batch_grid(s.batch, s.n_seg, (std::string(name) + ": batch * n_seg exceeds 2^31 - 1").c_str(), &flat_all)) return rc;
    if (kalman_segments_lds_bytes(s.m, s.obs.p) > LDS_LIMIT || other_lds_bytes > LDS_LIMIT)
      return fail(DSGE_ERR_TOO_LARGE, std::string(name) + ": LDS budget exceeded");
    const size_t mm = (size_t)s.m * s.m;
    rows_ = (size_t)chunk * s.n_seg;
    lay.add(&RQR, rows_ * mm);
    if (!s.q.batched()) lay.add(&Qx_, rows_ * s.q_width());
    if (!s.P0 && s.n_seg > 1) {
      lay.add(&T0_, chunk * mm);
      lay.add(&G0_, chunk * mm);
    }
    if (!s.P0) lay.add(&P0s_, chunk * mm);
    return DSGE_SUCCESS;
  }
  int reserve(const SegmentedProblem& s, hipStream_t st) {
    if (int rc = lay.reserve(g_scratch_pool, st)) return rc;
    // (a shared Q repeats with period S: its first nb * S rows serve every chunk)
    return s.q.batched() ? DSGE_SUCCESS : launch_segment_rows(Qx_, s.q.Q, rows_, (int)s.q_width(), s.n_seg, 1, st);
  }
  int run(const SegmentedProblem& c, int32_t* status, hipStream_t st) {
    const int mm = c.m * c.m;
    int rc;
    qe = c.q.batched() ? c.q : ShockCov{Qx_, c.q.diag() ? DSGE_Q_DIAG_BATCHED : DSGE_Q_FULL_BATCHED};
    // (no status here: a skipped draw's product is never read, and the words are per draw, not per (draw, segment))
    if ((rc = assemble_rqr(c.R, qe, (int)c.flat(), c.m, c.k, RQR, nullptr, st))) return rc;
    P0 = c.P0;
    if (P0) return DSGE_SUCCESS;
    const double* Ts = c.T;
    double* Gs = RQR;
    if (c.n_seg > 1) {
      if ((rc = launch_segment_rows(T0_, c.T, (size_t)c.batch, mm, c.batch, c.n_seg, st))) return rc;
      if ((rc = launch_segment_rows(G0_, RQR, (size_t)c.batch, mm, c.batch, c.n_seg, st))) return rc;
      Ts = T0_;
      Gs = G0_;
    }
    P0 = P0s_;
    return assemble_p0_from_rqr(Ts, Gs, c.batch, c.m, P0s_, status, false, st);
  }

 private:
  double *Qx_ = nullptr, *T0_ = nullptr, *G0_ = nullptr, *P0s_ = nullptr;
  size_t rows_ = 0;  // (draw, segment) problems of a full chunk
};
}  // namespace

extern "C" {

int dsge_abi_version(void) { return DSGE_ABI_VERSION; }
const char* dsge_last_error(void) { return g_last_error.c_str(); }

// The debug counter hooks: enable = 1 allocates (zeroed) the device buffer *slot of `count` int64 the kernels of one family
// stamp, cycles_out (host, may be NULL) reads it back behind a device synchronisation, enable = 0 frees it.
static int debug_counters(long long** slot, int count, int enable, long long* cycles_out) {
  int rc = ensure_device();
  if (rc) return rc;
  if (enable && !*slot) {
    HIP_TRY(hipMalloc((void**)slot, count * sizeof(long long)));
    HIP_TRY(hipMemset(*slot, 0, count * sizeof(long long)));
  }
  if (cycles_out && *slot) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(cycles_out, *slot, count * sizeof(long long), hipMemcpyDeviceToHost));
  }
  if (!enable && *slot) {
    (void)hipFree(*slot);
    *slot = nullptr;
  }
  return DSGE_SUCCESS;
}
int dsge_debug_cr_phases(int enable, long long* cycles_out) { return debug_counters(&g_cr_dbg, 8, enable, cycles_out); }
int dsge_debug_cr_fused_phases(int enable, long long* cycles_out) { return debug_counters(&g_cr_fused_dbg, 24, enable, cycles_out); }
int dsge_debug_second_order_phases(int enable, long long* cycles_out) { return debug_counters(&g_so_dbg, 8, enable, cycles_out); }
int dsge_debug_pruned_phases(int enable, long long* cycles_out) { return debug_counters(&g_pruned_dbg, 8, enable, cycles_out); }
int dsge_debug_shock_decomp_phases(int enable, long long* cycles_out) { return debug_counters(&g_shock_decomp_dbg, 8, enable, cycles_out); }
int dsge_debug_condfc_phases(int enable, long long* cycles_out) { return debug_counters(&g_condfc_dbg, 8, enable, cycles_out); }
int dsge_debug_adjoint_refine(int mode) {
  if (mode < 0 || mode > 2) return fail(DSGE_ERR_INVALID, "mode out of range (0..2)");
  g_adj_refine_mode = mode;
  return DSGE_SUCCESS;
}
int dsge_debug_cr_static_rows(int mode) {
  if (mode < 0 || mode > 2) return fail(DSGE_ERR_INVALID, "mode out of range (0..2)");
  g_cr_static_rows_mode = mode;
  return DSGE_SUCCESS;
}
int dsge_debug_cr_refine(int mode) {
  if (mode < 0 || mode > 1) return fail(DSGE_ERR_INVALID, "mode out of range (0..1)");
  g_cr_refine_mode = mode;
  return DSGE_SUCCESS;
}
int dsge_forget_measured_shapes(void) {
  cr_deflation_reset();
  gensys_shape_reset();
  return DSGE_SUCCESS;
}
int dsge_debug_kalman_steady_steps(int32_t* steady_at_device) {
  g_kalman_steady_at = steady_at_device;
  return DSGE_SUCCESS;
}
int dsge_debug_kalman_timeline(long long* timeline_device) {
  g_kalman_timeline = timeline_device;
  return DSGE_SUCCESS;
}

int dsge_device_count(void) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  int ok = 0;
  for (int i = 0; i < count; ++i) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, i) == hipSuccess && std::strncmp(prop.gcnArchName, "gfx950", 6) == 0) ++ok;
  }
  return ok;
}

int dsge_set_device(int device) {
  HIP_TRY(hipSetDevice(device));
  return DSGE_SUCCESS;
}

int dsge_stream_synchronize(void* stream) {
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  return DSGE_SUCCESS;
}

static int cr_entry(const double* A, const double* B, const double* C, int batch, int n, int max_iter, double tol,
                    double* T_out, int32_t* status, int32_t* n_iter, void* stream, int scan_mode) {
  int rc = check_common(batch, n, DSGE_MAX_N_BIG);
  if (rc) return rc;
  if (!A || !B || !C || !T_out || !status) return fail(DSGE_ERR_INVALID, "null pointer");
  if (max_iter < 0) return fail(DSGE_ERR_INVALID, "max_iter < 0");
  if ((rc = ensure_device())) return rc;
  if (batch == 0) return DSGE_SUCCESS;
  if (big_size(n))  // 65 .. 96 variables: one workgroup per draw (dsge_big.hpp)
    return launch_cr_big(A, B, C, batch, n, max_iter, tol, T_out, status, n_iter, (hipStream_t)stream, scan_mode, nullptr, 0,
                         nullptr);
  return launch_cr(A, B, C, batch, n, max_iter, tol, T_out, status, n_iter, (hipStream_t)stream, scan_mode);
}

int dsge_cycle_reduction_batched(const double* A, const double* B, const double* C, int batch, int n, int max_iter,
                                 double tol, double* T_out, int32_t* status, int32_t* n_iter, void* stream) {
  return cr_entry(A, B, C, batch, n, max_iter, tol, T_out, status, n_iter, stream, 0);
}

int dsge_scan_cycle_reduction_batched(const double* A, const double* B, const double* C, int batch, int n,
                                      int max_iter, double tol, double* T_out, int32_t* status, int32_t* n_steps,
                                      void* stream) {
  return cr_entry(A, B, C, batch, n, max_iter, tol, T_out, status, n_steps, stream, 1);
}

int dsge_gensys_batched(const double* A, const double* B, const double* C, const double* D, int batch, int n, int k,
                        double tol, int n_lead_hint, double* T_out, double* R_out, int32_t* eu_out, int32_t* status,
                        void* stream) {
  // 65 .. 96 variables: by spectral division only (csrc/dsge_big.hpp: gensys_certify_big_kernel; no ordered QZ at that size)
  const bool big = big_size(n) && opt().gensys_doubling != 0;
  int rc = check_common(batch, n, big ? DSGE_MAX_N_BIG : DSGE_MAX_N_GENSYS - 1);
  if (rc) return rc;
  if (!A || !B || !C || !T_out || !eu_out || !status) return fail(DSGE_ERR_INVALID, "null pointer");
  if (R_out && (!D || k < 1 || k > n)) return fail(DSGE_ERR_INVALID, "R_out requires D and 1 <= k <= n");
  if ((rc = ensure_device())) return rc;
  if (batch == 0) return DSGE_SUCCESS;
  if (big) return launch_gensys_big(A, B, C, D, batch, n, k, tol, T_out, R_out, eu_out, status, nullptr, (hipStream_t)stream);
  if ((rc = launch_gensys(A, B, C, batch, n, tol, n_lead_hint, T_out, eu_out, status, (hipStream_t)stream, nullptr, nullptr, nullptr,
                          R_out ? D : nullptr, k, R_out)))
    return rc;
  if (R_out)  // gensys_pt: R = -(C T + B)^-1 D  (gensys.py:681); computed for every draw, as the graph does
    return assemble_selection(nullptr, B, C, D, T_out, batch, n, k, R_out, nullptr, nullptr, (hipStream_t)stream);
  return DSGE_SUCCESS;
}

int dsge_gensys_pencil_batched(const double* g0, const double* g1, const double* c, const double* psi, const double* pi,
                               int batch, int N, int k, int n_eta, double tol, double* G1_out, double* C_out,
                               double* impact_out, double* gev_out, int32_t* eu_out, int32_t* status, void* stream) {
  return dsge_gensys_pencil_full_batched(g0, g1, c, psi, pi, batch, N, k, n_eta, tol, G1_out, C_out, impact_out, gev_out,
                                         eu_out, status, nullptr, stream);
}

int dsge_gensys_pencil_full_batched(const double* g0, const double* g1, const double* c, const double* psi,
                                    const double* pi, int batch, int N, int k, int n_eta, double tol, double* G1_out,
                                    double* C_out, double* impact_out, double* gev_out, int32_t* eu_out, int32_t* status,
                                    const dsge_gensys_forward* forward, void* stream) {
  int rc = check_common(batch, N, DSGE_MAX_N_GENSYS);
  if (rc) return rc;
  if (k < 1 || n_eta < 0 || n_eta + k + 1 > 64) return fail(DSGE_ERR_INVALID, "need k >= 1, n_eta >= 0, n_eta + k + 1 <= 64");
  if (!g0 || !g1 || !psi || (n_eta > 0 && !pi) || !G1_out || !C_out || !impact_out || !gev_out || !eu_out || !status)
    return fail(DSGE_ERR_INVALID, "null pointer");
  if ((rc = ensure_device())) return rc;
  if (batch == 0) return DSGE_SUCCESS;
  if (forward && forward->loose && n_eta < 1) return fail(DSGE_ERR_INVALID, "loose needs n_eta >= 1");
  return launch_gensys_pencil(g0, g1, c, psi, pi, batch, N, k, n_eta, tol, G1_out, C_out, impact_out, gev_out, eu_out, status,
                              (hipStream_t)stream, forward);
}

int dsge_bk_eigenvalues_batched(const double* A, const double* B, const double* C, int batch, int n, double tol,
                                double* eig_re, double* eig_im, int32_t* n_eig, int32_t* n_forward,
                                int32_t* n_unstable, int32_t* status, void* stream) {
  int rc = check_common(batch, n, DSGE_MAX_N_GENSYS - 1);
  if (rc) return rc;
  if (!A || !B || !C || !eig_re || !eig_im || !n_eig || !n_forward || !n_unstable || !status)
    return fail(DSGE_ERR_INVALID, "null pointer");
  if ((rc = ensure_device())) return rc;
  if (batch == 0) return DSGE_SUCCESS;
  return launch_gensys_bk(A, B, C, batch, n, tol, eig_re, eig_im, n_eig, n_forward, n_unstable, status,
                          (hipStream_t)stream);
}

int dsge_selection_batched(const double* A, const double* B, const double* C, const double* D, const double* T,
                           int batch, int n, int k, double* R_out, double* resid_out, void* stream) {
  int rc = check_common(batch, n, DSGE_MAX_N_BIG);
  if (rc) return rc;
  if (k < 1 || k > n) return fail(DSGE_ERR_INVALID, "k out of range (1..n)");
  if (!B || !C || !D || !T || !R_out) return fail(DSGE_ERR_INVALID, "null pointer");
  if (resid_out && !A) return fail(DSGE_ERR_INVALID, "resid_out requires A");
  if ((rc = ensure_device())) return rc;
  if (batch == 0) return DSGE_SUCCESS;
  if (big_size(n)) return launch_selection_big(A, B, C, D, T, batch, n, k, R_out, resid_out, nullptr, (hipStream_t)stream);
  return assemble_selection(A, B, C, D, T, batch, n, k, R_out, resid_out, nullptr, (hipStream_t)stream);
}

int dsge_policy_adjoints_batched(const double* B, const double* C, const double* T, const double* T_bar, int batch,
                                 int n, double* A_bar, double* B_bar, double* C_bar, int32_t* status, void* stream) {
  int rc = check_common(batch, n, 56);  // [M' | T_bar | C'] + two operands in LDS: n <= 56 (132 KB at the 64-wide tile, not built)
  if (rc) return rc;
  if (!B || !C || !T || !T_bar || !A_bar || !B_bar || !C_bar || !status) return fail(DSGE_ERR_INVALID, "null pointer");
  if ((rc = ensure_device())) return rc;
  if (batch == 0) return DSGE_SUCCESS;
  return launch_adjoint(B, C, T, T_bar, batch, n, A_bar, B_bar, C_bar, status, (hipStream_t)stream);
}

int dsge_selection_adjoints_batched(const double* B, const double* C, const double* T, const double* R, const double* R_bar,
                                    int batch, int n, int k, double* B_bar, double* C_bar, double* D_bar, double* T_bar,
                                    void* stream) {
  int rc = check_common(batch, n, 56);  // (grad_assemble_kernel: 153 KB of LDS at the 56-wide tile, 199 KB at 64)
  if (rc) return rc;
  if (k < 1 || k > n) return fail(DSGE_ERR_INVALID, "k out of range (1..n)");
  if (!B || !C || !T || !R || !R_bar || !B_bar || !C_bar || !D_bar || !T_bar) return fail(DSGE_ERR_INVALID, "null pointer");
  if ((rc = ensure_device())) return rc;
  if (batch == 0) return DSGE_SUCCESS;
  return launch_grad_assemble(B, C, T, R, nullptr, 0, nullptr, batch, n, k, nullptr, T_bar, B_bar, C_bar, D_bar, nullptr,
                              (hipStream_t)stream, R_bar);
}

int dsge_policy_norms_batched(const double* A, const double* B, const double* C, const double* D, const double* T,
                              const double* R, const int32_t* state_mask, int batch, int n, int k,
                              double* det_norm_out, double* stoch_norm_out, void* stream) {
  int rc = check_common(batch, n, 56);  // five n x n matrices in LDS: n <= 56
  if (rc) return rc;
  if (k < 1 || k > n) return fail(DSGE_ERR_INVALID, "k out of range (1..n)");
  if (!A || !B || !C || !D || !T || !R || !state_mask || !det_norm_out || !stoch_norm_out)
    return fail(DSGE_ERR_INVALID, "null pointer");
  if ((rc = ensure_device())) return rc;
  if (batch == 0) return DSGE_SUCCESS;
  return launch_norms(A, B, C, D, T, R, state_mask, batch, n, k, det_norm_out, stoch_norm_out, (hipStream_t)stream);
}

int dsge_backward_direct_batched(const double* A, const double* B, const double* D, int batch, int n, int k,
                                 double* T_out, double* R_out, void* stream) {
  int rc = check_common(batch, n, DSGE_MAX_N_CR);
  if (rc) return rc;
  if (k < 1 || k > n) return fail(DSGE_ERR_INVALID, "k out of range (1..n)");
  if (!A || !B || !D || !T_out || !R_out) return fail(DSGE_ERR_INVALID, "null pointer");
  if ((rc = ensure_device())) return rc;
  if (batch == 0) return DSGE_SUCCESS;
  return launch_bdirect(A, B, D, batch, n, k, T_out, R_out, (hipStream_t)stream);
}

int dsge_lyapunov_batched(const double* T, const double* R, const double* Q, int q_mode, int batch, int m, int k,
                          double* P0_out, double* RQR_out, int32_t* status, void* stream) {
  int rc = check_common(batch, m, DSGE_MAX_N);
  if (rc) return rc;
  if (k < 1 || k > m) return fail(DSGE_ERR_INVALID, "k out of range (1..m)");
  if (q_mode < 0 || q_mode > 3) return fail(DSGE_ERR_INVALID, "bad q_mode");
  if (!T || !R || !Q || !P0_out || !status) return fail(DSGE_ERR_INVALID, "null pointer");
  if ((rc = ensure_device())) return rc;
  if (batch == 0) return DSGE_SUCCESS;
  HIP_TRY(hipMemsetAsync(status, 0, sizeof(int32_t) * batch, (hipStream_t)stream));
  return assemble_rqr_p0(T, R, ShockCov{Q, q_mode}, batch, m, k, RQR_out, P0_out, status, (hipStream_t)stream);
}

int dsge_autocorrelation_batched(const double* T, const double* R, const double* Q, int q_mode, const double* Z,
                                 const double* Hdiag, int batch, int m, int k, int p, int n_lags, int lag_step,
                                 int correlation, double* acf_out, double* Sigma_out, int32_t* status, void* stream) {
  int rc = check_common(batch, m, DSGE_MAX_N);
  if (rc) return rc;
  if (k < 1 || k > m) return fail(DSGE_ERR_INVALID, "k out of range (1..m)");
  if (q_mode < 0 || q_mode > 3) return fail(DSGE_ERR_INVALID, "bad q_mode");
  if (n_lags < 0 || lag_step < 1) return fail(DSGE_ERR_INVALID, "n_lags >= 0 and lag_step >= 1 required");
  if (Z && (p < 1 || p > DSGE_MAX_P)) return fail(DSGE_ERR_INVALID, "p out of range (1..DSGE_MAX_P)");
  if (!T || !R || !Q || !acf_out || !status) return fail(DSGE_ERR_INVALID, "null pointer");
  if ((rc = ensure_device())) return rc;
  if (batch == 0) return DSGE_SUCCESS;
  hipStream_t st = (hipStream_t)stream;
  double* Sigma = Sigma_out;
  if (!Sigma) {
    ScratchLayout lay;
    lay.add(&Sigma, (size_t)batch * m * m);
    if ((rc = lay.reserve(g_scratch_pool, st))) return rc;
  }
  HIP_TRY(hipMemsetAsync(status, 0, sizeof(int32_t) * batch, st));
  if ((rc = assemble_rqr_p0(T, R, ShockCov{Q, q_mode}, batch, m, k, nullptr, Sigma, status, st))) return rc;
  return launch_acf(T, Sigma, Z, Hdiag, batch, m, p, n_lags, lag_step, correlation, acf_out, status, st);
}

int dsge_kalman_filter_outputs_batched(const double* T, const double* R, const double* Q, int q_mode, const double* Z,
                                       int z_batched, const double* d, int d_batched, const double* Hdiag, int h_batched,
                                       const double* y, int batch, int m, int k, int p, int T_len, double jitter,
                                       double missing_fill, double* ll_out, double* a_pred_out, double* a_filt_out,
                                       double* p_pred_out, double* p_filt_out, int full_cov, int32_t* status_io, void* stream) {
  const ObsModel obs{Z, z_batched, d, d_batched, Hdiag, h_batched, y, p, T_len, jitter, missing_fill};
  const ShockCov q{Q, q_mode};
  int rc = check_kalman(batch, m, k, obs, q, T && R && ll_out && status_io);
  if (rc) return rc;
  if ((rc = ensure_device())) return rc;
  if (batch == 0) return DSGE_SUCCESS;
  hipStream_t st = (hipStream_t)stream;
  const size_t mm = (size_t)batch * m * m;
  double *RQR = nullptr, *P0 = nullptr;
  ScratchLayout lay;
  lay.add(&RQR, mm);
  lay.add(&P0, mm);
  if ((rc = lay.reserve(g_scratch_pool, st))) return rc;
  if ((rc = assemble_rqr_p0(T, R, q, batch, m, k, RQR, P0, status_io, st))) return rc;
  return launch_kalman_outputs(T, RQR, P0, obs, batch, m, ll_out, a_pred_out, a_filt_out, p_pred_out, p_filt_out, full_cov,
                               status_io, st);
}

// The likelihood across dated breaks (dsge_kalman_seg.hpp), a chain on the caller's stream: SegmentChain on the whole batch, then the
// filter.
int dsge_kalman_logp_segments_batched(const double* T, const double* R, const double* Q, int q_mode, const double* Z, int z_batched,
                                      const double* d, int d_batched, const double* Hdiag, int h_batched, const double* a0,
                                      const double* P0, const double* shift, const double* y, const int32_t* seg_start, int n_seg,
                                      int batch, int m, int k, int p, int T_len, double jitter, double missing_fill, double* logp_out,
                                      double* ll_out, double* a_last_out, double* P_last_out, int32_t* status_io, void* stream) {
  const ObsModel obs{Z, z_batched, d, d_batched, Hdiag, h_batched, y, p, T_len, jitter, missing_fill};
  const ShockCov q{Q, q_mode};
  int rc = check_kalman_segments(batch, m, k, obs, q, seg_start, n_seg, T && R && logp_out && status_io);
  if (rc) return rc;
  if ((rc = ensure_device())) return rc;
  if (batch == 0 || T_len == 0) return DSGE_SUCCESS;
  hipStream_t st = (hipStream_t)stream;
  const SegmentedProblem s{T, R, q, obs, a0, P0, shift, seg_start, n_seg, batch, m, k};
  SegmentChain ch;
  if ((rc = ch.declare(s, batch, "segmented filter", 0))) return rc;
  if ((rc = ch.reserve(s, st))) return rc;
  if ((rc = ch.run(s, status_io, st))) return rc;
  return launch_kalman_segments(s, ch.RQR, ch.P0, logp_out, ll_out, a_last_out, P_last_out, status_io, st);
}

// Smoothed states, covariances and shocks (dsge_kalman_smooth.hpp): the forward pass is launch_kalman_outputs with full
// covariances into library scratch, one contiguous chunk of draws after the other on the caller's stream.
int dsge_kalman_smoother_batched(const double* T, const double* R, const double* Q, int q_mode, const double* Z, int z_batched,
                                 const double* d, int d_batched, const double* Hdiag, int h_batched, const double* y, int batch,
                                 int m, int k, int p, int T_len, double jitter, double missing_fill, double rank_tol,
                                 size_t scratch_limit_bytes, double* ll_out, double* a_smooth_out, double* p_smooth_out,
                                 double* eps_smooth_out, int full_cov, int32_t* status_io, void* stream) {
  const ObsModel obs{Z, z_batched, d, d_batched, Hdiag, h_batched, y, p, T_len, jitter, missing_fill};
  const ShockCov q{Q, q_mode};
  int rc = check_smoother(batch, m, k, obs, q, T && R && status_io, a_smooth_out || p_smooth_out || eps_smooth_out);
  if (rc) return rc;
  if ((rc = ensure_device())) return rc;
  if (batch == 0 || T_len == 0) return DSGE_SUCCESS;
  hipStream_t st = (hipStream_t)stream;
  if (!(rank_tol > 0.0)) rank_tol = 1e-10;
  // the per-step filter outputs of one draw (the limit counts these; the per-draw matrices next to them are a few m^2)
  const size_t tm = (size_t)T_len * m, per_draw = (2 * tm * m + 2 * tm) * sizeof(double);
  const int chunk = chunk_for(scratch_limit_bytes, per_draw, batch);
  const size_t mm = (size_t)chunk * m * m, img = (size_t)chunk * smoother_image_doubles(m);
  double *RQR = nullptr, *P0 = nullptr, *U = nullptr, *UT = nullptr, *UR = nullptr, *ap = nullptr, *af = nullptr, *pp = nullptr, *pf = nullptr;
  double* ll = nullptr;
  int32_t* rank = nullptr;
  ScratchLayout lay;
  lay.add(&RQR, mm);
  lay.add(&P0, mm);
  lay.add(&U, img);
  lay.add(&UT, img);
  lay.add(&UR, img);
  lay.add(&ap, chunk * tm);
  lay.add(&af, chunk * tm);
  lay.add(&pp, chunk * tm * m);
  lay.add(&pf, chunk * tm * m);
  lay.add(&rank, (size_t)chunk);
  if (!ll_out) lay.add(&ll, (size_t)chunk * T_len);
  if ((rc = lay.reserve(g_scratch_pool, st))) return rc;
  const size_t tc = full_cov ? tm * m : tm;
  for (int c0 = 0; c0 < batch; c0 += chunk) {
    const int nb = chunk_draws(batch, c0, chunk);
    const size_t o = (size_t)c0;
    const double *Tc = T + o * m * m, *Rc = R + o * m * k;
    const ShockCov qc = q.at(o, k);
    int32_t* sc = status_io + o;
    if ((rc = assemble_rqr_p0(Tc, Rc, qc, nb, m, k, RQR, P0, sc, st))) return rc;
    if ((rc = launch_kalman_outputs(Tc, RQR, P0, obs.at(o, m), nb, m, ll_out ? ll_out + o * T_len : ll, ap, af, pp, pf, 1, sc, st)))
      return rc;
    if ((rc = launch_kalman_smoother(Tc, Rc, qc, nb, m, k, T_len, rank_tol, U, UT, UR, rank, ap, af, pp, pf,
                                     a_smooth_out ? a_smooth_out + o * tm : nullptr, p_smooth_out ? p_smooth_out + o * tc : nullptr,
                                     eps_smooth_out ? eps_smooth_out + o * T_len * k : nullptr, full_cov, sc, st)))
      return rc;
  }
  return DSGE_SUCCESS;
}

// The smoother across dated breaks (docs/design/segmented_smoother.md), per chunk of draws on the caller's stream: the chain of
// dsge_kalman_logp_segments_batched up to P0, the storing instantiation of its filter (full covariances into library scratch, the
// per-step outputs the caller asked for next to them), the basis of every (draw, segment) and the backward pass.
int dsge_kalman_smoother_segments_batched(const double* T, const double* R, const double* Q, int q_mode, const double* Z, int z_batched,
                                          const double* d, int d_batched, const double* Hdiag, int h_batched, const double* a0,
                                          const double* P0, const double* shift, const double* y, const int32_t* seg_start, int n_seg,
                                          int batch, int m, int k, int p, int T_len, double jitter, double missing_fill,
                                          double rank_tol, size_t scratch_limit_bytes, int full_cov, double* ll_out,
                                          double* a_pred_out, double* a_filt_out, double* p_pred_out, double* p_filt_out,
                                          double* a_smooth_out, double* p_smooth_out, double* eps_smooth_out, int32_t* status_io,
                                          void* stream) {
  const ObsModel obs{Z, z_batched, d, d_batched, Hdiag, h_batched, y, p, T_len, jitter, missing_fill};
  const ShockCov q{Q, q_mode};
  int rc = check_smoother_segments(batch, m, k, obs, q, seg_start, n_seg, T && R && status_io,
                                   ll_out || a_pred_out || a_filt_out || p_pred_out || p_filt_out || a_smooth_out || p_smooth_out ||
                                       eps_smooth_out);
  if (rc) return rc;
  if ((rc = ensure_device())) return rc;
  if (batch == 0 || T_len == 0) return DSGE_SUCCESS;
  hipStream_t st = (hipStream_t)stream;
  const SegmentedProblem s{T, R, q, obs, a0, P0, shift, seg_start, n_seg, batch, m, k};
  if (!(rank_tol > 0.0)) rank_tol = 1e-10;
  const size_t S = (size_t)n_seg, tm = (size_t)T_len * m;
  const size_t per_draw = (2 * tm * m + 2 * tm + 3 * S * smoother_image_doubles(m)) * sizeof(double);
  const int chunk = chunk_for(scratch_limit_bytes, per_draw, batch);
  const size_t cf = (size_t)chunk * S, img = cf * smoother_image_doubles(m);
  const bool smooth = a_smooth_out || p_smooth_out || eps_smooth_out;
  double *U = nullptr, *UT = nullptr, *UR = nullptr, *ap = nullptr, *af = nullptr, *pp = nullptr, *pf = nullptr;
  int32_t *rank = nullptr, *sflat = nullptr;
  SegmentChain ch;
  if ((rc = ch.declare(s, chunk, "segmented smoother", smoother_lds_bytes(m)))) return rc;
  ch.lay.add(&U, img);
  ch.lay.add(&UT, img);
  ch.lay.add(&UR, img);
  ch.lay.add(&ap, chunk * tm);
  ch.lay.add(&af, chunk * tm);
  ch.lay.add(&pp, chunk * tm * m);
  ch.lay.add(&pf, chunk * tm * m);
  ch.lay.add(&rank, cf);
  ch.lay.add(&sflat, cf);
  if ((rc = ch.reserve(s, st))) return rc;
  const size_t tc = full_cov ? tm * m : tm;
  auto at = [](double* x, size_t off) { return x ? x + off : nullptr; };
  for (int c0 = 0; c0 < batch; c0 += chunk) {
    const size_t o = (size_t)c0;
    const SegmentedProblem c = s.at(o, chunk_draws(batch, c0, chunk));
    int32_t* sc = status_io + o;
    if ((rc = ch.run(c, sc, st))) return rc;
    if ((rc = launch_kalman_segments_store(c, ch.RQR, ch.P0, nullptr, at(ll_out, o * T_len), ap, af, pp, pf, at(a_pred_out, o * tm),
                                           at(a_filt_out, o * tm), at(p_pred_out, o * tc), at(p_filt_out, o * tc), full_cov, sc, st)))
      return rc;
    if (smooth && (rc = launch_kalman_smoother_segments(c.T, c.R, ch.qe, seg_start, n_seg, c.batch, m, k, T_len, rank_tol, U, UT, UR, rank,
                                                        sflat, ap, af, pp, pf, at(a_smooth_out, o * tm), at(p_smooth_out, o * tc),
                                                        at(eps_smooth_out, o * T_len * k), full_cov, sc, st)))
      return rc;
  }
  return DSGE_SUCCESS;
}

// The gradient of the likelihood across dated breaks (docs/design/segmented_gradient.md), per chunk of draws on the caller's stream:
// the chain of dsge_kalman_logp_segments_batched up to P0, the storing instantiation of its filter (logp, and the moments of every
// period into library scratch), the reverse sweep over them, then R_bar / Q_bar from the cotangent of sym(R Q R').
int dsge_kalman_logp_segments_grad_batched(const double* T, const double* R, const double* Q, int q_mode, const double* Z, int z_batched,
                                           const double* d, int d_batched, const double* Hdiag, int h_batched, const double* a0,
                                           const double* P0, const double* shift, const double* y, const int32_t* seg_start, int n_seg,
                                           int batch, int m, int k, int p, int T_len, double jitter, double missing_fill,
                                           size_t scratch_limit_bytes, double* logp_out, double* T_bar, double* R_bar, double* Q_bar,
                                           double* Z_bar, double* d_bar, double* h_bar, double* shift_bar, double* a0_bar, double* P0_bar,
                                           int32_t* status_io, void* stream) {
  const ObsModel obs{Z, z_batched, d, d_batched, Hdiag, h_batched, y, p, T_len, jitter, missing_fill};
  const ShockCov q{Q, q_mode};
  int rc = check_kalman_segments(batch, m, k, obs, q, seg_start, n_seg, T && R && logp_out && status_io);
  if (rc) return rc;
  if ((rc = ensure_device())) return rc;
  if (batch == 0 || T_len == 0) return DSGE_SUCCESS;
  hipStream_t st = (hipStream_t)stream;
  const SegmentedProblem s{T, R, q, obs, a0, P0, shift, seg_start, n_seg, batch, m, k};
  const size_t S = (size_t)n_seg, mm = (size_t)m * m, qw = s.q_width(), tm = (size_t)T_len * m;
  // per draw: the stored forward pass and the accumulators of Tbar and Gbar (Tbar's are counted also when the caller's T_bar serves)
  const size_t per_draw = (2 * tm * m + 2 * tm + 2 * S * mm) * sizeof(double);
  const int chunk = chunk_for(scratch_limit_bytes, per_draw, batch);
  const size_t cf = (size_t)chunk * S;
  double *Tb = nullptr, *Gb = nullptr, *ap = nullptr, *af = nullptr, *pp = nullptr, *pf = nullptr;
  SegmentChain ch;
  if ((rc = ch.declare(s, chunk, "segmented gradient", kalman_segments_grad_lds_bytes(m, p)))) return rc;
  if (!T_bar) ch.lay.add(&Tb, cf * mm);
  ch.lay.add(&Gb, cf * mm);
  ch.lay.add(&ap, chunk * tm);
  ch.lay.add(&af, chunk * tm);
  ch.lay.add(&pp, chunk * tm * m);
  ch.lay.add(&pf, chunk * tm * m);
  if ((rc = ch.reserve(s, st))) return rc;
  // every cotangent the sweep adds to, or writes for healthy draws only, starts from zero: a failed draw keeps the zeros
  const size_t fa = (size_t)batch * S;
  if (T_bar) HIP_TRY(hipMemsetAsync(T_bar, 0, sizeof(double) * fa * mm, st));
  if (Z_bar) HIP_TRY(hipMemsetAsync(Z_bar, 0, sizeof(double) * fa * p * m, st));
  if (d_bar) HIP_TRY(hipMemsetAsync(d_bar, 0, sizeof(double) * fa * p, st));
  if (h_bar) HIP_TRY(hipMemsetAsync(h_bar, 0, sizeof(double) * fa * p, st));
  if (shift_bar) HIP_TRY(hipMemsetAsync(shift_bar, 0, sizeof(double) * fa * m, st));
  if (a0_bar) HIP_TRY(hipMemsetAsync(a0_bar, 0, sizeof(double) * (size_t)batch * m, st));
  if (P0_bar) HIP_TRY(hipMemsetAsync(P0_bar, 0, sizeof(double) * (size_t)batch * mm, st));
  auto at = [](double* x, size_t off) { return x ? x + off : nullptr; };
  for (int c0 = 0; c0 < batch; c0 += chunk) {
    const size_t o = (size_t)c0, fo = o * S;
    const SegmentedProblem c = s.at(o, chunk_draws(batch, c0, chunk));
    int32_t* sc = status_io + o;
    if ((rc = ch.run(c, sc, st))) return rc;
    // (the forward pass: logp alone goes to the caller, the moments of every period into scratch)
    if ((rc = launch_kalman_segments_store(c, ch.RQR, ch.P0, logp_out + o, nullptr, ap, af, pp, pf, nullptr, nullptr, nullptr, nullptr, 0,
                                           sc, st)))
      return rc;
    double* Tbc = T_bar ? T_bar + fo * mm : Tb;
    if (!T_bar) HIP_TRY(hipMemsetAsync(Tb, 0, sizeof(double) * c.flat() * mm, st));
    if ((rc = launch_kalman_segments_grad(c, ap, af, pp, pf, Tbc, Gb, at(Z_bar, fo * p * m), at(d_bar, fo * p), at(h_bar, fo * p),
                                          at(shift_bar, fo * m), at(a0_bar, o * m), at(P0_bar, o * mm), sc, st)))
      return rc;
    if ((rc = launch_kalman_segments_grad_rq(Gb, c.R, ch.qe, (int)c.flat(), n_seg, m, k, at(R_bar, fo * m * k), at(Q_bar, fo * qw),
                                             logp_out + o, sc, st)))
      return rc;
  }
  return DSGE_SUCCESS;
}

// Joint posterior draws of the state path and the shocks (dsge_simsmooth.hpp): the smoother's forward pass and basis per chunk of
// draws, x+ of every path through the propagation kernel, then the two path kernels -- all on the caller's stream.
int dsge_simulation_smoother_batched(const double* T, const double* R, const double* Q, int q_mode, const double* Z, int z_batched,
                                     const double* d, int d_batched, const double* Hdiag, int h_batched, const double* y, int batch,
                                     int m, int k, int p, int T_len, double jitter, double missing_fill, double rank_tol,
                                     size_t scratch_limit_bytes, const double* x0, int x0_batched, const double* eps,
                                     int eps_batched, const double* eta, int eta_batched, int n_paths, double* ll_out,
                                     double* x_out, double* eps_out, int32_t* status_io, void* stream) {
  const ObsModel obs{Z, z_batched, d, d_batched, Hdiag, h_batched, y, p, T_len, jitter, missing_fill};
  const ShockCov q{Q, q_mode};
  int rc = check_simulation_smoother(batch, m, k, obs, q, T && R && status_io, n_paths, eps, eta, x_out || eps_out);
  if (rc) return rc;
  if ((rc = ensure_device())) return rc;
  if (batch == 0 || n_paths == 0 || T_len == 0) return DSGE_SUCCESS;
  hipStream_t st = (hipStream_t)stream;
  if (!(rank_tol > 0.0)) rank_tol = 1e-10;
  // per draw: the per-step filter outputs of the smoother entry (an upper bound: the means of y are not stored here), and x+,
  // a*_pred, a*_filt of every path
  const size_t tm = (size_t)T_len * m, ptm = (size_t)n_paths * tm, per_draw = (2 * tm * m + 2 * tm + 3 * ptm) * sizeof(double);
  const int chunk = chunk_for(scratch_limit_bytes, per_draw, batch);
  const size_t mm = (size_t)chunk * m * m, img = (size_t)chunk * smoother_image_doubles(m);
  double *RQR = nullptr, *P0 = nullptr, *U = nullptr, *UT = nullptr, *UR = nullptr, *pp = nullptr, *pf = nullptr;
  double *xp = nullptr, *asp = nullptr, *asf = nullptr, *ll = nullptr;
  int32_t *rank = nullptr, *snap = nullptr;
  ScratchLayout lay;
  lay.add(&RQR, mm);
  lay.add(&P0, mm);
  lay.add(&U, img);
  lay.add(&UT, img);
  lay.add(&UR, img);
  lay.add(&pp, chunk * tm * m);
  lay.add(&pf, chunk * tm * m);
  lay.add(&xp, chunk * ptm);
  lay.add(&asp, chunk * ptm);
  lay.add(&asf, chunk * ptm);
  lay.add(&rank, (size_t)chunk);
  lay.add(&snap, (size_t)chunk);
  if (!ll_out) lay.add(&ll, (size_t)chunk * T_len);
  if ((rc = lay.reserve(g_scratch_pool, st))) return rc;
  const long long eps_path = (long long)T_len * k, eps_draw = eps_batched ? n_paths * eps_path : 0;
  const long long eta_draw = eta_batched ? (long long)n_paths * T_len * p : 0, x0_draw = x0_batched ? (long long)n_paths * m : 0;
  for (int c0 = 0; c0 < batch; c0 += chunk) {
    const int nb = chunk_draws(batch, c0, chunk);
    const size_t o = (size_t)c0;
    const double *Tc = T + o * m * m, *Rc = R + o * m * k;
    const ShockCov qc = q.at(o, k);
    const ObsModel oc = obs.at(o, m);
    int32_t* sc = status_io + o;
    const double* epc = eps + o * eps_draw;
    if ((rc = assemble_rqr_p0(Tc, Rc, qc, nb, m, k, RQR, P0, sc, st))) return rc;
    if ((rc = launch_kalman_outputs(Tc, RQR, P0, oc, nb, m, ll_out ? ll_out + o * T_len : ll, nullptr, nullptr, pp, pf, 1, sc, st)))
      return rc;  // (the means of y itself are not stored: the path kernels filter y*)
    if ((rc = launch_smoother_basis(Tc, Rc, qc, nb, m, k, rank_tol, U, UT, UR, rank, sc, st))) return rc;
    if ((rc = launch_propagate(Tc, Rc, epc, eps_draw, eps_path, k, 1, 0, x0 ? x0 + o * x0_draw : nullptr, x0_draw, nullptr, 0, nullptr, nb, m,
                               k, n_paths, T_len, T_len, xp, nullptr, st)))
      return rc;
    if ((rc = launch_simulation_smoother(Tc, qc, oc, nb, m, k, n_paths, U, UT, UR, rank, pp, pf, xp, epc, eps_draw,
                                         eta ? eta + o * eta_draw : nullptr, eta_draw, asp, asf, x_out ? x_out + o * ptm : nullptr,
                                         eps_out ? eps_out + o * n_paths * eps_path : nullptr, sc, snap, st)))
      return rc;
  }
  return DSGE_SUCCESS;
}

// ---- post-solve dynamics (dsge_dynamics.hpp): simulate, impulse responses + FEVD, forecast -----------------------------------
int dsge_simulate_batched(const double* T, const double* R, const double* eps, int eps_batched, const double* x0, int x0_batched,
                          const int32_t* status, int batch, int m, int k, int n_paths, int n_steps, int n_shock_steps,
                          double* x_out, void* stream) {
  int rc = check_simulate(T, R, eps, batch, m, k, n_paths, n_steps, n_shock_steps, x_out);
  if (rc) return rc;
  if ((rc = ensure_device())) return rc;
  if (batch == 0 || n_paths == 0 || n_steps == 0) return DSGE_SUCCESS;
  const long long per_path = (long long)n_shock_steps * k;
  return launch_propagate(T, R, eps, eps_batched ? n_paths * per_path : 0, per_path, k, 1, 0, x0,
                          x0_batched ? (long long)n_paths * m : 0, nullptr, 0, status, batch, m, k, n_paths, n_steps, n_shock_steps,
                          x_out, nullptr, (hipStream_t)stream);
}

// Impulse j is column j of S: the propagation kernel entered with e_0 = S[:, j] and no shock afterwards.  Up to 16 impulses the FEVD
// is accumulated on chip by the same launch; beyond, a second pass reads the stored responses (library scratch when the caller
// wants the FEVD alone).
int dsge_irf_batched(const double* T, const double* R, const double* S, int s_batched, const double* weights, int w_batched,
                     const int32_t* status, int batch, int m, int k, int c, int n_steps, double* irf_out, double* fevd_out,
                     void* stream) {
  int rc = check_irf(T, R, S, batch, m, k, c, n_steps, irf_out, fevd_out);
  if (rc) return rc;
  if ((rc = ensure_device())) return rc;
  if (batch == 0 || c == 0 || n_steps == 0) return DSGE_SUCCESS;
  hipStream_t st = (hipStream_t)stream;
  const bool second_pass = fevd_out && c > 16;
  double* irf = irf_out;
  if (second_pass && !irf) {
    ScratchLayout lay;
    lay.add(&irf, (size_t)batch * c * n_steps * m);
    if ((rc = lay.reserve(g_scratch_pool, st))) return rc;
  }
  const long long w_draw = w_batched ? c : 0;
  if ((rc = launch_propagate(T, R, S, s_batched ? (long long)k * c : 0, 1, 0, c, S ? 0 : 1, nullptr, 0, weights, w_draw, status, batch, m,
                             k, c, n_steps, 1, irf, second_pass ? nullptr : fevd_out, st)))
    return rc;
  if (second_pass) return launch_fevd(irf, weights, w_draw, status, batch, m, c, n_steps, fevd_out, st);
  return DSGE_SUCCESS;
}

// ---- second-order dynamics (dsge_pruned.hpp): pruned simulation and generalised impulse responses -----------------------------
// The panel of the second-order blocks is library scratch, packed per draw; a batch whose panels exceed PRUNED_SCRATCH_BYTES runs
// in contiguous chunks of draws, one after the other on the caller's stream.
static constexpr size_t PRUNED_SCRATCH_BYTES = (size_t)1 << 30;
static int pruned_run(const PrunedProblem& p, int batch, const double* eps, const double* xf0, const double* xs0, const double* imp,
                      const int32_t* status, double* x_out, double* xf_out, double* xs_out, double* girf_out, hipStream_t st) {
  const size_t pd = pruned_panel_doubles(p.n, p.s, p.k);
  const int chunk = chunk_for(PRUNED_SCRATCH_BYTES, pd * sizeof(double), batch);
  double* panel = nullptr;
  ScratchLayout lay;
  lay.add(&panel, (size_t)chunk * pd);
  int rc;
  if ((rc = lay.reserve(g_scratch_pool, st))) return rc;
  const size_t n = p.n, s = p.s, k = p.k, sim = (size_t)p.n_paths * p.n_steps * n, gi = (size_t)p.c * p.n_steps * n;
  for (int c0 = 0; c0 < batch; c0 += chunk) {
    const int nb = chunk_draws(batch, c0, chunk);
    const size_t o = (size_t)c0;
    PrunedProblem q = p;
    q.T += o * n * n; q.R += o * n * k; q.gyy += o * n * s * s; q.gyu += o * n * s * k; q.guu += o * n * k * k; q.gss += o * n;
    if ((rc = launch_pruned(q, nb, eps ? eps + o * p.eps_draw : nullptr, xf0 ? xf0 + o * p.x0_draw : nullptr,
                            xs0 ? xs0 + o * p.x0_draw : nullptr, imp ? imp + o * p.imp_draw : nullptr, status ? status + o : nullptr,
                            panel, x_out ? x_out + o * sim : nullptr, xf_out ? xf_out + o * sim : nullptr,
                            xs_out ? xs_out + o * sim : nullptr, girf_out ? girf_out + o * gi : nullptr, st)))
      return rc;
  }
  return DSGE_SUCCESS;
}

int dsge_simulate_pruned_batched(const double* T, const double* R, const double* gyy, const double* gyu, const double* guu,
                                 const double* gss, const int32_t* state_idx, int n_state, const double* eps, int eps_batched,
                                 const double* xf0, const double* xs0, int x0_batched, const int32_t* status, int batch, int n, int k,
                                 int n_paths, int n_steps, int n_shock_steps, double* x_out, double* xf_out, double* xs_out,
                                 void* stream) {
  int rc = check_pruned(T, R, gyy, gyu, guu, gss, state_idx, n_state, eps, batch, n, k, n_paths, n_steps, n_shock_steps,
                        x_out || xf_out || xs_out);
  if (rc) return rc;
  if ((rc = ensure_device())) return rc;
  if (batch == 0 || n_paths == 0 || n_steps == 0) return DSGE_SUCCESS;
  const PrunedProblem p{T, R, gyy, gyu, guu, gss, state_idx, n, n_state, k, 0, n_paths, n_steps, n_shock_steps,
                        eps_batched ? (long long)n_paths * n_shock_steps * k : 0, x0_batched ? (long long)n_paths * n : 0, 0};
  return pruned_run(p, batch, eps, xf0, xs0, nullptr, status, x_out, xf_out, xs_out, nullptr, (hipStream_t)stream);
}

int dsge_girf_pruned_batched(const double* T, const double* R, const double* gyy, const double* gyu, const double* guu,
                             const double* gss, const int32_t* state_idx, int n_state, const double* S_imp, int s_batched, int c,
                             const double* eps, int eps_batched, const double* xf0, const double* xs0, int x0_batched,
                             const int32_t* status, int batch, int n, int k, int n_paths, int n_steps, int n_shock_steps,
                             double* girf_out, void* stream) {
  int rc = check_girf_pruned(T, R, gyy, gyu, guu, gss, state_idx, n_state, S_imp, c, eps, batch, n, k, n_paths, n_steps, n_shock_steps,
                             girf_out);
  if (rc) return rc;
  if ((rc = ensure_device())) return rc;
  if (batch == 0 || c == 0 || n_steps == 0) return DSGE_SUCCESS;
  const PrunedProblem p{T, R, gyy, gyu, guu, gss, state_idx, n, n_state, k, c, n_paths, n_steps, n_shock_steps,
                        eps_batched ? (long long)n_paths * n_shock_steps * k : 0, x0_batched ? (long long)n_paths * n : 0,
                        s_batched ? (long long)k * c : 0};
  return pruned_run(p, batch, eps, xf0, xs0, S_imp, status, nullptr, nullptr, nullptr, girf_out, (hipStream_t)stream);
}

// ---- historical shock decomposition (dsge_shock_decomp.hpp): one launch on the caller's stream, no scratch -------------------------
int dsge_shock_decomposition_batched(const double* T, const double* R, const double* eps, const double* x,
                                     const int32_t* group_of_shock, int n_groups, const int32_t* var_idx, int n_out, const double* Z,
                                     int z_batched, const int32_t* status, int batch, int m, int k, int p, int n_paths, int T_len,
                                     int remainder, double* contrib_out, double* obs_out, void* stream) {
  int rc = check_shock_decomp(T, R, eps, x, group_of_shock, n_groups, var_idx, n_out, Z, batch, m, k, p, n_paths, T_len, remainder,
                              contrib_out, obs_out);
  if (rc) return rc;
  if ((rc = ensure_device())) return rc;
  if (batch == 0 || n_paths == 0) return DSGE_SUCCESS;
  return launch_shock_decomp(T, R, eps, x, group_of_shock, n_groups, var_idx, n_out, Z, z_batched, status, batch, m, k, Z ? p : 0,
                             n_paths, T_len, remainder, contrib_out, obs_out, (hipStream_t)stream);
}

// ---- conditional forecast (dsge_condfc.hpp): two launches on the caller's stream; the scratch holds per-draw setup data only ----
int dsge_conditional_forecast_batched(const double* T, const double* R, const double* Q, int q_mode, const double* Z, int z_batched,
                                      const double* d, int d_batched, const double* x0, int x0_batched, int x0_paths,
                                      const double* eps, int eps_batched, const int32_t* cond_t, const int32_t* cond_j, int n_cond,
                                      const double* cond_val, int cv_batched, int cv_paths, const int32_t* free_shock,
                                      int32_t* status_io, int batch, int m, int k, int p, int n_paths, int n_steps,
                                      int n_shock_steps, double rank_tol, double* x_out, double* eps_out, double* obs_out,
                                      void* stream) {
  CondFcProblem c{batch, m, k, p, n_paths, n_steps, n_shock_steps, n_cond, x0_batched, x0_paths, eps_batched, cv_batched, cv_paths,
                  cond_t, cond_j, free_shock, rank_tol};
  const ShockCov q{Q, q_mode};
  int rc = check_conditional_forecast(c, T, R, q, Z, x0, eps, cond_val, x_out, eps_out, obs_out);
  if (rc) return rc;
  if ((rc = ensure_device())) return rc;
  if (batch == 0) return DSGE_SUCCESS;
  hipStream_t st = (hipStream_t)stream;
  double *chol = nullptr, *psi = nullptr, *psiq = nullptr;
  int32_t* flag = nullptr;
  if (n_cond > 0) {
    const size_t b = (size_t)batch, lag = (size_t)(c.t_max + 1) * p * k;
    ScratchLayout lay;
    lay.add(&chol, b * n_cond * (n_cond + 1) / 2);
    lay.add(&psi, b * lag);
    lay.add(&psiq, b * lag);
    lay.add(&flag, b);
    if ((rc = lay.reserve(g_scratch_pool, st))) return rc;
  }
  return launch_condfc(c, T, R, q, Z, z_batched, d, d_batched, x0, eps, cond_val, status_io, chol, psi, psiq, flag, x_out, eps_out,
                       obs_out, st);
}

// ---- spectral moments (dsge_spectral.hpp): two launches per chunk of draws on the caller's stream; the scratch holds the
// per-frequency F_n of the chunk's draws and a flag per draw ----
int dsge_spectral_moments_batched(const double* T, const double* R, const double* Q, int q_mode, const double* Z, int z_batched,
                                  const double* Hdiag, int h_batched, const double* gain, int batch, int m, int k, int p,
                                  int n_grid, int n_lags, int correlation, double rank_tol, size_t scratch_limit_bytes,
                                  double* acov_out, double* spectrum_out, int32_t* status_io, void* stream) {
  SpectralProblem s{batch, m, k, p, n_grid, n_lags, correlation, z_batched, h_batched, rank_tol};
  const ShockCov q{Q, q_mode};
  int rc = check_spectral_moments(s, T, R, q, Z, Hdiag, acov_out, spectrum_out);
  if (rc) return rc;
  if ((rc = ensure_device())) return rc;
  if (batch == 0) return DSGE_SUCCESS;
  hipStream_t st = (hipStream_t)stream;
  const size_t dim = Z ? p : m, nf = (size_t)n_grid / 2 + 1, dd = dim * dim;
  const size_t per_draw = acov_out ? 2 * nf * dd * sizeof(double) : sizeof(int32_t);
  const int chunk = chunk_for(scratch_limit_bytes, per_draw, batch);
  double* F = nullptr;
  int32_t* flag = nullptr;
  ScratchLayout lay;
  if (acov_out) lay.add(&F, (size_t)chunk * 2 * nf * dd);
  lay.add(&flag, (size_t)chunk);
  if ((rc = lay.reserve(g_scratch_pool, st))) return rc;
  for (int c0 = 0; c0 < batch; c0 += chunk) {
    const size_t o = (size_t)c0;
    s.batch = chunk_draws(batch, c0, chunk);
    if ((rc = launch_spectral(s, T + o * m * m, R + o * m * k, q.at(o, k), Z && z_batched ? Z + o * p * m : Z,
                              Hdiag && h_batched ? Hdiag + o * p : Hdiag, gain, status_io ? status_io + o : nullptr, flag, F,
                              acov_out ? acov_out + o * (n_lags + 1) * dd : nullptr,
                              spectrum_out ? spectrum_out + o * nf * dd * 2 : nullptr, st)))
      return rc;
  }
  return DSGE_SUCCESS;
}

// ---- anticipated shocks (dsge_anticipated.hpp): two launches on the caller's stream; the scratch holds G and a flag per draw, and
// the parked anticipation term only when neither x_out nor w_out is there to park it in ----
int dsge_anticipated_paths_batched(const double* B, const double* C, const double* T, const double* R, const double* eps,
                                   int eps_batched, int mode, int n_lead, const double* x0, int x0_batched, int x0_paths,
                                   const double* Z, int z_batched, const double* d, int d_batched, int32_t* status_io, int batch,
                                   int n, int k, int p, int n_paths, int n_steps, int n_shock_steps, double rank_tol, double* x_out,
                                   double* w_out, double* obs_out, double* G_out, void* stream) {
  const AnticipatedProblem c{batch, n, k, p, n_paths, n_steps, n_shock_steps, mode, n_lead, eps_batched, x0_batched, x0_paths,
                             z_batched, d_batched, rank_tol};
  int rc = check_anticipated_paths(c, B, C, T, R, eps, Z, x_out, w_out, obs_out, G_out);
  if (rc) return rc;
  if ((rc = ensure_device())) return rc;
  if (batch == 0 || n_paths == 0 || n_steps == 0) return DSGE_SUCCESS;
  hipStream_t st = (hipStream_t)stream;
  const size_t b = (size_t)batch;
  double *G = G_out, *park = w_out ? w_out : x_out;
  int32_t* flag = nullptr;
  ScratchLayout lay;
  if (!G) lay.add(&G, b * n * n);
  lay.add(&flag, b);
  if (!park && obs_out) lay.add(&park, b * n_paths * n_steps * n);
  if ((rc = lay.reserve(g_scratch_pool, st))) return rc;
  return launch_anticipated(c, B, C, T, R, eps, x0, Z, d, status_io, G, G_out != nullptr, flag, park, x_out, w_out, obs_out, st);
}

// ---- occasionally binding bound (dsge_obc.hpp): a chain of launches on the caller's stream (launch_obc.hip); the scratch holds G and
// a flag per draw, the unit shocks, Mz, the parked terms of a chunk of unit paths, e', max|q| and the bits per path, and the paths
// themselves when x_out is not there to hold them ----
int dsge_constrained_paths_batched(const double* B, const double* C, const double* T, const double* R, const double* eps,
                                   int eps_batched, const double* x0, int x0_batched, int x0_paths, const double* Z, int z_batched,
                                   const double* d, int d_batched, const double* c_row, int c_batched, const double* bound,
                                   int bound_batched, int shock, int horizon, int max_iter, int32_t* status_io, int batch, int n, int k,
                                   int p, int n_paths, int n_steps, int n_shock_steps, double rank_tol, double* x_out, double* w_out,
                                   double* obs_out, double* nu_out, double* gap_out, double* Mz_out, int32_t* path_status_out,
                                   int32_t* iters_out, void* stream) {
  const ConstrainedProblem c{{batch, n, k, p, n_paths, n_steps, n_shock_steps, DSGE_ANT_PERFECT_FORESIGHT, 0, eps_batched, x0_batched,
                              x0_paths, z_batched, d_batched, rank_tol},
                             c_batched, bound_batched, shock, horizon, max_iter};
  const void* other = nu_out ? (const void*)nu_out : gap_out ? (const void*)gap_out : Mz_out ? (const void*)Mz_out
                      : path_status_out ? (const void*)path_status_out : (const void*)iters_out;
  int rc = check_constrained_paths(c, B, C, T, R, eps, Z, c_row, bound, x_out, w_out, obs_out, other);
  if (rc) return rc;
  if ((rc = ensure_device())) return rc;
  if (batch == 0 || n_paths == 0 || n_steps == 0) return DSGE_SUCCESS;
  hipStream_t st = (hipStream_t)stream;
  const size_t b = (size_t)batch, np = (size_t)n_paths, H = (size_t)horizon;
  const size_t nsp = (size_t)n_shock_steps > H ? (size_t)n_shock_steps : H;
  ConstrainedBuffers buf{B, C, T, R, eps, x0, Z, d, c_row, bound, status_io, x_out, w_out, obs_out, nu_out, gap_out, Mz_out,
                         path_status_out, iters_out};
  buf.xbuf = x_out;
  ScratchLayout lay;
  lay.add(&buf.G, b * n * n);
  lay.add(&buf.flag, b);
  lay.add(&buf.unit, H * H * k);
  lay.add(&buf.mzt, b * H * H);
  lay.add(&buf.mzpark, (size_t)constrained_chunk(batch, n, horizon) * H * H * n);
  if (!buf.xbuf) lay.add(&buf.xbuf, b * np * n_steps * n);
  lay.add(&buf.eps2, b * np * nsp * k);
  lay.add(&buf.qmax, b * np);
  lay.add(&buf.pstat, b * np);
  if ((rc = lay.reserve(g_scratch_pool, st))) return rc;
  return launch_constrained(c, buf, st);
}

// ---- stochastic simulation at the bound (dsge_obc_sim.hpp): a chain of launches on the caller's stream (launch_obc_sim.hip); the
// scratch holds what the Mz chain of the entry above needs (G, a flag per draw, the unit shocks, Mz, the parked terms of a chunk of
// unit paths), the tables Cq and W per draw and the bits per path ----
int dsge_constrained_simulate_batched(const double* B, const double* C, const double* T, const double* R, const double* eps,
                                      int eps_batched, const double* x0, int x0_batched, int x0_paths, const double* Z, int z_batched,
                                      const double* d, int d_batched, const double* c_row, int c_batched, const double* bound,
                                      int bound_batched, int shock, int horizon, int max_iter, int32_t* status_io, int batch, int n,
                                      int k, int p, int n_paths, int n_steps, int n_shock_steps, double rank_tol, double* x_out,
                                      double* obs_out, double* gap_out, double* shadow_out, double* plan_out, int32_t* duration_out,
                                      int32_t* iters_out, double* Mz_out, int32_t* path_status_out, int32_t* fail_step_out,
                                      void* stream) {
  const ConstrainedProblem c{{batch, n, k, p, n_paths, n_steps, n_shock_steps, DSGE_ANT_PERFECT_FORESIGHT, 0, eps_batched, x0_batched,
                              x0_paths, z_batched, d_batched, rank_tol},
                             c_batched, bound_batched, shock, horizon, max_iter};
  const void* outs[] = {gap_out, shadow_out, plan_out, duration_out, iters_out, Mz_out, path_status_out, fail_step_out};
  const void* other = nullptr;
  for (const void* o : outs) other = other ? other : o;
  int rc = check_constrained_simulate(c, B, C, T, R, eps, Z, c_row, bound, x_out, obs_out, other);
  if (rc) return rc;
  if ((rc = ensure_device())) return rc;
  if (batch == 0 || n_paths == 0 || n_steps == 0) return DSGE_SUCCESS;
  hipStream_t st = (hipStream_t)stream;
  const size_t b = (size_t)batch, np = (size_t)n_paths, H = (size_t)horizon;
  ConstrainedSimBuffers buf{};
  buf.mz = ConstrainedBuffers{B, C, T, R, eps, x0, Z, d, c_row, bound, status_io};
  buf.x_out = x_out; buf.obs_out = obs_out; buf.gap_out = gap_out; buf.shadow_out = shadow_out; buf.plan_out = plan_out;
  buf.duration_out = duration_out; buf.iters_out = iters_out; buf.Mz_out = Mz_out; buf.path_status_out = path_status_out;
  buf.fail_step_out = fail_step_out;
  ScratchLayout lay;
  lay.add(&buf.mz.G, b * n * n);
  lay.add(&buf.mz.flag, b);
  lay.add(&buf.mz.unit, H * H * k);
  lay.add(&buf.mz.mzt, b * H * H);
  lay.add(&buf.mz.mzpark, (size_t)constrained_chunk(batch, n, horizon) * H * H * n);
  lay.add(&buf.cq, b * H * n);
  lay.add(&buf.wt, b * H * n);
  lay.add(&buf.pstat, b * np);
  if ((rc = lay.reserve(g_scratch_pool, st))) return rc;
  return launch_constrained_sim(c, buf, st);
}

int dsge_forecast_batched(const double* T, const double* R, const double* Q, int q_mode, const double* Z, int z_batched,
                          const double* d, int d_batched, const double* Hdiag, int h_batched, const double* a0, const double* P0,
                          const int32_t* status, int batch, int m, int k, int p, int n_steps, double* a_out, double* p_out,
                          int full_cov, double* y_out, double* f_out, void* stream) {
  const ObsModel obs{Z, z_batched, d, d_batched, Hdiag, h_batched, nullptr, p, 0, 0.0, 0.0};  // (no panel: the moments only)
  const ShockCov q{Q, q_mode};
  int rc = check_forecast(T, R, q, obs, a0, batch, m, k, n_steps, a_out, p_out, y_out, f_out);
  if (rc) return rc;
  if ((rc = ensure_device())) return rc;
  if (batch == 0 || n_steps == 0) return DSGE_SUCCESS;
  return launch_forecast(T, R, q, obs, a0, P0, status, batch, m, k, n_steps, a_out, p_out, full_cov, y_out, f_out,
                         (hipStream_t)stream);
}

int dsge_kalman_logp_batched(const double* T, const double* R, const double* Q, int q_mode, const double* Z,
                             int z_batched, const double* d, int d_batched, const double* Hdiag, int h_batched,
                             const double* y, int batch, int m, int k, int p, int T_len, double jitter,
                             double missing_fill, int n_state_hint, int z_selector_hint, double* logp_out,
                             int32_t* status_io, void* stream) {
  const ObsModel obs{Z, z_batched, d, d_batched, Hdiag, h_batched, y, p, T_len, jitter, missing_fill};
  const ShockCov q{Q, q_mode};
  int rc = check_kalman(batch, m, k, obs, q, T && R && logp_out && status_io);
  if (rc) return rc;
  if ((rc = ensure_device())) return rc;
  if (batch == 0) return DSGE_SUCCESS;
  hipStream_t st = (hipStream_t)stream;
  const size_t mm = (size_t)batch * m * m;
  double *RQR = nullptr, *P0 = nullptr;
  ScratchLayout lay;
  lay.add(&RQR, mm);
  lay.add(&P0, mm);
  if ((rc = lay.reserve(g_scratch_pool, st))) return rc;
  if ((rc = assemble_rqr(R, q, batch, m, k, RQR, status_io, st))) return rc;
  return launch_kalman(T, RQR, P0, 0, obs, batch, m, n_state_hint, z_selector_hint, logp_out, status_io, st);
}

// The scratch of the fused pipeline for one batch, declared once for both of its routes: pipeline_unchunked and pipeline_big
// take their pointers from it, the chunked entry asks it for the bytes of one chunk first.  T, R and the iteration counts are
// the caller's outputs where given.
struct PipelineScratch {
  double *Tw, *Rw, *RQR, *P0;
  int32_t *eu_w, *it_w;
  int32_t *key_w, *vst_w;     // n <= 64: dispatch key of the Kalman launch; status words of an overlapped gensys verdict
  unsigned long long* cm_w;   // n <= 64: non-zero columns of T, from the solver
  double *T_r, *R_r, *Z_r;    // n > 64: the gathered model at 64 filtered variables
  int32_t* park_w;            // n > 64
};
static void pipeline_declare(ScratchLayout& lay, PipelineScratch& s, int batch, int n, int k, int z_batched, double* T_out,
                             double* R_out, int32_t* n_iter_out) {
  const size_t b = (size_t)batch, nn = b * n * n, uu = b * 64 * 64;
  s = PipelineScratch{};
  if (!(s.Tw = T_out)) lay.add(&s.Tw, nn);
  if (!(s.Rw = R_out)) lay.add(&s.Rw, b * n * k);
  if (big_size(n)) {  // pipeline_big
    lay.add(&s.T_r, uu);
    lay.add(&s.R_r, b * 64 * k);
    lay.add(&s.Z_r, (z_batched ? b : 1) * DSGE_MAX_P * 64);  // (not p: the chunked entry sizes a chunk before p is checked)
    lay.add(&s.RQR, uu);
    lay.add(&s.P0, uu);
    if (!(s.it_w = n_iter_out)) lay.add(&s.it_w, b);
    lay.add(&s.park_w, b);
    lay.add(&s.eu_w, b * 3);  // (gensys: the certificate's eu codes)
    return;
  }
  lay.add(&s.RQR, nn);
  lay.add(&s.P0, nn);
  lay.add(&s.eu_w, b * 3);
  if (!(s.it_w = n_iter_out)) lay.add(&s.it_w, b);  // cycle-reduction iterations
  lay.add(&s.key_w, b);
  lay.add(&s.cm_w, b);
  lay.add(&s.vst_w, b);
}

// ---- 65 .. 96 variables (dsge_big.hpp): cycle reduction with one workgroup per draw, then the EXISTING filter kernels on the
// model restricted to F = {state variables} u {observed variables}: x_t[F] = T[F, F] x_{t-1}[F] + R[F, :] eps_t is exact because
// every column of T outside the state variables is zero (T = -(B + C T)^-1 A inherits the zero columns of A), and y_t reads
// x_t[F] only.  |F| <= 64 or DSGE_ERR_TOO_LARGE.  Measuring F synchronises the stream once per call.
static int pipeline_big(const double* A, const double* B, const double* C, const double* D, const ShockCov& q, const ObsModel& o,
                        int batch, int n, int k, int solver, bool park_failures, double tol, int max_iter, int z_selector_hint,
                        double* logp_out, int32_t* status_out, double* T_out, double* R_out, double* resid_out, int32_t* n_iter_out,
                        hipStream_t st, int reps, float* ms_out, void* scratch_slice) {
  const int p = o.p;
  int rc;
  ScratchLayout lay;
  PipelineScratch s;
  pipeline_declare(lay, s, batch, n, k, o.z_batched, T_out, R_out, n_iter_out);
  if ((rc = lay.reserve(g_scratch_pool, st, scratch_slice))) return rc;
  double *Tw = s.Tw, *Rw = s.Rw, *T_r = s.T_r, *R_r = s.R_r, *Z_r = s.Z_r, *RQR = s.RQR, *P0 = s.P0;
  int32_t *it_w = s.it_w, *park_w = s.park_w, *eu_w = s.eu_w;
  // F depends on A and Z only: measured FIRST (one small launch, a 72-byte read-back, one stream synchronisation per call -- not
  // per repetition), so that a model with more than 64 state + observed variables is refused before anything is enqueued and
  // before any output of this call is touched (DSGE_ERR_TOO_LARGE: "nothing computed", include/dsge_hip.h)
  unsigned char idx[64];
  int u = 0, ns = 0;
  if ((rc = big_filtered_variables(A, o.Z, o.z_batched, batch, n, p, st, idx, &u, &ns))) return rc;
  if (u > 64)
    return fail(DSGE_ERR_TOO_LARGE, "solve + Kalman with n > 64: " + std::to_string(u) +
                                        " state and observed variables, the filter kernels take at most 64");
  if (u < 1) return fail(DSGE_ERR_INVALID, "solve + Kalman with n > 64: no state and no observed variable");
  EventGuard ev[4];
  float acc_ms[3] = {0.f, 0.f, 0.f};
  if (ms_out)
    for (auto& e : ev) HIP_TRY(e.create());
  const int n_rep = ms_out ? reps : 1;
  for (int rep = 0; rep < n_rep; ++rep) {
    if (ms_out) HIP_TRY(hipEventRecord(ev[0], st));
    const bool scan = solver == DSGE_SOLVER_SCAN_CYCLE_REDUCTION;
    // R from the final elimination of the (njit-rule) iteration; the scan variant and a requested residual take the explicit
    // selection R = -(C T + B)^-1 D
    // (nor with the reference's default gating: a failed draw carries T = 0 on, and its R = -(C 0 + B)^-1 D comes from the
    // explicit selection, which runs after the statuses have been parked)
    const bool fuse_R = !scan && !resid_out && !park_failures;
    if (solver == DSGE_SOLVER_GENSYS) {
      // gensys at this size = the doubling iteration + the certificate of eu = [1, 1, 0] (gensys_certify_big_kernel), R from the
      // certificate's elimination; a draw without the certificate is a failed draw (no ordered QZ beyond 64 variables)
      if ((rc = launch_gensys_big(A, B, C, D, batch, n, k, tol, Tw, Rw, eu_w, status_out, it_w, st))) return rc;
      if (resid_out && (rc = launch_selection_big(A, B, C, D, Tw, batch, n, k, nullptr, resid_out, status_out, st))) return rc;
    } else {
    if ((rc = launch_cr_big(A, B, C, batch, n, max_iter, tol, Tw, status_out, it_w, st, scan ? 1 : 0, fuse_R ? D : nullptr, k,
                            fuse_R ? Rw : nullptr)))
      return rc;
    if (park_failures && (rc = launch_status_park(status_out, park_w, batch, 0, st))) return rc;
    if (!fuse_R && (rc = launch_selection_big(A, B, C, D, Tw, batch, n, k, Rw, resid_out, status_out, st))) return rc;
    }
    if (ms_out) HIP_TRY(hipEventRecord(ev[1], st));
    if ((rc = launch_big_compress(Tw, Rw, o.Z, o.z_batched, batch, n, k, p, idx, u, T_r, R_r, Z_r, st))) return rc;
    const int ns_hint = (ns > 0 && ns < u) ? ns : 0;
    const bool fold_rqr = !park_failures && q.diag() && kalman_folds_rqr(u, p, k, ns_hint, z_selector_hint);
    if (fold_rqr)
      rc = DSGE_SUCCESS;
    else if (q.diag() && k <= 16)
      rc = launch_rqr(R_r, q.Q, q.batched(), batch, u, k, status_out, RQR, st);
    else
      rc = assemble_rqr(R_r, q, batch, u, k, RQR, status_out, st);
    if (rc) return rc;
    if (ms_out) HIP_TRY(hipEventRecord(ev[2], st));
    const int32_t* okey = (opt().kalman_order == 1) ? it_w : nullptr;
    ObsModel o_r = o;  // the observation model on the gathered variables
    o_r.Z = Z_r;
    if ((rc = launch_kalman(T_r, RQR, P0, 0, o_r, batch, u, ns_hint, z_selector_hint, logp_out, status_out, st, okey,
                            fold_rqr ? R_r : nullptr, q, k)))
      return rc;
    if (park_failures && (rc = launch_status_park(status_out, park_w, batch, 1, st))) return rc;
    if (ms_out) {
      HIP_TRY(hipEventRecord(ev[3], st));
      HIP_TRY(hipEventSynchronize(ev[3]));
      for (int i = 0; i < 3; ++i) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
        acc_ms[i] += ms;
      }
    }
  }
  if (ms_out)
    for (int i = 0; i < 3; ++i) ms_out[i] = acc_ms[i] / (float)n_rep;
  return DSGE_SUCCESS;
}

}  // extern "C"

// (declared in dsge_host.hpp: the fused host twin calls it chunk by chunk)
int dsge_host::pipeline_unchunked(const double* A, const double* B, const double* C, const double* D, const ShockCov& q,
                                  const ObsModel& o, int batch, int n, int k, int solver, double tol, int max_iter, int n_state_hint,
                                  int z_selector_hint, int n_lead_hint, double* logp_out, int32_t* status_out, double* T_out,
                                  double* R_out, double* resid_out, int32_t* n_iter_out, hipStream_t st, int reps, float* ms_out,
                                  void* scratch_slice) {
  const bool zero_T_on_failure = (solver & DSGE_SOLVER_FLAG_ZERO_T_ON_FAILURE) != 0;
  solver &= ~DSGE_SOLVER_FLAG_ZERO_T_ON_FAILURE;
  const bool is_cr = solver == DSGE_SOLVER_CYCLE_REDUCTION || solver == DSGE_SOLVER_SCAN_CYCLE_REDUCTION;
  const bool park_failures = zero_T_on_failure && is_cr;
  const int p = o.p;
  int rc;
  if ((rc = ensure_device())) return rc;
  if (batch == 0) return DSGE_SUCCESS;
  if (big_size(n))
    return pipeline_big(A, B, C, D, q, o, batch, n, k, solver, park_failures, tol, max_iter, z_selector_hint, logp_out, status_out,
                        T_out, R_out, resid_out, n_iter_out, st, reps, ms_out, scratch_slice);

  ScratchLayout lay;
  PipelineScratch s;
  pipeline_declare(lay, s, batch, n, k, o.z_batched, T_out, R_out, n_iter_out);
  // (scratch_slice: a slice of an arena the caller reserved -- chunks in flight on several streams)
  if ((rc = lay.reserve(g_scratch_pool, st, scratch_slice))) return rc;
  double *Tw = s.Tw, *Rw = s.Rw, *RQR = s.RQR, *P0 = s.P0;
  int32_t *eu_w = s.eu_w, *it_w = s.it_w, *key_w = s.key_w, *vst_w = s.vst_w;
  unsigned long long* cm_w = s.cm_w;

  EventGuard ev[4];
  float acc_ms[3] = {0.f, 0.f, 0.f};
  if (ms_out)
    for (auto& e : ev) HIP_TRY(e.create());
  const int n_rep = ms_out ? reps : 1;
  for (int rep = 0; rep < n_rep; ++rep) {
    if (ms_out) HIP_TRY(hipEventRecord(ev[0], st));
    // Cycle reduction (njit semantics) can hand back R from its final elimination (A1_hat = B + C T at convergence);
    // the explicit R = -(C T + B)^-1 D of the assemble kernel is kept whenever the caller wants the policy residual.
    const bool fuse_R = (solver == DSGE_SOLVER_CYCLE_REDUCTION) && !resid_out && opt().cr_fused_selection && !park_failures;
    bool have_colmask = false;
    int gensys_key = 0;  // 1: the gensys launches have written the Kalman dispatch key
    const int32_t* gensys_qz_marks = nullptr;  // gensys by spectral division: Rw already holds R of the unmarked draws
    dsge_host::GensysOverlap gov;              // ... with the verdict on a second stream (used = 1: join, merge, second filter pass below)
    ForkGuard verdict_guard{nullptr, st};      // (armed in front of launch_gensys: joins the verdict on every return before the join below)
    if (is_cr) {
      int deflated = 0;
      // static variables deflated first (the iteration then runs on n - h variables); not when the caller asks for the
      // iteration counts or the residual, whose contract is the full-size iteration
      // (round 16) T and R in the arena: the filter below is their only reader, and it reads the states and the observed variables
      // only -- the one-launch kernel is told the observation model and leaves the static rows of a draw that observes none of
      // its deflated variables at zero (dsge_cr_fused.hpp, phase 3).  A caller who receives T or R gets every row.
      const bool rows_unread = g_cr_static_rows_mode == 2 || (g_cr_static_rows_mode == 0 && !T_out && !R_out);
      const ObsModel* skip_obs = (rows_unread && o.Z && p >= 1 && p <= 8) ? &o : nullptr;
      if (fuse_R && !n_iter_out && (rc = launch_cr_deflated(A, B, C, D, batch, n, k, max_iter, tol, Tw, Rw, status_out, it_w, st,
                                                            &deflated, cm_w, skip_obs)))
        return rc;
      have_colmask = deflated == 2;
      if (!deflated)
        rc = launch_cr(A, B, C, batch, n, max_iter, tol, Tw, status_out, it_w, st,
                       solver == DSGE_SOLVER_SCAN_CYCLE_REDUCTION ? 1 : 0, fuse_R ? D : nullptr, k, fuse_R ? Rw : nullptr);
    } else if (solver == DSGE_SOLVER_GENSYS) {
      if (n_iter_out) HIP_TRY(hipMemsetAsync(n_iter_out, 0, sizeof(int32_t) * batch, st));
      // Round 6: gensys by spectral division with the VERDICT -- certificate, compaction, the ordered QZ of the draws without one:
      // 0.38 ms + six (mostly empty) launches per 4096 draws -- on a second stream NEXT to the filter: the filter of every draw
      // starts behind the doubling iteration with that iteration's T and R; afterwards the draws the verdict re-solved are filtered
      // again (second passes) and the ones it rejected get their status and logp = -inf.  A certified draw -- every draw of an
      // estimation run -- is filtered once, with exactly the inputs of the serial order.  Only in the plain fused evaluation
      // (no residual, no profiling, R folded into the filter, not while the caller captures the stream); dsge_options.
      // gensys_doubling = 3 keeps the verdict on the caller's stream.
      hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
      const bool capturing = (hipStreamIsCapturing(st, &cap) == hipSuccess) && cap != hipStreamCaptureStatusNone;
      const bool want_overlap = opt().gensys_doubling == 1 && !ms_out && !resid_out && !park_failures && !capturing && batch >= 256 &&
                                q.diag() && n <= 64 && kalman_folds_rqr(n, p, k, n_state_hint, z_selector_hint);
      if (want_overlap) {
        gov.side = verdict_guard.side = &t_verdict;
        gov.status = vst_w;
      }
      rc = launch_gensys(A, B, C, batch, n, tol, n_lead_hint, Tw, eu_w, status_out, st, nullptr,
                         (opt().kalman_order != 0 && batch >= 512) ? key_w : nullptr, &gensys_key, D, k, Rw, n_state_hint,
                         &gensys_qz_marks, want_overlap ? &gov : nullptr);
    } else {
      HIP_TRY(hipMemsetAsync(status_out, 0, sizeof(int32_t) * batch, st));
      if (n_iter_out) HIP_TRY(hipMemsetAsync(n_iter_out, 0, sizeof(int32_t) * batch, st));
      rc = launch_bdirect(A, B, D, batch, n, k, Tw, Rw, st);
    }
    if (rc) return rc;
    if (park_failures) {  // failed draws carry T = 0 on as ordinary draws (the column-mask buffer is free: no deflated solve in this mode)
      if ((rc = launch_status_park(status_out, (int32_t*)cm_w, batch, 0, st))) return rc;
    }
    if (ms_out) HIP_TRY(hipEventRecord(ev[1], st));
    // backward_direct already produced R; the assemble kernel recomputes it from the same
    // formula (C T + B = B when C == 0), which keeps a single code path for resid/RQR/P0.
    // sym(R Q R') inside the filter kernel (its retained block only) when the fast selector kernel takes the draws
    // (round 4: also behind the explicit selection of gensys / backward-direct / a requested residual -- the assemble launch then
    // forms R (and the residual) only: no 40 x 40 product, no 51 MB of R Q R' through HBM per 4096 draws)
    const bool fold_rqr = !park_failures && q.diag() && n <= 64 && kalman_folds_rqr(n, p, k, n_state_hint, z_selector_hint);
    if (fold_rqr && fuse_R)
      rc = DSGE_SUCCESS;
    else if (fold_rqr && gov.used)
      rc = DSGE_SUCCESS;  // (R of the draws the verdict re-solves: behind the join, below)
    else if (fold_rqr)
      rc = assemble_selection(A, B, C, D, Tw, batch, n, k, Rw, resid_out, status_out, st, resid_out ? nullptr : gensys_qz_marks);
    else if (fuse_R && q.diag() && k <= 16 && n <= 64)
      rc = launch_rqr(Rw, q.Q, q.batched(), batch, n, k, status_out, RQR, st);  // (RQR_KMAX = 16)
    else if (fuse_R)
      rc = assemble_rqr(Rw, q, batch, n, k, RQR, status_out, st);
    else
      rc = assemble_selection_rqr(A, B, C, D, Tw, q, batch, n, k, Rw, resid_out, RQR, status_out, st);
    if (rc) return rc;
    if (ms_out) HIP_TRY(hipEventRecord(ev[2], st));
    const int32_t* okey = nullptr;
    // dispatch key of the Kalman launch: the cycle-reduction iteration counts when there are any (free, and the better
    // predictor on the bench workload), else a persistence key computed from T itself (gensys, backward-direct)
    if (opt().kalman_order == 1 && is_cr) {
      okey = it_w;
    } else if (opt().kalman_order != 0 && batch >= 512 && n <= 64) {
      // gensys on the window path has written the key from its own spectrum (gensys_post_kernel)
      if (!gensys_key && (rc = launch_persistence_key(Tw, status_out, batch, n, key_w, st))) return rc;
      okey = key_w;
    }
    if ((rc = launch_kalman(Tw, RQR, P0, 0, o, batch, n, n_state_hint, z_selector_hint, logp_out, status_out, st, okey,
                            fold_rqr ? Rw : nullptr, q, k, have_colmask ? cm_w : nullptr)))
      return rc;
    if (gov.used) {
      // join the verdict; R of the draws the ordered QZ solved (explicit selection, marked draws only, by the verdict's status);
      // their status words; their filter (every launch a second pass)
      if ((rc = gov.side->join(st))) return rc;
      if ((rc = assemble_selection(A, B, C, D, Tw, batch, n, k, Rw, nullptr, gov.status, st, gov.marks))) return rc;
      if ((rc = dsge_host::launch_gensys_overlap_merge(batch, gov.marks, gov.status, status_out, logp_out, st))) return rc;
      if ((rc = launch_kalman(Tw, RQR, P0, 0, o, batch, n, n_state_hint, z_selector_hint, logp_out, status_out, st, nullptr,
                              fold_rqr ? Rw : nullptr, q, k, nullptr, 1)))
        return rc;
    }
    if (park_failures) {
      if ((rc = launch_status_park(status_out, (int32_t*)cm_w, batch, 1, st))) return rc;
    }
    if (ms_out) {
      HIP_TRY(hipEventRecord(ev[3], st));
      HIP_TRY(hipEventSynchronize(ev[3]));
      for (int i = 0; i < 3; ++i) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
        acc_ms[i] += ms;
      }
    }
  }
  if (ms_out)
    for (int i = 0; i < 3; ++i) ms_out[i] = acc_ms[i] / (float)n_rep;
  return DSGE_SUCCESS;
}

extern "C" {

int dsge_solve_kalman_logp_batched(const double* A, const double* B, const double* C, const double* D, const double* Q,
                                   int q_mode, const double* Z, int z_batched, const double* d, int d_batched,
                                   const double* Hdiag, int h_batched, const double* y, int batch, int n, int k, int p,
                                   int T_len, int solver, double tol, int max_iter, double jitter, double missing_fill,
                                   int n_state_hint, int z_selector_hint, int n_lead_hint, double* logp_out,
                                   int32_t* status_out, double* T_out, double* R_out, double* resid_out,
                                   int32_t* n_iter_out, void* stream) {
  // Large batches run as chunks alternating over two library-owned streams (fork / join by events on the caller's
  // stream): a draw whose covariance recursion converges late -- or never, within the sample -- keeps ONE wavefront of the
  // Kalman launch busy for up to 200 full steps (1.5 ms) while the rest of the GPU has long finished; with two chunk
  // pipelines in flight that tail overlaps the cycle-reduction launch of the next chunk instead of being idle time.
  const ObsModel obs{Z, z_batched, d, d_batched, Hdiag, h_batched, y, p, T_len, jitter, missing_fill};
  const ShockCov q{Q, q_mode};
  int rc = check_pipeline(batch, n, k, obs, q, solver, A && B && C && D && logp_out && status_out);
  if (rc) return rc;
  if (opt().pipeline_chunks < 2 || batch < 1024 || batch / opt().pipeline_chunks < 256)
    return pipeline_unchunked(A, B, C, D, q, obs, batch, n, k, solver, tol, max_iter, n_state_hint, z_selector_hint, n_lead_hint,
                              logp_out, status_out, T_out, R_out, resid_out, n_iter_out, (hipStream_t)stream, 1, nullptr);
  if ((rc = ensure_device())) return rc;
  hipStream_t caller = (hipStream_t)stream;
  const int n_chunks = opt().pipeline_chunks;
  const int n_str = n_chunks < MAX_CHUNK_STREAMS ? n_chunks : MAX_CHUNK_STREAMS;
  const int per = ((batch + n_chunks - 1) / n_chunks + 63) & ~63;
  size_t slice;  // bytes of one chunk's layout (a multiple of 256)
  {
    ScratchLayout one;
    PipelineScratch unused;
    pipeline_declare(one, unused, per, n, k, z_batched, T_out, R_out, n_iter_out);
    slice = one.bytes();
  }
  void* base = nullptr;
  if ((rc = g_scratch_pool.reserve(slice * n_chunks, caller, &base))) return rc;
  ForkGuard open[MAX_CHUNK_STREAMS];  // (whatever ends the chunk loop early: the caller's stream waits for every chunk stream)
  for (int i = 0; i < n_str; ++i) {
    open[i].side = &t_chunk[i];
    open[i].into = caller;
    if ((rc = t_chunk[i].fork(caller))) return rc;
  }
  for (int c = 0; c * per < batch; ++c) {
    const int c0 = c * per;
    const int nb = (batch - c0 < per) ? batch - c0 : per;
    const size_t o2 = (size_t)c0 * n * n, ok = (size_t)c0 * n * k;
    rc = pipeline_unchunked(A + o2, B + o2, C + o2, D + ok, q.at(c0, k), obs.at(c0, n), nb, n, k, solver, tol, max_iter, n_state_hint,
                            z_selector_hint, n_lead_hint, logp_out + c0, status_out + c0, T_out ? T_out + o2 : nullptr,
                            R_out ? R_out + ok : nullptr, resid_out ? resid_out + c0 : nullptr, n_iter_out ? n_iter_out + c0 : nullptr,
                            t_chunk[c % n_str].stream(), 1, nullptr, (char*)base + slice * c);
    if (rc) return rc;
  }
  for (int i = 0; i < n_str; ++i)
    if ((rc = t_chunk[i].join(caller))) return rc;
  return DSGE_SUCCESS;
}

int dsge_second_order_logp_batched(const double* A, const double* B, const double* C, const double* D,
                                   const int32_t* hess_idx, int nnz, const double* hess_val, const double* q, int q_batched,
                                   const double* Z, const double* d, const double* Hdiag, const double* y, int batch, int n,
                                   int k, int p, int T_len, int solver, double tol, int max_iter, double jitter,
                                   double missing_fill, const int32_t* state_idx, int n_state, const int32_t* lead_idx,
                                   int n_lead, const int32_t* ret_idx, int n_ret, double* logp_out, int32_t* status_out,
                                   double* T_out, double* R_out, double* gyy_out, double* gyu_out, double* guu_out,
                                   double* gss_out, float* stage_ms, void* stream) {
  const ObsModel obs{Z, 0, d, 0, Hdiag, 0, y, p, T_len, jitter, missing_fill};
  const ShockCov qc{q, q_batched ? DSGE_Q_DIAG_BATCHED : DSGE_Q_DIAG_SHARED};
  int rc = check_second_order(batch, n, k, obs, qc, solver, nnz, state_idx, n_state, lead_idx, n_lead, ret_idx, n_ret,
                              A && B && C && D && (nnz == 0 || (hess_idx && hess_val)) && logp_out && status_out);
  if (rc) return rc;
  if ((rc = ensure_device())) return rc;
  if (batch == 0) return DSGE_SUCCESS;
  hipStream_t st = (hipStream_t)stream;
  const size_t nn = (size_t)batch * n * n, nk = (size_t)batch * n * k;
  double *Tw = T_out, *Rw = R_out;
  int32_t *eu_w = nullptr, *it_w = nullptr;
  ScratchLayout lay;
  if (!Tw) lay.add(&Tw, nn);
  if (!Rw) lay.add(&Rw, nk);
  lay.add(&eu_w, (size_t)batch * 3);
  lay.add(&it_w, (size_t)batch);
  if ((rc = lay.reserve(g_scratch_pool, st))) return rc;
  EventGuard e0, e1;  // (destroyed on every return path)
  if (stage_ms) {
    HIP_TRY(e0.create());
    HIP_TRY(e1.create());
    HIP_TRY(hipEventRecord(e0, st));
  }
  if (solver == DSGE_SOLVER_CYCLE_REDUCTION) {
    int deflated = 0;
    if ((rc = launch_cr_deflated(A, B, C, D, batch, n, k, max_iter, tol, Tw, Rw, status_out, it_w, st, &deflated))) return rc;
    if (!deflated && (rc = launch_cr(A, B, C, batch, n, max_iter, tol, Tw, status_out, it_w, st, 0, D, k, Rw))) return rc;
  } else {
    if ((rc = launch_gensys(A, B, C, batch, n, tol, n_lead, Tw, eu_w, status_out, st))) return rc;
    if ((rc = assemble_selection(A, B, C, D, Tw, batch, n, k, Rw, nullptr, status_out, st))) return rc;
  }
  if (stage_ms) HIP_TRY(hipEventRecord(e1, st));
  rc = launch_second_order(B, C, Tw, Rw, hess_idx, nnz, hess_val, q, q_batched, Z, d, Hdiag, y, batch, n, k, p, T_len, jitter,
                           missing_fill, state_idx, n_state, lead_idx, n_lead, ret_idx, n_ret, logp_out, status_out, gyy_out,
                           gyu_out, guu_out, gss_out, g_kalman_steady_at, nullptr, st, stage_ms ? stage_ms + 1 : nullptr,
                           solver == DSGE_SOLVER_CYCLE_REDUCTION ? it_w : nullptr);
  if (rc) return rc;
  if (stage_ms) {
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipEventElapsedTime(&stage_ms[0], e0, e1));
  }
  return DSGE_SUCCESS;
}

int dsge_solve_kalman_logp_augmented_batched(const double* A, const double* B, const double* C, const double* D,
                                             const double* Q, int q_mode, const double* Z, int z_batched,
                                             const double* d, int d_batched, const double* Hdiag, int h_batched,
                                             const double* y, int batch, int n, int k, int p, int T_len, int solver,
                                             double tol, int max_iter, double jitter, double missing_fill, int m,
                                             const int32_t* inv_var_order, int n_links, const int32_t* link_rows,
                                             const int32_t* link_cols, int n_state_hint, int z_selector_hint,
                                             int n_lead_hint, double* logp_out, int32_t* status_out, double* T_aug_out,
                                             double* R_aug_out, double* resid_out, void* stream) {
  const bool is_cr = solver == DSGE_SOLVER_CYCLE_REDUCTION || solver == DSGE_SOLVER_SCAN_CYCLE_REDUCTION;
  const ObsModel obs{Z, z_batched, d, d_batched, Hdiag, h_batched, y, p, T_len, jitter, missing_fill};
  const ShockCov q{Q, q_mode};
  int rc = check_augmented(batch, n, k, obs, q, solver, m, n_links,
                           A && B && C && D && logp_out && status_out && (n_links == 0 || (link_rows && link_cols)));
  if (rc) return rc;
  if ((rc = ensure_device())) return rc;
  if (batch == 0) return DSGE_SUCCESS;
  hipStream_t st = (hipStream_t)stream;
  const size_t nn = (size_t)batch * n * n, nk = (size_t)batch * n * k, mm = (size_t)batch * m * m, mk = (size_t)batch * m * k;
  double *Tw = nullptr, *Rw = nullptr, *Ta = T_aug_out, *Ra = R_aug_out, *RQR = nullptr, *P0 = nullptr;
  int32_t* eu_w = nullptr;
  ScratchLayout lay;
  lay.add(&Tw, nn);
  lay.add(&Rw, nk);
  if (!Ta) lay.add(&Ta, mm);
  if (!Ra) lay.add(&Ra, mk);
  lay.add(&RQR, mm);
  lay.add(&P0, mm);
  lay.add(&eu_w, (size_t)batch * 3);
  if ((rc = lay.reserve(g_scratch_pool, st))) return rc;
  if (is_cr) {
    rc = launch_cr(A, B, C, batch, n, max_iter, tol, Tw, status_out, nullptr, st, solver == DSGE_SOLVER_SCAN_CYCLE_REDUCTION);
  } else if (solver == DSGE_SOLVER_GENSYS) {
    rc = launch_gensys(A, B, C, batch, n, tol, n_lead_hint, Tw, eu_w, status_out, st);
  } else {
    HIP_TRY(hipMemsetAsync(status_out, 0, sizeof(int32_t) * batch, st));
    rc = launch_bdirect(A, B, D, batch, n, k, Tw, Rw, st);
  }
  if (rc) return rc;
  // R and the policy residual in SOLVER order (statespace.py:213), then un-permute + augment
  if ((rc = assemble_selection(A, B, C, D, Tw, batch, n, k, Rw, resid_out, status_out, st))) return rc;
  if ((rc = launch_augment(Tw, Rw, batch, n, k, m, inv_var_order, n_links, link_rows, link_cols, Ta, Ra, st))) return rc;
  if (m > DSGE_MAX_N) {
    // Round 6: 65 .. 96 augmented states (cumulator and observation-lag chains on a 40-variable model, statespace.py:598-723).
    // The filter does not grow with m: the model restricted to F = {non-zero columns of T_aug} u {observed variables} is exact
    // (x_t[F] depends on x_{t-1}[F] only, y_t on x_t[F] only -- the argument of the 65 .. 96-variable route, csrc/dsge_big.hpp),
    // and the existing kernels take |F| <= 64.  F is measured on the device (one 32-byte read-back: the call synchronises its
    // stream once); a model beyond 64 filtered variables is DSGE_ERR_TOO_LARGE -- with T_aug, R_aug, the status words and the
    // residual of this call already written (they do not depend on the filter).
    unsigned char idx[64];
    int u = 0, ns = 0;
    if ((rc = big_filtered_variables(Ta, Z, z_batched, batch, m, p, st, idx, &u, &ns))) return rc;
    if (u > 64)
      return fail(DSGE_ERR_TOO_LARGE, "augmented solve + Kalman with m > 64: " + std::to_string(u) +
                                          " state (incl. chain) and observed variables, the filter kernels take at most 64");
    if (u < 1) return fail(DSGE_ERR_INVALID, "augmented solve + Kalman with m > 64: no state and no observed variable");
    const size_t uu = (size_t)batch * 64 * 64;
    double *T_r = nullptr, *RQR_r = nullptr, *P0_r = nullptr, *R_r = nullptr, *Z_r = nullptr;
    ScratchLayout gathered;
    gathered.add(&T_r, uu);
    gathered.add(&RQR_r, uu);
    gathered.add(&P0_r, uu);
    gathered.add(&R_r, (size_t)batch * 64 * k);
    gathered.add(&Z_r, z_batched ? (size_t)batch * p * 64 : (size_t)p * 64);
    if ((rc = gathered.reserve(g_aug_big_pool, st))) return rc;
    if ((rc = launch_big_compress(Ta, Ra, Z, z_batched, batch, m, k, p, idx, u, T_r, R_r, Z_r, st))) return rc;
    if ((rc = assemble_rqr(R_r, q, batch, u, k, RQR_r, status_out, st))) return rc;
    const int ns_hint = (ns > 0 && ns < u) ? ns : 0;
    ObsModel o_r = obs;  // the observation model on the gathered variables
    o_r.Z = Z_r;
    return launch_kalman(T_r, RQR_r, P0_r, 0, o_r, batch, u, ns_hint, z_selector_hint, logp_out, status_out, st);
  }
  if ((rc = assemble_rqr(Ra, q, batch, m, k, RQR, status_out, st))) return rc;
  return launch_kalman(Ta, RQR, P0, 0, obs, batch, m, n_state_hint, z_selector_hint, logp_out, status_out, st);
}

// dense_z = 0: the selector path.  dense_z = 1: any design matrix, by carrying the observed combinations as p extra variables
// (dsge_augment.hpp: dense_z_augment_kernel): the reverse sweep runs on the augmented model of n + p variables, the assembly
// reverse and the policy adjoints on the original n; n_filter_hint then counts the STATE variables (non-zero columns of A).
static int grad_pipeline(const double* A, const double* B, const double* C, const double* D, const ShockCov& q, const ObsModel& o,
                         int batch, int n, int k, int solver, double tol, int max_iter, int n_filter_hint, int n_lead_hint,
                         double* logp_out, int32_t* status_out, double* A_bar, double* B_bar, double* C_bar, double* D_bar,
                         double* q_bar, double* d_bar, double* h_bar, int dense_z, double* Z_bar, void* stream) {
  const int p = o.p, T_len = o.T_len;
  int rc = check_grad(batch, n, k, o, q, solver, dense_z != 0,
                      A && B && C && D && logp_out && status_out && A_bar && B_bar && C_bar && D_bar && q_bar);
  if (rc) return rc;
  if ((rc = ensure_device())) return rc;
  if (batch == 0) return DSGE_SUCCESS;
  hipStream_t st = (hipStream_t)stream;
  const int m = dense_z ? n + p : n;                                   // size of the model the reverse sweep runs on
  const int u_hint = dense_z ? (n_filter_hint > 0 ? n_filter_hint + p : 0) : n_filter_hint;
  const bool qfull = !q.diag();                            // DSGE_Q_FULL_*: Q and q_bar are k x k
  const size_t qstride = qfull ? (size_t)k * k : (size_t)k;
  // the reverse sweep re-reads the stored (a_t, P_t): chunk the batch so that the store stays <= 16 GiB of the 288 GB
  const size_t per_draw = kalman_grad_store_doubles_per_draw(u_hint, m, T_len) * sizeof(double);
  size_t chunk = per_draw ? ((size_t)16 << 30) / per_draw : (size_t)batch;
  if (chunk < 1) chunk = 1;
  if (chunk > (size_t)batch) chunk = (size_t)batch;
  const size_t nn = chunk * n * n, nk = chunk * n * k;
  const size_t mm = chunk * (size_t)m * m, mk = chunk * (size_t)m * k;
  double *Tw = nullptr, *Rw = nullptr, *RQR = nullptr, *Tbar = nullptr, *Gbar = nullptr, *store = nullptr;
  int32_t *eu_w = nullptr, *it_w = nullptr, *ord_w = nullptr;
  double *Ta = nullptr, *Ra = nullptr, *RQRa = nullptr, *Tbar_a = nullptr, *Gbar_a = nullptr, *Zaug = nullptr;
  ScratchLayout lay;
  lay.add(&Tw, nn);
  lay.add(&Rw, nk);
  lay.add(&RQR, nn);
  lay.add(&Tbar, nn);
  lay.add(&Gbar, nn);
  lay.add(&eu_w, chunk * 3);
  lay.add(&it_w, chunk);  // cycle-reduction iterations = dispatch key of the reverse-sweep launch
  lay.add(&ord_w, chunk);
  lay.add(&store, chunk * per_draw / sizeof(double) + 1);
  if (dense_z) {
    lay.add(&Ta, mm);
    lay.add(&Ra, mk);
    lay.add(&RQRa, mm);
    lay.add(&Tbar_a, mm);
    lay.add(&Gbar_a, mm);
    lay.add(&Zaug, (size_t)p * m);
  }
  if ((rc = lay.reserve(g_scratch_pool, st))) return rc;
  for (size_t c0 = 0; c0 < (size_t)batch; c0 += chunk) {
    const int nb = (int)(((size_t)batch - c0 < chunk) ? (size_t)batch - c0 : chunk);
    const double *Ac = A + c0 * n * n, *Bc = B + c0 * n * n, *Cc = C + c0 * n * n, *Dc = D + c0 * n * k;
    const ShockCov qc = q.at(c0, k);
    const ObsModel oc = o.at(c0, n);
    int32_t* stc = status_out + c0;
    if (solver == DSGE_SOLVER_GENSYS)
      rc = launch_gensys(Ac, Bc, Cc, nb, n, tol, n_lead_hint, Tw, eu_w, stc, st);
    bool have_R = false;  // R from the solver's final elimination (as in the forward-only call): only sym(RQR') is left
    if (solver != DSGE_SOLVER_GENSYS) {
      int deflated = 0;  // static variables deflated first, as in the forward-only call
      if (solver == DSGE_SOLVER_CYCLE_REDUCTION &&
          (rc = launch_cr_deflated(Ac, Bc, Cc, Dc, nb, n, k, max_iter, tol, Tw, Rw, stc, it_w, st, &deflated)))
        return rc;
      have_R = deflated != 0;
      if (!deflated) {
        const bool fr = solver == DSGE_SOLVER_CYCLE_REDUCTION && opt().cr_fused_selection;
        rc = launch_cr(Ac, Bc, Cc, nb, n, max_iter, tol, Tw, stc, it_w, st, solver == DSGE_SOLVER_SCAN_CYCLE_REDUCTION,
                       fr ? Dc : nullptr, k, fr ? Rw : nullptr);
        have_R = fr;
      }
    }
    if (rc) return rc;
    if (have_R && k <= 16 && n <= 64 && !qfull) {
      if (!dense_z && (rc = launch_rqr(Rw, qc.Q, qc.mode, nb, n, k, stc, RQR, st))) return rc;
    } else if ((rc = assemble_selection_rqr(Ac, Bc, Cc, Dc, Tw, qc, nb, n, k, Rw, nullptr, RQR, stc, st)))
      return rc;
    if (dense_z) {  // the augmented model and its sym(R Q R')
      if ((rc = launch_dense_z_augment(Tw, Rw, oc.Z, oc.z_batched, nb, n, k, p, Ta, Ra, Zaug, st))) return rc;
      if ((rc = assemble_rqr(Ra, qc, nb, m, k, RQRa, stc, st))) return rc;
    }
    int32_t* gkey = (solver == DSGE_SOLVER_GENSYS) ? nullptr : it_w;  // (the gradient's forward sweep overwrites it with its step counts)
    if (opt().kalman_order == 0) {
      gkey = nullptr;
    } else if ((opt().kalman_order == 2 || solver == DSGE_SOLVER_GENSYS) && nb >= 512) {
      if ((rc = launch_persistence_key(Tw, stc, nb, n, it_w, st))) return rc;  // (the iteration counts are not needed again)
      gkey = it_w;
    }
    double *dbc = d_bar ? d_bar + c0 * p : nullptr, *hbc = h_bar ? h_bar + c0 * p : nullptr;
    if (dense_z) {
      ObsModel oa = oc;  // the observed combinations are variables of the augmented model: one shared selector
      oa.Z = Zaug;
      oa.z_batched = 0;
      if ((rc = launch_kalman_grad(Ta, RQRa, oa, nb, m, u_hint, store, logp_out + c0, stc, Tbar_a, Gbar_a, dbc, hbc, st, gkey,
                                   ord_w)))
        return rc;
      if ((rc = launch_dense_z_deaugment(Tbar_a, Gbar_a, Tw, RQRa, oc.Z, oc.z_batched, stc, nb, n, p, Tbar, Gbar,
                                         Z_bar ? Z_bar + c0 * p * n : nullptr, st)))
        return rc;
    } else if ((rc = launch_kalman_grad(Tw, RQR, oc, nb, n, u_hint, store, logp_out + c0, stc, Tbar, Gbar, dbc, hbc, st, gkey,
                                        ord_w)))
      return rc;
    // Round 6: diagonal Q, k <= 16, up to 40 variables: one launch for the reverse of the assembly AND the policy adjoints (they
    // share the elimination of B + C T; adjoint_kernel<BS, false, true>), the two-kernel path behind it for what it flags
    if (!qfull && k <= 16 && n <= 40 && opt().grad_fused_adjoint) {
      if ((rc = launch_adjoint_fused(Bc, Cc, Tw, Rw, qc.Q, qc.mode, Gbar, Tbar, nb, n, k, A_bar + c0 * n * n, B_bar + c0 * n * n,
                                     C_bar + c0 * n * n, D_bar + c0 * n * k, q_bar + c0 * qstride, stc, st)))
        return rc;
      continue;
    }
    if ((rc = launch_grad_assemble(Bc, Cc, Tw, Rw, qc.Q, qc.mode, Gbar, nb, n, k, stc, Tbar, B_bar + c0 * n * n,
                                   C_bar + c0 * n * n, D_bar + c0 * n * k, q_bar + c0 * qstride, st)))
      return rc;
    if ((rc = launch_adjoint(Bc, Cc, Tw, Tbar, nb, n, A_bar + c0 * n * n, B_bar + c0 * n * n, C_bar + c0 * n * n, stc, st,
                             1)))
      return rc;
  }
  return DSGE_SUCCESS;
}

int dsge_solve_kalman_logp_grad_batched(const double* A, const double* B, const double* C, const double* D, const double* q,
                                        int q_batched, const double* Z, int z_batched, const double* d, int d_batched,
                                        const double* Hdiag, int h_batched, const double* y, int batch, int n, int k,
                                        int p, int T_len, int solver, double tol, int max_iter, double jitter,
                                        double missing_fill, int n_filter_hint, int n_lead_hint, double* logp_out,
                                        int32_t* status_out, double* A_bar, double* B_bar, double* C_bar, double* D_bar,
                                        double* q_bar, double* d_bar, double* h_bar, void* stream) {
  return grad_pipeline(A, B, C, D, ShockCov{q, q_batched},
                       ObsModel{Z, z_batched, d, d_batched, Hdiag, h_batched, y, p, T_len, jitter, missing_fill}, batch, n, k, solver, tol,
                       max_iter, n_filter_hint, n_lead_hint, logp_out, status_out, A_bar, B_bar, C_bar, D_bar, q_bar, d_bar, h_bar, 0, nullptr,
                       stream);
}

int dsge_solve_kalman_logp_grad_dense_z_batched(const double* A, const double* B, const double* C, const double* D,
                                                const double* q, int q_batched, const double* Z, int z_batched, const double* d,
                                                int d_batched, const double* Hdiag, int h_batched, const double* y, int batch,
                                                int n, int k, int p, int T_len, int solver, double tol, int max_iter,
                                                double jitter, double missing_fill, int n_state_hint, int n_lead_hint,
                                                double* logp_out, int32_t* status_out, double* A_bar, double* B_bar,
                                                double* C_bar, double* D_bar, double* q_bar, double* d_bar, double* h_bar,
                                                double* Z_bar, void* stream) {
  return grad_pipeline(A, B, C, D, ShockCov{q, q_batched},
                       ObsModel{Z, z_batched, d, d_batched, Hdiag, h_batched, y, p, T_len, jitter, missing_fill}, batch, n, k, solver, tol,
                       max_iter, n_state_hint, n_lead_hint, logp_out, status_out, A_bar, B_bar, C_bar, D_bar, q_bar, d_bar, h_bar, 1, Z_bar,
                       stream);
}

int dsge_profile_pipeline(const double* A, const double* B, const double* C, const double* D, const double* Q,
                          int q_mode, const double* Z, int z_batched, const double* d, int d_batched,
                          const double* Hdiag, int h_batched, const double* y, int batch, int n, int k, int p,
                          int T_len, int solver, double tol, int max_iter, double jitter, double missing_fill,
                          int n_state_hint, int z_selector_hint, int n_lead_hint, double* logp_out,
                          int32_t* status_out, int reps, float* ms_out, void* stream) {
  if (!ms_out || reps < 1) return fail(DSGE_ERR_INVALID, "ms_out null or reps < 1");
  const ObsModel obs{Z, z_batched, d, d_batched, Hdiag, h_batched, y, p, T_len, jitter, missing_fill};
  const ShockCov q{Q, q_mode};
  int rc = check_pipeline(batch, n, k, obs, q, solver, A && B && C && D && logp_out && status_out);
  if (rc) return rc;
  return pipeline_unchunked(A, B, C, D, q, obs, batch, n, k, solver, tol, max_iter, n_state_hint, z_selector_hint, n_lead_hint,
                            logp_out,
                            status_out, nullptr, nullptr, nullptr, nullptr, (hipStream_t)stream, reps, ms_out);
}

// Debug hook: when enabled, kalman_sel_kernel accumulates the shader cycles draw 0 spends in each
// of its five per-step phases, [5] = cycles in steady-state steps, [6] = number of steady-state steps,
// [7] = total; dsge_debug_kalman_phases(0/1 enable, out[8]) reads them back.
int dsge_debug_kalman_phases(int enable, long long* cycles_out) { return debug_counters(&g_kalman_dbg, 16, enable, cycles_out); }

// Debug hook: cr_big_kernel (n > 64) accumulates the shader cycles workgroup 0 spends on its first draw: [0] register-block loads,
// [1] eliminations, [2] row scatters, [3] the four products and norms, [4] iterations, [5] total (with the final solve);
// [8..12] inside the eliminations (thread 0): candidates + column, first barrier, pivot row, second barrier, update.  16 values.
int dsge_debug_big_phases(int enable, long long* cycles_out) { return debug_counters(&g_big_dbg, 16, enable, cycles_out); }

// Debug hook (not part of the drop-in surface): shader-clock stamps of draw 0 at the phase
// boundaries of gensys_kernel: [start, after Hessenberg-triangular, after QZ, after reordering,
// after SVDs / eu codes, end].  Device pointers; cycles_out is a HOST array of 6 int64.
int dsge_debug_gensys_phases(const double* A, const double* B, const double* C, int batch, int n, double tol,
                             int n_lead_hint, double* T_out, int32_t* eu_out, int32_t* status, long long* cycles_out) {
  int rc = check_common(batch, n, DSGE_MAX_N_GENSYS - 1);
  if (rc) return rc;
  if ((rc = ensure_device())) return rc;
  hipStream_t tw_st = nullptr, tw_st1 = nullptr;
  if ((rc = twin_streams(&tw_st, &tw_st1))) return rc;
  (void)tw_st1;
  long long* d = nullptr;
  HIP_TRY(hipMalloc((void**)&d, 6 * sizeof(long long)));
  HIP_TRY(hipMemset(d, 0, 6 * sizeof(long long)));
  rc = launch_gensys(A, B, C, batch, n, tol, n_lead_hint, T_out, eu_out, status, nullptr, d);
  if (!rc) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(cycles_out, d, 6 * sizeof(long long), hipMemcpyDeviceToHost));
  }
  (void)hipFree(d);
  return rc;
}

// Debug hook: enable = 1 allocates the stamp buffer of the window kernels (draw 0 of each launch: reduce [0..4], QZ [8..11],
// eu [16..19], post [20..26]); cycles_out (host int64[32], may be NULL) reads it back; enable = 0 frees it.
int dsge_debug_gensys_stage_ms(int enable, float* ms_out) {
  static float stage[8];
  if (ms_out)
    for (int i = 0; i < 8; ++i) ms_out[i] = stage[i];
  if (enable) {
    for (float& x : stage) x = 0.f;
    g_gensys_stage_ms = stage;
  } else {
    g_gensys_stage_ms = nullptr;
  }
  return DSGE_SUCCESS;
}

int dsge_debug_gensys_window_phases(int enable, long long* cycles_out) {
  return debug_counters(&g_gensys_win_dbg, 32, enable, cycles_out);
}

// ---- per-call options (include/dsge_hip.h: dsge_options) --------------------------------------------------------------
int dsge_options_init(dsge_options* o) {
  if (!o) return fail(DSGE_ERR_INVALID, "null pointer");
  *o = g_defaults;  // (the dsge_options part: struct_size set, reserved_ zero -- struct Options, dsge_host.hpp)
  return DSGE_SUCCESS;
}

namespace {
thread_local std::vector<OptionsGuard*> t_scope;  // dsge_options_push / dsge_options_pop of this thread
}

int dsge_options_push(const dsge_options* o) {
  if (!o) return fail(DSGE_ERR_INVALID, "null pointer");
  int rc = check_options(o);
  if (rc) return rc;
  t_scope.push_back(new OptionsGuard(o));
  return DSGE_SUCCESS;
}

int dsge_options_pop(void) {
  if (t_scope.empty()) return fail(DSGE_ERR_INVALID, "dsge_options_pop without a matching push on this thread");
  delete t_scope.back();
  t_scope.pop_back();
  return DSGE_SUCCESS;
}

int dsge_solve_kalman_logp_batched_opt(const dsge_options* opt, const double* A, const double* B, const double* C,
                                       const double* D, const double* Q, int q_mode, const double* Z, int z_batched,
                                       const double* d, int d_batched, const double* Hdiag, int h_batched, const double* y,
                                       int batch, int n, int k, int p, int T_len, int solver, double tol, int max_iter,
                                       double jitter, double missing_fill, int n_state_hint, int z_selector_hint,
                                       int n_lead_hint, double* logp_out, int32_t* status_out, double* T_out, double* R_out,
                                       double* resid_out, int32_t* n_iter_out, void* stream) {
  int rc = check_options(opt);
  if (rc) return rc;
  OptionsGuard guard(opt);
  return dsge_solve_kalman_logp_batched(A, B, C, D, Q, q_mode, Z, z_batched, d, d_batched, Hdiag, h_batched, y, batch, n, k, p,
                                        T_len, solver, tol, max_iter, jitter, missing_fill, n_state_hint, z_selector_hint,
                                        n_lead_hint, logp_out, status_out, T_out, R_out, resid_out, n_iter_out, stream);
}

int dsge_solve_kalman_logp_batched_host_opt(const dsge_options* opt, const double* A, const double* B, const double* C,
                                            const double* D, const double* Q, int q_mode, const double* Z, int z_batched,
                                            const double* d, int d_batched, const double* Hdiag, int h_batched,
                                            const double* y, int batch, int n, int k, int p, int T_len, int solver, double tol,
                                            int max_iter, double jitter, double missing_fill, int n_state_hint,
                                            int z_selector_hint, int n_lead_hint, double* logp_out, int32_t* status_out,
                                            double* T_out, double* R_out, double* resid_out, int32_t* n_iter_out) {
  int rc = check_options(opt);
  if (rc) return rc;
  OptionsGuard guard(opt);
  return dsge_solve_kalman_logp_batched_host(A, B, C, D, Q, q_mode, Z, z_batched, d, d_batched, Hdiag, h_batched, y, batch, n,
                                             k, p, T_len, solver, tol, max_iter, jitter, missing_fill, n_state_hint,
                                             z_selector_hint, n_lead_hint, logp_out, status_out, T_out, R_out, resid_out,
                                             n_iter_out);
}

int dsge_solve_kalman_logp_grad_batched_opt(const dsge_options* opt, const double* A, const double* B, const double* C,
                                            const double* D, const double* q, int q_batched, const double* Z, int z_batched,
                                            const double* d, int d_batched, const double* Hdiag, int h_batched,
                                            const double* y, int batch, int n, int k, int p, int T_len, int solver, double tol,
                                            int max_iter, double jitter, double missing_fill, int n_filter_hint,
                                            int n_lead_hint, double* logp_out, int32_t* status_out, double* A_bar,
                                            double* B_bar, double* C_bar, double* D_bar, double* q_bar, double* d_bar,
                                            double* h_bar, void* stream) {
  int rc = check_options(opt);
  if (rc) return rc;
  OptionsGuard guard(opt);
  return dsge_solve_kalman_logp_grad_batched(A, B, C, D, q, q_batched, Z, z_batched, d, d_batched, Hdiag, h_batched, y, batch, n,
                                             k, p, T_len, solver, tol, max_iter, jitter, missing_fill, n_filter_hint,
                                             n_lead_hint, logp_out, status_out, A_bar, B_bar, C_bar, D_bar, q_bar, d_bar, h_bar,
                                             stream);
}

int dsge_solve_kalman_logp_grad_batched_host_opt(const dsge_options* opt, const double* A, const double* B, const double* C,
                                                 const double* D, const double* q, int q_batched, const double* Z,
                                                 int z_batched, const double* d, int d_batched, const double* Hdiag,
                                                 int h_batched, const double* y, int batch, int n, int k, int p, int T_len,
                                                 int solver, double tol, int max_iter, double jitter, double missing_fill,
                                                 int n_filter_hint, int n_lead_hint, double* logp_out, int32_t* status_out,
                                                 double* A_bar, double* B_bar, double* C_bar, double* D_bar, double* q_bar,
                                                 double* d_bar, double* h_bar) {
  int rc = check_options(opt);
  if (rc) return rc;
  OptionsGuard guard(opt);
  return dsge_solve_kalman_logp_grad_batched_host(A, B, C, D, q, q_batched, Z, z_batched, d, d_batched, Hdiag, h_batched, y,
                                                  batch, n, k, p, T_len, solver, tol, max_iter, jitter, missing_fill,
                                                  n_filter_hint, n_lead_hint, logp_out, status_out, A_bar, B_bar, C_bar, D_bar,
                                                  q_bar, d_bar, h_bar);
}

}  // extern "C"
