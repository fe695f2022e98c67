// Host-side plumbing shared by the translation units of libdsge_hip.so: error reporting, the tile-size
// dispatch and the prototypes of the kernel launchers.  Each launch_*.hip file instantiates only its
// own kernels, so the library builds as independent (parallel) hipcc jobs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>
#include <string>
#include <vector>

#include "../../include/dsge_hip.h"
#include "dsge_filter_conv.hpp"

namespace dsge_host {

int fail(int code, const std::string& msg);  // records the message for dsge_last_error(), returns code

#define HIP_TRY(expr)                                                                              \
  do {                                                                                             \
    hipError_t _e = (expr);                                                                        \
    if (_e != hipSuccess) {                                                                        \
      (void)hipGetLastError(); /* clear the sticky error so later calls are not poisoned */        \
      return dsge_host::fail(DSGE_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));     \
    }                                                                                              \
  } while (0)

constexpr size_t LDS_LIMIT = 160 * 1024;

// Library-owned device scratch: ONE arena per (device, stream) and pool -- the library is re-entrant per stream:
// two calls enqueued on two streams never share intermediates.  Slots are created on demand (a host thread's library streams
// release theirs when the thread exits: ThreadStream, stream_arenas_release); beyond MAX_SLOTS live (device, stream) pairs the least
// recently used slot is recycled after a device-wide synchronisation, and it changes owner -- the former stream gets a
// fresh slot on its next call, so no two streams ever hold the same memory.
class StreamArenaPool {
 public:
  StreamArenaPool();
  int reserve(size_t bytes, hipStream_t st, void** out);  // the arena of (current device, st), grown to >= bytes
  void release(hipStream_t st);                            // the stream is going away: its slots become free
 private:
  struct Slot {
    void* ptr = nullptr;
    size_t cap = 0;
    int dev = -1;
    hipStream_t stream = nullptr;
    bool used = false;
    unsigned long long stamp = 0;
  };
  static constexpr size_t MAX_SLOTS = 64;
  std::vector<Slot> slots_;
  std::mutex mu_;
  unsigned long long clock_ = 0;
};
void stream_arenas_release(hipStream_t st);  // every pool of the library (dsge_api.hip)

// The scratch buffers of one entry point, declared ONCE: add() names a typed pointer slot and its element count, reserve() sizes
// the arena from that list (every buffer rounded to 256 bytes, PAD bytes behind the last), takes it from `pool` for the stream --
// or places it into a slice of an arena the caller reserved -- and fills the slots.  What is carved can therefore never exceed
// what was reserved.  An output pointer the caller supplied declares nothing: `double* Tw = T_out; if (!Tw) lay.add(&Tw, nn);`.
// Fixed capacity, no heap: the fused entry only enqueues.
class ScratchLayout {
 public:
  static constexpr size_t PAD = 8192;
  template <typename T>
  void add(T** slot, size_t count) {
    if (n_ < MAX_BUFS) bufs_[n_] = Buf{(void*)slot, count * sizeof(T)};
    ++n_;
  }
  size_t bytes() const;  // of the whole arena
  int reserve(StreamArenaPool& pool, hipStream_t st, void* slice = nullptr);
 private:
  struct Buf {
    void* slot;  // address of the caller's T*
    size_t bytes;
  };
  static size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }
  static constexpr int MAX_BUFS = 16;
  Buf bufs_[MAX_BUFS];
  int n_ = 0;
};

// A library stream of the CALLING THREAD on its current device (non-blocking), with a fork and a join event: created on first
// use, dropped and created again when the thread's device changed or an earlier creation stopped half-way.  When the thread
// exits, the stream is synchronised, its arenas are released (stream_arenas_release) and stream and events are destroyed with
// the owning device made current.  Two host threads never share one, hence never an arena.  `thread_local` instances only.
class ThreadStream {
 public:
  ThreadStream() = default;
  ThreadStream(const ThreadStream&) = delete;
  ThreadStream& operator=(const ThreadStream&) = delete;
  ~ThreadStream() { drop(); }
  int ensure();                      // the stream exists on the current device
  hipStream_t stream() const { return s_; }
  int fork(hipStream_t from);        // ensure(); this stream waits for what is enqueued on `from`
  int join(hipStream_t into);        // `into` waits for what is enqueued on this stream
  // no fork stays open: enqueues the join if one is owed and synchronises this stream if that fails; reports nothing
  void close(hipStream_t into);
 private:
  void drop();
  hipStream_t s_ = nullptr;
  hipEvent_t ev_[2] = {nullptr, nullptr};  // fork, join
  int dev_ = -1;
  bool open_ = false;                // forked, join not enqueued yet
};
// Around a forked section: whichever way the scope is left (the early returns of HIP_TRY included), the caller's stream `into`
// waits for the side stream, so an error code never comes back with work in flight on buffers the caller may free.  On the
// success path the section enqueues side->join(into) itself, where the order of work wants it; the guard then does nothing.
// It never touches the error being returned.
struct ForkGuard {
  ThreadStream* side = nullptr;  // null = nothing was (or will be) forked
  hipStream_t into = nullptr;
  ~ForkGuard() {
    if (side) side->close(into);
  }
};
// The two streams the host twins of the calling thread run on
int twin_streams(hipStream_t* s0, hipStream_t* s1);

// The observation side of a filter problem -- y_t = Z x_t + d + e_t, e_t ~ N(0, diag(Hdiag)), the data panel and how it is read --
// as every entry of the filter family receives it
struct ObsModel {
  const double* Z; int z_batched;      // [p][m] or [batch][p][m]
  const double* d; int d_batched;      // [p] or [batch][p]; may be null
  const double* Hdiag; int h_batched;  // likewise
  const double* y;                     // [T_len][p]
  int p, T_len;
  double jitter, missing_fill;
  // the same description for the draws from c0 on, of a model with m variables: only the per-draw members move
  ObsModel at(size_t c0, int m) const {
    ObsModel o = *this;
    if (z_batched) o.Z += c0 * p * m;
    if (d && d_batched) o.d += c0 * p;
    if (Hdiag && h_batched) o.Hdiag += c0 * p;
    return o;
  }
};
// The shock covariance in one of the layouts DSGE_Q_*: [k], [batch][k], [k][k] or [batch][k][k]
struct ShockCov {
  const double* Q = nullptr; int mode = DSGE_Q_DIAG_SHARED;
  bool diag() const { return mode == DSGE_Q_DIAG_SHARED || mode == DSGE_Q_DIAG_BATCHED; }
  bool batched() const { return mode == DSGE_Q_DIAG_BATCHED || mode == DSGE_Q_FULL_BATCHED; }
  size_t elems(int batch, int k) const { return (size_t)(batched() ? batch : 1) * k * (diag() ? 1 : k); }
  ShockCov at(size_t c0, int k) const { return ShockCov{batched() ? Q + c0 * elems(1, k) : Q, mode}; }
};
// The filter problem across dated breaks (dsge_kalman_seg.hpp), as the likelihood, the smoother and the gradient receive it.  The
// segment axis stands behind the draw axis: T, R, shift and the per-draw members of q and obs are [batch][S] problems, the shared
// members of q and obs [S] ones; a0, P0: [batch].  a0, P0 and shift may be null; seg_start: HOST list of S entries, already checked
struct SegmentedProblem {
  const double *T, *R;
  ShockCov q;
  ObsModel obs;
  const double *a0, *P0, *shift;
  const int32_t* seg_start;
  int n_seg, batch, m, k;
  size_t flat() const { return (size_t)batch * n_seg; }                      // (draw, segment) problems
  size_t q_width() const { return q.diag() ? (size_t)k : (size_t)k * k; }    // doubles of one Q
  // the same description for the nb draws from c0 on: the per-draw members move by c0, the per-(draw, segment) ones by c0 * S
  SegmentedProblem at(size_t c0, int nb) const {
    SegmentedProblem c = *this;
    const size_t fo = c0 * n_seg, mm = (size_t)m * m;
    c.T += fo * mm;
    c.R += fo * m * k;
    c.q = q.at(fo, k);
    c.obs = obs.at(fo, m);
    if (a0) c.a0 += c0 * m;
    if (P0) c.P0 += c0 * mm;
    if (shift) c.shift += fo * m;
    c.batch = nb;
    return c;
  }
};

// An entry that runs its batch in contiguous chunks of draws under the caller's scratch limit (0 = 2 GiB): the draws of a chunk at
// per_draw_bytes of scratch each (at least one, at most the batch), and the draws of the chunk that starts at c0
inline int chunk_for(size_t scratch_limit_bytes, size_t per_draw_bytes, int batch) {
  if (scratch_limit_bytes == 0) scratch_limit_bytes = (size_t)2 << 30;
  const size_t fit = scratch_limit_bytes / per_draw_bytes;
  return fit < 1 ? 1 : (fit > (size_t)batch ? batch : (int)fit);
}
inline int chunk_draws(int batch, int c0, int chunk) { return batch - c0 < chunk ? batch - c0 : chunk; }

int ensure_device();  // lazy check for a gfx950 device: nothing touches HIP before the first call
// The fused solve + filter pipeline of ONE batch on ONE stream: what dsge_solve_kalman_logp_batched runs when it does not
// split the batch (dsge_options.pipeline_chunks), with the stage timing of dsge_profile_pipeline (reps, ms_out) and an
// optional slice of a scratch arena the caller reserved (chunks in flight on several streams).  Arguments as the public entry,
// which has checked them (check_pipeline, below).
int pipeline_unchunked(const double* A, const double* B, const double* C, const double* D, const ShockCov& q, const ObsModel& o,
                       int batch, int n, int k, int solver, double tol, int max_iter, int n_state_hint, int z_selector_hint,
                       int n_lead_hint, double* logp_out, int32_t* status_out, double* T_out, double* R_out, double* resid_out,
                       int32_t* n_iter_out, hipStream_t st, int reps, float* ms_out, void* scratch_slice = nullptr);

// hipEvent_t that destroys itself: stage-timing events must not leak on the early returns of HIP_TRY
struct EventGuard {
  hipEvent_t e = nullptr;
  EventGuard() = default;
  EventGuard(const EventGuard&) = delete;
  EventGuard& operator=(const EventGuard&) = delete;
  ~EventGuard() {
    if (e) (void)hipEventDestroy(e);
  }
  hipError_t create() { return hipEventCreate(&e); }
  operator hipEvent_t() const { return e; }
};

inline int tile_bs(int n) {
  int bs = (n + 7) / 8;
  return bs < 1 ? 1 : bs;
}

// Grid of a second pass that only takes the draws an earlier kernel flagged (normally none): the workgroups loop over the
// draws, so a quarter of the batch-sized grid costs a few microseconds less per empty pass and still fills the chip.
inline int rerun_grid(int batch) { return batch < 1024 ? batch : 1024; }

template <typename K>
int set_lds(K kernel, size_t bytes) {
  HIP_TRY(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  return DSGE_SUCCESS;
}

// One launch with a dynamic LDS image: refused beyond LDS_LIMIT (DSGE_ERR_TOO_LARGE, message `what`), else set_lds, launch, check.
template <typename K, typename A>
int launch_with_lds(K kernel, unsigned grid, int threads, size_t lds_bytes, hipStream_t stream, const A& args, const char* what) {
  if (lds_bytes > LDS_LIMIT) return fail(DSGE_ERR_TOO_LARGE, what);
  if (int rc = set_lds(kernel, lds_bytes)) return rc;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(threads), lds_bytes, stream, args);
  HIP_TRY(hipGetLastError());
  return DSGE_SUCCESS;
}

// grid = batch x units workgroups; beyond 2^31 - 1 the call is refused (DSGE_ERR_TOO_LARGE, `what` is the message)
inline int batch_grid(int batch, int units, const char* what, unsigned* grid) {
  const long long g = (long long)batch * units;
  if (g > 0x7fffffffLL) return fail(DSGE_ERR_TOO_LARGE, what);
  *grid = (unsigned)g;
  return DSGE_SUCCESS;
}

#define DISPATCH_BS(bs, MAXBS, ...)                                                  \
  switch (bs) {                                                                      \
    case 1: { constexpr int BS = 1; __VA_ARGS__; } break;                            \
    case 2: { constexpr int BS = 2; __VA_ARGS__; } break;                            \
    case 3: { constexpr int BS = 3; __VA_ARGS__; } break;                            \
    case 4: { constexpr int BS = 4; __VA_ARGS__; } break;                            \
    case 5: { constexpr int BS = 5; __VA_ARGS__; } break;                            \
    case 6: { constexpr int BS = 6; __VA_ARGS__; } break;                            \
    case 7: if (MAXBS >= 7) { constexpr int BS = (MAXBS >= 7 ? 7 : 6); __VA_ARGS__; } break; \
    case 8: if (MAXBS >= 8) { constexpr int BS = (MAXBS >= 8 ? 8 : 6); __VA_ARGS__; } break; \
    default: break;                                                                  \
  }

// ---- launchers (launch_solvers.hip, launch_assemble.hip, launch_kalman.hip, launch_gensys.hip) ----
int launch_cr(const double* A, const double* B, const double* C, int batch, int n, int max_iter, double tol,
              double* T_out, int32_t* status, int32_t* n_iter, hipStream_t st, int scan_mode = 0,
              const double* D = nullptr, int k = 0, double* R_out = nullptr);  // D, R_out: also R = -A1_hat^-1 D
// launch_big.hip (dsge_big.hpp): models with 65 .. DSGE_MAX_N_BIG variables, one workgroup per draw
bool big_size(int n);
int launch_cr_big(const double* A, const double* B, const double* C, int batch, int n, int max_iter, double tol, double* T_out,
                  int32_t* status, int32_t* n_iter, hipStream_t st, int scan_mode, const double* D, int k, double* R_out);
int launch_gensys_big(const double* A, const double* B, const double* C, const double* D, int batch, int n, int k, double tol,
                      double* T_out, double* R_out, int32_t* eu_out, int32_t* status, int32_t* n_iter, hipStream_t st);
int launch_selection_big(const double* A, const double* B, const double* C, const double* D, const double* T, int batch, int n,
                         int k, double* R_out, double* resid_out, const int32_t* status, hipStream_t st);
int big_filtered_variables(const double* A, const double* Z, int z_batched, int batch, int n, int p, hipStream_t st,
                           unsigned char* idx_out, int* u_out, int* ns_out);
int launch_big_compress(const double* T, const double* R, const double* Z, int z_batched, int batch, int n, int k, int p,
                        const unsigned char* idx, int u, double* T_r, double* R_r, double* Z_r, hipStream_t st);
int launch_cr_deflated(const double* A, const double* B, const double* C, const double* D, int batch, int n, int k,
                       int max_iter, double tol, double* T_out, double* R_out, int32_t* status, int32_t* n_iter,
                       hipStream_t st, int* used, unsigned long long* colmask = nullptr, const ObsModel* skip_obs = nullptr);
// (*used = 2: the one-launch kernel ran and colmask[draw] holds the non-zero columns of T_out[draw], ~0 = not known)  // static-variable deflation + cycle reduction on the reduced system
// skip_obs (p <= 8; the one-launch kernel only): T_out and R_out are read by a filter with this observation model and by nobody
// else -- a draw none of whose deflated static variables is observed gets zeros in the static rows of T_out and R_out
// (dsge_cr_fused.hpp, phase 3).  Null: every row is computed.
void cr_deflation_reset();
void gensys_shape_reset();  // launch_gensys.hip
int launch_bdirect(const double* A, const double* B, const double* D, int batch, int n, int k, double* T_out,
                   double* R_out, hipStream_t st);
int launch_rqr(const double* R, const double* q, int q_batched, int batch, int n, int k, const int32_t* status,
               double* RQR_out, hipStream_t st, int rerun_only = 0);  // sym(R diag(q) R') alone, k <= RQR_KMAX (dsge_kernels.hpp);
                                                                      // rerun_only: draws flagged DSGE_ST_INTERNAL_RERUN
// launch_assemble.hip: the operations of assemble_kernel (dsge_kernels.hpp), each with the arguments it reads.  status (may be null):
// a draw with a non-zero word gets zero-filled outputs (resid = inf)
// selection R = -(C T + B)^-1 D, optionally the policy residual |A + (B + C T) T|_F^2 (reads A); only_marked: draws with a non-zero mark
int assemble_selection(const double* A, const double* B, const double* C, const double* D, const double* T, int batch, int n, int k,
                       double* R_out, double* resid_out, int32_t* status, hipStream_t st, const int32_t* only_marked = nullptr);
// sym(R Q R') alone; the selection and sym(R Q R') in one launch
int assemble_rqr(const double* R, const ShockCov& q, int batch, int n, int k, double* RQR_out, int32_t* status, hipStream_t st);
int assemble_selection_rqr(const double* A, const double* B, const double* C, const double* D, const double* T, const ShockCov& q,
                           int batch, int n, int k, double* R_out, double* resid_out, double* RQR_out, int32_t* status, hipStream_t st);
// sym(R Q R') (RQR_out may be null) and P0 = solve_discrete_lyapunov(T, R Q R'); a draw that does not converge: DSGE_ST_LYAP_FAIL
int assemble_rqr_p0(const double* T, const double* R, const ShockCov& q, int batch, int n, int k, double* RQR_out, double* P0_out,
                    int32_t* status, hipStream_t st);
// P0 from a stored sym(R Q R'): for every healthy draw, or for the draws flagged DSGE_ST_INTERNAL_RERUN only
int assemble_p0_from_rqr(const double* T, double* RQR, int batch, int n, double* P0_out, int32_t* status, bool flagged_only,
                         hipStream_t st);
int launch_dense_z_augment(const double* T, const double* R, const double* Z, int z_batched, int batch, int n, int k, int p,
                           double* T_aug, double* R_aug, double* Z_aug, hipStream_t st);
int launch_dense_z_deaugment(const double* Tbar_a, const double* Gbar_a, const double* T, const double* G_aug, const double* Z,
                             int z_batched, const int32_t* status, int batch, int n, int p, double* Tbar, double* Gbar,
                             double* Z_bar, hipStream_t st);
int launch_status_park(int32_t* status, int32_t* park, int batch, int restore, hipStream_t st);
int launch_adjoint(const double* B, const double* C, const double* T, const double* Tbar, int batch, int n, double* Ab,
                   double* Bb, double* Cb, int32_t* status, hipStream_t st, int accumulate = 0, int only_flag = 0);
int launch_adjoint_fused(const double* B, const double* C, const double* T, const double* R, const double* q, int q_batched,
                         const double* Gbar, double* Tbar, int batch, int n, int k, double* Ab, double* Bb, double* Cb, double* Db,
                         double* qb, int32_t* status, hipStream_t st);
int launch_norms(const double* A, const double* B, const double* C, const double* D, const double* T, const double* R,
                 const int32_t* mask, int batch, int n, int k, double* det, double* sto, hipStream_t st);
int launch_augment(const double* T, const double* R, int batch, int n, int k, int m, const int32_t* inv_var_order,
                   int n_links, const int32_t* link_rows, const int32_t* link_cols, double* T_aug, double* R_aug,
                   hipStream_t st);
int launch_acf(const double* T, const double* Sigma, const double* Z, const double* Hdiag, int batch, int m, int p,
               int n_lags, int lag_step, int correlation, double* out, const int32_t* status, hipStream_t st);
int launch_kalman(const double* T, double* RQR, double* P0, int p0_valid, const ObsModel& o, int batch, int m, int n_state_hint,
                  int z_selector_hint, double* logp, int32_t* status, hipStream_t st, const int32_t* order_key = nullptr,
                  const double* Rsel = nullptr, const ShockCov& q = ShockCov{}, int k_shocks = 0,  // R folded into the filter, see below
                  const unsigned long long* colmask = nullptr,
                  int rerun_all = 0);  // 1: every launch is a second pass -- only the draws flagged DSGE_ST_INTERNAL_RERUN are filtered
int launch_kalman_outputs(const double* T, const double* RQR, const double* P0, const ObsModel& o, int batch, int m, double* ll,
                          double* a_pred, double* a_filt, double* p_pred, double* p_filt, int full_cov, int32_t* status, hipStream_t st);
// launch_kalman_seg.hip (dsge_kalman_seg.hpp): the filter across dated breaks.  Of s: T, a0, shift, obs, seg_start and the sizes;
// RQR: [batch][S][m][m]; P0: [batch][m][m], the caller's or the chain's; ll, a_last, P_last may be null
int launch_kalman_segments(const SegmentedProblem& s, const double* RQR, const double* P0, double* logp, double* ll, double* a_last,
                           double* P_last, int32_t* status, hipStream_t st);
size_t kalman_segments_lds_bytes(int m, int p);
// dst[r][0 .. width-1] = src[(r % mod) * mul][0 .. width-1], r = 0 .. rows-1: a shared [S][width] repeated per draw (mod = S, mul = 1),
// segment 0 of every draw out of [batch][S][width] (mod = rows, mul = S)
int launch_segment_rows(double* dst, const double* src, size_t rows, int width, int mod, int mul, hipStream_t st);
// launch_smooth.hip (dsge_kalman_smooth.hpp): basis of range(P_pred) per draw (U, UT, UR: [batch] images of smoother_image_doubles(m)
// doubles, rank: [batch]) and the backward pass over the stored outputs of launch_kalman_outputs (full covariances)
size_t smoother_image_doubles(int m);
int launch_kalman_smoother(const double* T, const double* R, const ShockCov& q, int batch, int m, int k, int T_len,
                           double rank_tol, double* U, double* UT, double* UR, int32_t* rank, const double* a_pred, const double* a_filt,
                           const double* p_pred, const double* p_filt, double* a_s, double* p_s, double* e_s, int full_cov,
                           int32_t* status, hipStream_t st);
int launch_smoother_basis(const double* T, const double* R, const ShockCov& q, int batch, int m, int k, double rank_tol, double* U,
                          double* UT, double* UR, int32_t* rank, int32_t* status, hipStream_t st);  // the basis alone
size_t smoother_lds_bytes(int m);
// launch_kalman_seg_store.hip: the filter of launch_kalman_segments that also stores the moments of every period, the forward pass
// of the smoother and of the gradient across dated breaks -- logp, ll: may be null; ap_s .. pf_s: [batch][T_len][m] /
// [batch][T_len][m][m] scratch; ap_o .. pf_o: the caller's, each may be null, covariances as diagonals or full by full_cov.
// launch_smooth.hip: the bases and the backward pass of the smoother over that scratch -- T, R, U, UT, UR: [batch][S] problems; q: a
// *_BATCHED layout over batch * S; rank, status_flat: [batch * S] scratch
int launch_kalman_segments_store(const SegmentedProblem& s, const double* RQR, const double* P0, double* logp, double* ll,
                                 double* ap_s, double* af_s, double* pp_s, double* pf_s, double* ap_o, double* af_o, double* pp_o,
                                 double* pf_o, int full_cov, int32_t* status, hipStream_t st);
int launch_kalman_smoother_segments(const double* T, const double* R, const ShockCov& q, const int32_t* seg_start, int n_seg, int batch,
                                    int m, int k, int T_len, double rank_tol, double* U, double* UT, double* UR, int32_t* rank,
                                    int32_t* status_flat, const double* a_pred, const double* a_filt, const double* p_pred,
                                    const double* p_filt, double* a_s, double* p_s, double* e_s, int full_cov, int32_t* status,
                                    hipStream_t st);
// launch_kalman_seg_grad.hip (dsge_kalman_seg_grad.hpp): the gradient of the likelihood across dated breaks.  The reverse sweep over
// the scratch of launch_kalman_segments_store (of s: T, shift, obs, seg_start, the sizes, and whether P0 is the caller's; Tbar:
// [batch][S][m][m] zeroed, the caller's or scratch; Gbar: scratch; the other cotangents: the caller's, zeroed, each may be null);
// R_bar, Q_bar of the flattened batch * S from Gbar (q: a *_BATCHED layout over it), zeros and logp = -inf for a failed draw
size_t kalman_segments_grad_lds_bytes(int m, int p);
int launch_kalman_segments_grad(const SegmentedProblem& s, const double* ap, const double* af, const double* pp, const double* pf,
                                double* Tbar, double* Gbar, double* Zbar, double* dbar, double* hbar, double* shbar, double* a0bar,
                                double* P0bar, const int32_t* status, hipStream_t st);
int launch_kalman_segments_grad_rq(const double* Gbar, const double* R, const ShockCov& q, int flat, int n_seg, int m, int k,
                                   double* Rbar, double* Qbar, double* logp, const int32_t* status, hipStream_t st);
// launch_simsmooth.hip (dsge_simsmooth.hpp): the simulation smoother's forward (filter means of n_paths transformed data sets per
// draw over the stored P_pred) and backward pass (smoother means, x+ / eps+ added) for groups of 16 paths per draw.  xp, a_pred,
// a_filt: [batch][n_paths][T_len][m] (a_pred, a_filt: scratch); eps / eta: draw strides, 0 = shared; snap: [batch] scratch
int launch_simulation_smoother(const double* T, const ShockCov& q, const ObsModel& o, int batch, int m, int k, int n_paths,
                               const double* U, const double* UT, const double* UR, const int32_t* rank, const double* p_pred,
                               const double* p_filt, const double* xp, const double* eps, long long eps_draw, const double* eta,
                               long long eta_draw, double* a_pred, double* a_filt, double* x_out, double* e_out, int32_t* status,
                               int32_t* snap, hipStream_t st);
// launch_dynamics.hip (dsge_dynamics.hpp): x_t = T x_{t-1} + R e_t for groups of 16 paths per draw (shock element (draw, path,
// step, component) at the four strides; identity: unit impulses, nothing read), optionally the FEVD of <= 16 paths; the FEVD of
// more as a second pass over stored responses; the forecast moment recursion
int launch_propagate(const double* T, const double* R, const double* shocks, long long sh_draw, long long sh_path, long long sh_step,
                     long long sh_comp, int identity, const double* x0, long long x0_draw, const double* weights, long long w_draw,
                     const int32_t* status, int batch, int m, int k, int n_paths, int n_steps, int n_shock_steps, double* x_out,
                     double* fevd_out, hipStream_t st);
int launch_fevd(const double* irf, const double* weights, long long w_draw, const int32_t* status, int batch, int m, int c,
                int n_steps, double* fevd_out, hipStream_t st);
int launch_forecast(const double* T, const double* R, const ShockCov& q, const ObsModel& o, const double* a0, const double* P0,
                    const int32_t* status, int batch, int m, int k, int n_steps, double* a_out, double* p_out, int full_cov,
                    double* y_out, double* f_out, hipStream_t st);  // (of o: Z, d, Hdiag, p)
// launch_pruned.hip (dsge_pruned.hpp): the pruned second-order recursion.  One description of the problem for both entries; the
// coefficient pointers are those of the first draw of a chunk, S is a HOST index list.  panel: scratch, [batch] x pruned_panel_doubles.
// girf_out != nullptr: generalised impulse responses to the c columns of imp (nullptr: unit impulses), else the paths themselves.
struct PrunedProblem {
  const double *T, *R, *gyy, *gyu, *guu, *gss;
  const int32_t* S;
  int n, s, k, c, n_paths, n_steps, n_shock_steps;
  long long eps_draw, x0_draw, imp_draw;  // strides from one draw to the next, 0 = shared
};
size_t pruned_panel_doubles(int n, int s, int k);
int launch_pruned(const PrunedProblem& p, int batch, const double* eps, const double* xf0, const double* xs0, const double* imp,
                  const int32_t* status, double* panel, double* x_out, double* xf_out, double* xs_out, double* girf_out,
                  hipStream_t st);
// launch_shock_decomp.hip (dsge_shock_decomp.hpp): the historical shock decomposition, one workgroup per draw and pack of
// floor(16 / (n_groups + 1)) paths; grp (k entries) and var (n_out entries) are HOST index lists, already checked
size_t shock_decomp_lds_bytes(int m, int k, int p, int n_groups);
int launch_shock_decomp(const double* T, const double* R, const double* eps, const double* x, const int32_t* grp, int n_groups,
                        const int32_t* var, int n_out, const double* Z, int z_batched, const int32_t* status, int batch, int m, int k,
                        int p, int n_paths, int T_len, int remainder, double* contrib_out, double* obs_out, hipStream_t st);
// launch_condfc.hip (dsge_condfc.hpp): the conditional forecast, a setup workgroup per draw, then one workgroup per draw and
// group of 16 paths.  The sizes, flags and HOST index lists of one call; check_conditional_forecast fills t_max and n_free
struct CondFcProblem {
  int batch, m, k, p, n_paths, n_steps, n_shock_steps, n_cond;
  int x0_batched, x0_paths, eps_batched, cv_batched, cv_paths;
  const int32_t *cond_t, *cond_j, *free_shock;  // [n_cond], [n_cond], [k] or null (all free)
  double rank_tol;
  int t_max = -1, n_free = 0;
};
// bytes of the larger of the two kernels' LDS images; lags = t_max + 1
size_t condfc_lds_bytes(int m, int k, int p, int n_cond, int lags, int n_free);
int launch_condfc(const CondFcProblem& c, const double* T, const double* R, const ShockCov& q, const double* Z, int z_batched,
                  const double* d, int d_batched, const double* x0, const double* eps, const double* cond_val, int32_t* status,
                  double* chol, double* psi, double* psiq, int32_t* flag, double* x_out, double* eps_out, double* obs_out,
                  hipStream_t st);
// launch_spectral.hip (dsge_spectral.hpp): spectral densities and filtered autocovariances, a wavefront per draw and frequency
// group, then a reduction workgroup per draw.  The sizes and flags of one call
struct SpectralProblem {
  int batch, m, k, p, n_grid, n_lags, correlation, z_batched, h_batched;
  double rank_tol;
};
// bytes of the solve kernel's LDS image (the reduction's is 8 (2 n_grid + dim), at most 66 KB)
size_t spectral_lds_bytes(int m, int k, int p, int has_z);
int launch_spectral(const SpectralProblem& s, const double* T, const double* R, const ShockCov& q, const double* Z,
                    const double* Hdiag, const double* gain, int32_t* status, int32_t* flag, double* F, double* acov_out,
                    double* spectrum_out, hipStream_t st);
// launch_anticipated.hip (dsge_anticipated.hpp): paths with anticipated shocks, a setup workgroup per draw (G = -(B + C T)^-1 C),
// then one workgroup per draw and group of 16 paths.  The sizes and flags of one call
struct AnticipatedProblem {
  int batch, m, k, p, n_paths, n_steps, n_shock_steps, mode, n_lead;
  int eps_batched, x0_batched, x0_paths, z_batched, d_batched;
  double rank_tol;
};
// bytes of the larger of the two kernels' LDS images
size_t anticipated_lds_bytes(int m, int k, int p);
// G: G_out (g_is_out) or scratch [batch][m][m]; flag: scratch [batch]; park: where w_t waits for the forward pass -- w_out if
// given, else x_out, else scratch [batch][n_paths][n_steps][m]; nullptr: no path output is wanted (G alone).  phases: which of the
// two launches are made (launch_obc.hip runs the setup once and the paths kernel several times on its G and flag)
constexpr int ANT_SETUP = 1, ANT_PATHS = 2;
int launch_anticipated(const AnticipatedProblem& c, const double* B, const double* C, const double* T, const double* R,
                       const double* eps, const double* x0, const double* Z, const double* d, int32_t* status, double* G,
                       int g_is_out, int32_t* flag, double* park, double* x_out, double* w_out, double* obs_out, hipStream_t st,
                       int phases = ANT_SETUP | ANT_PATHS);
// launch_obc.hip (dsge_obc.hpp): perfect-foresight paths under an occasionally binding bound -- the two kernels above, the regime
// kernel and the gap kernel, a chain on one stream.  `a`: the sizes and flags of the paths (mode perfect foresight, n_lead 0)
struct ConstrainedProblem {
  AnticipatedProblem a;
  int c_batched, bound_batched, shock, horizon, max_iter;
};
// what the caller gave (inputs, outputs: any may be null) and the library's scratch of one call
struct ConstrainedBuffers {
  const double *B, *C, *T, *R, *eps, *x0, *Z, *d, *c_row, *bound;
  int32_t* status;
  double *x_out, *w_out, *obs_out, *nu_out, *gap_out, *Mz_out;
  int32_t *path_status_out, *iters_out;
  double* G;        // [batch][m][m]
  int32_t* flag;    // [batch]
  double* unit;     // [H][H][k]
  double* mzt;      // [batch][H][H]
  double* mzpark;   // [constrained_chunk()][H][H][m]
  double* xbuf;     // [batch][n_paths][n_steps][m]: x_out, or scratch without it
  double* eps2;     // [batch][n_paths][max(n_shock_steps, H)][k]
  double* qmax;     // [batch][n_paths]
  int32_t* pstat;   // [batch][n_paths]
};
// draws per launch of the unit paths: their parked anticipation terms, H H m doubles per draw, take at most 256 MB of scratch
int constrained_chunk(int batch, int m, int horizon);
int launch_constrained(const ConstrainedProblem& c, const ConstrainedBuffers& b, hipStream_t st);
// its first two steps alone: G, the flag and Mz (mzt) of every draw, from B, C, T, R, c_row, status, unit and mzpark of `b`
int launch_constrained_mz(const ConstrainedProblem& c, const ConstrainedBuffers& b, hipStream_t st);
// launch_obc_sim.hip (dsge_obc_sim.hpp): the stochastic simulation at the bound -- surprise shocks, the regime iteration every
// period.  `mz`: the inputs and the scratch of launch_constrained_mz (its outputs are not used); n_shock_steps <= n_steps
struct ConstrainedSimBuffers {
  ConstrainedBuffers mz;
  double *x_out, *obs_out, *gap_out, *shadow_out, *plan_out;
  int32_t *duration_out, *iters_out;
  double* Mz_out;
  int32_t *path_status_out, *fail_step_out;
  double* cq;      // [batch][H][m]
  double* wt;      // [batch][H][m]
  int32_t* pstat;  // [batch][n_paths]
};
// bytes of the simulation kernel's LDS image (R inside it where that fits LDS_LIMIT)
size_t constrained_sim_lds_bytes(int m, int k, int horizon);
int launch_constrained_sim(const ConstrainedProblem& c, const ConstrainedSimBuffers& b, hipStream_t st);
// true if launch_kalman, given the selection matrix R and a diagonal Q of k shocks (Rsel, q, k_shocks), forms sym(R Q R')[U,U] inside the
// fast filter kernel: the caller then skips the full-size product (RQR is filled for handed-on draws only).  It is `fold` of the plan
// launch_kalman executes (dsge_kalman_plan.hpp), so the two cannot disagree.
bool kalman_folds_rqr(int m, int p, int k, int n_state_hint, int z_selector_hint);
// launch_grad.hip: reverse sweep of the Kalman filter + reverse of the assembly (dsge_kalman_grad.hpp)
int launch_persistence_key(const double* T, const int32_t* status, int batch, int n, int32_t* key, hipStream_t st);
int launch_kalman_grad(const double* T, const double* RQR, const ObsModel& o, int batch, int m, int u_hint, double* store,
                       double* logp, int32_t* status, double* Tbar, double* Gbar, double* dbar, double* hbar, hipStream_t st,
                       int32_t* order_key = nullptr, int32_t* order_buf = nullptr);
size_t kalman_grad_store_doubles_per_draw(int u_hint, int m, int T_len);
int launch_grad_assemble(const double* B, const double* C, const double* T, const double* R, const double* q,
                         int q_batched, const double* Gbar, int batch, int n, int k, const int32_t* status, double* Tbar,
                         double* B_bar, double* C_bar, double* D_bar, double* q_bar, hipStream_t st,
                         const double* Rbar_in = nullptr, int only_flag = 0);  // Rbar_in: pullback of R = -(C T + B)^-1 D alone (Tbar written)
int gensys_caps(int n, int n_lead_hint, int* n_cap, int* l_cap);
// gensys by spectral division with the verdict next to the filter (round 6; launch_gensys.hip::launch_gensys_doubling)
struct GensysOverlap {
  ThreadStream* side = nullptr;   // in: the verdict's stream, forked from the caller's stream behind the iteration
  int32_t* status = nullptr;      // in: [batch] status words the verdict works on
  const int32_t* marks = nullptr; // out: [batch], non-zero = the verdict re-solved (or rejected) the draw
  int used = 0;                   // out: 1 = the verdict was forked
};
int launch_gensys_overlap_merge(int batch, const int32_t* marks, const int32_t* vstatus, int32_t* status, double* logp,
                                hipStream_t st);
int launch_gensys(const double* A, const double* B, const double* C, int batch, int n, double tol, int n_lead_hint,
                  double* T_out, int32_t* eu_out, int32_t* status, hipStream_t st, long long* dbg = nullptr,
                  int32_t* key_out = nullptr, int* key_written = nullptr,  // key_out: Kalman dispatch key from the QZ spectrum
                                                                           // (window path only: *key_written tells)
                  const double* D = nullptr, int k = 0, double* R_tmp = nullptr, int n_state_hint = 0,
                  const int32_t** qz_marks = nullptr,  // *qz_marks: [batch], non-zero = the ordered QZ solved the draw (R_tmp is not its R)
                  GensysOverlap* ov = nullptr);
// (D, k, R_tmp, n_state_hint: only for dsge_options.gensys_doubling -- with them the doubling iteration runs as the one-launch
//  deflated cycle reduction, whose final elimination needs a right-hand side; R_tmp is scratch, [batch][n][k])

int launch_gensys_pencil(const double* g0, const double* g1, const double* c, const double* psi, const double* pi, int batch,
                         int N, int k, int ell, double tol, double* G1_out, double* C_out, double* impact_out,
                         double* gev_out, int32_t* eu_out, int32_t* status, hipStream_t st,
                         const dsge_gensys_forward* fw = nullptr);

int launch_gensys_bk(const double* A, const double* B, const double* C, int batch, int n, double tol, double* eig_re,
                     double* eig_im, int32_t* n_eig, int32_t* n_forward, int32_t* n_unstable, int32_t* status,
                     hipStream_t st);

// launch_second_order.hip (dsge_second_order.hpp); S, L, U: host index lists
int launch_second_order(const double* B, const double* C, const double* T, const double* R, const int32_t* hess_idx, int nnz,
                        const double* hess_val, const double* q, int q_batched, const double* Z, const double* d,
                        const double* Hdiag, const double* y, int batch, int n, int k, int p, int T_len, double jitter,
                        double missing_fill, const int32_t* S, int s, const int32_t* L, int l, const int32_t* U, int u,
                        double* logp, int32_t* status_io, double* gyy_out, double* gyu_out, double* guu_out, double* gss_out,
                        int32_t* steady_at, int32_t* n_doublings, hipStream_t st, float* ms, const int32_t* order_key = nullptr);

extern int g_adj_refine_mode;          // launch_assemble.hip: 0 = residual rule, 1 = refine every draw, 2 = never (debug)
extern long long* g_so_dbg;            // launch_second_order.hip: debug phase counters of the second-order filter kernel
extern long long* g_pruned_dbg;        // launch_pruned.hip: debug phase counters of pruned_propagate_kernel
extern long long* g_shock_decomp_dbg;  // launch_shock_decomp.hip: debug phase counters of shock_decomp_kernel
extern long long* g_condfc_dbg;        // launch_condfc.hip: debug phase counters of the two conditional-forecast kernels
extern long long* g_cr_dbg;            // launch_solvers.hip: debug phase counters of the compact CR kernel
extern long long* g_cr_fused_dbg;      // launch_solvers.hip: debug phase counters of the fused CR kernel (stamped instance)
extern int g_cr_static_rows_mode;      // launch_solvers.hip: 0 = static rows skipped where nobody reads them, 1 = never, 2 = also into T_out / R_out (debug)
extern int g_cr_refine_mode;           // launch_solvers.hip: 0 = the refinement rule, 1 = never refine on cr_fused_kernel_occ2<5, 4> (debug, changes results)
extern long long* g_big_dbg;         // launch_big.hip: debug phase cycles of cr_big_kernel
extern long long* g_kalman_dbg;       // launch_kalman.hip: debug buffer for per-phase cycles of draw 0
extern long long* g_gensys_win_dbg;   // launch_gensys.hip: debug phase stamps of the window kernels (device int64[32])
extern float* g_gensys_stage_ms;      // launch_gensys.hip: debug, host float[8]: launch durations of the window path (dsge_debug_gensys_stage_ms)
extern long long* g_kalman_timeline;  // debug: device int64 [batch][8] {start, end, HW_ID, steady step} per draw (kalman_nt_kernel)
extern int32_t* g_kalman_steady_at;   // debug: device buffer [batch], first steady step per draw (-1 = never)

// Kernel-variant switches.  They are PER CALL: the *_opt entry points carry a dsge_options, which an RAII guard installs
// for the duration of the call on the calling thread (launching is synchronous on the host, every kernel argument is
// passed by value at launch), so two host threads -- two PyMC chains, two streams -- never see each other's settings.
// Calls without options use the compiled-in defaults (g_defaults is never written: ABI 8 removed the dsge_set_* setters).
// The fields ARE the public dsge_options (one list, include/dsge_hip.h); the constructor is the only place their defaults are
// written: dsge_options_init hands out a copy, a call with options installs a copy of the caller's struct.
struct Options : dsge_options {
  int grad_fused_adjoint = 1;  // gradient pipeline: reverse of the assembly + policy adjoints in one launch (internal; DSGE_GRAD_FUSED_ADJOINT=0 switches it off)
  Options() : dsge_options{} {   // (reserved_ stays zero)
    struct_size = (uint32_t)sizeof(dsge_options);
    cr_compact = 1;          // 0 = dense cycle-reduction kernel only
    cr_fused_selection = 1;  // fused pipeline: R from the cycle-reduction kernel's final elimination
    cr_deflation = 1;        // static-variable deflation in front of cycle reduction
    cr_two_waves = 1;        // 4 x 4-tile compact kernel built for two waves per SIMD
    n_static_hint = -1;      // static variables (zero columns of A and C): -1 = measure on the device, >= 0 caller's bound
    kalman_order = 1;        // Kalman workgroups slow-draws-first (1 = CR iteration count / persistence key, 2 = key, 0 = index)
    kalman_tiny = 1;         // thread-per-draw kernel for small models
    kalman_block = 0;        // steady tail handed to kalman_tail_kernel
    kalman_mfma = 2;         // prediction products on the FP64 matrix core: 2 = 4 x 4 x 4 blocks in the NT kernel (round 6), 1 = 16 x 16 x 4 (round 2, slower), 0 = VALU
    cr_four_waves = 1;       // n = 49..64: cr_wide_kernel (256 threads per draw) instead of cr_compact_kernel<7|8>
    cr_fused_deflation = 1;  // deflation + cycle reduction + inflation in one launch (dsge_cr_fused.hpp)
    kalman_nt_products = 1;  // selector fast path: kalman_nt_kernel (NT prediction products, 16-byte LDS loads); 0 = kalman_sel_kernel
    pipeline_chunks = 0;     // fused device call in chunks over library-owned streams
    gensys_split = 1;        // 0 = single-launch gensys kernel, 1 = window path unless small, 2 = always
    gensys_real_stage = 1;   // window path: real double-shift sweeps in front of the complex single-shift iteration
    kalman_steady_tol = 1e-14;  // steady-state switch of the fast Kalman kernel (0 = never)
    gensys_pairs = 1;        // window path: two draws per wavefront in the real double-shift sweeps (dsge_gensys_pair.hpp)
    gensys_shape_cache = 1;  // window path: capacity record measured once per model size
    gensys_direct_blocks = 1;  // window path: isolated 2 x 2 blocks triangularised in closed form in front of the complex iteration
    kalman_narrow = 1;       // fast filter: the SK = 20 instance of the 32-wide tile when the state block fits
    gensys_doubling = 1;     // gensys by spectral division: cycle reduction + certificate, ordered QZ only for uncertified draws (0: QZ for all)
    kalman_grad_split = 2;   // gradient: forward sweep by a logp kernel with record output, reverse sweep by kalman_grad_kernel<BS, true>; 2: + kalman_grad_tail_kernel
    kalman_head_draws = 0;   // fast filter: this many draws at the head of the dispatch order on the two-wavefront kernel (-1 = all)
    // conventions of the filter step (third party: pymc_extras; include/dsge_hip.h "Filter conventions")
    ll_constant = DSGE_LL_CONST_P;
    mask_d = 0;
    joseph = 1;
    jitter_F = -1.0;         // < 0: the call's `jitter` argument
    jitter_P = -1.0;
  }
};
extern const Options g_defaults;
extern thread_local const Options* t_call_options;
inline const Options& opt() { return t_call_options ? *t_call_options : g_defaults; }
// the conventions of the filter step for a call whose `jitter` argument is given: what every filter kernel receives by value
inline dsge::FilterConv filter_conv(double jitter) {
  const Options& o = opt();
  dsge::FilterConv cv;
  cv.jit_F = (o.jitter_F >= 0.0) ? o.jitter_F : jitter;
  cv.jit_P = (o.jitter_P >= 0.0) ? o.jitter_P : jitter;
  cv.jit_V = o.joseph ? cv.jit_F : 0.0;
  cv.ll_mode = o.ll_constant;
  cv.mask_d = o.mask_d ? 1 : 0;
  return cv;
}
// what every kernel of the family across dated breaks reads of the problem, into its argument struct (KsegArgs, KsegStoreArgs,
// KsegGradArgs): the list of starts padded with 0x7fffffff, as kseg_start reads it
template <typename A>
void fill_segment_args(A& a, const SegmentedProblem& s) {
  const ObsModel& o = s.obs;
  a.T = s.T; a.shift = s.shift; a.Z = o.Z; a.d = o.d; a.Hdiag = o.Hdiag; a.y = o.y;
  a.batch = s.batch; a.m = s.m; a.p = o.p; a.T_len = o.T_len; a.n_seg = s.n_seg;
  a.z_batched = o.z_batched; a.d_batched = o.d_batched; a.h_batched = o.h_batched;
  for (int i = 0; i < DSGE_MAX_SEGMENTS; ++i) a.seg_start[i] = i < s.n_seg ? s.seg_start[i] : 0x7fffffff;
  a.cv = filter_conv(o.jitter);
  a.missing_fill = o.missing_fill;
}

// ---- Argument checks, each written ONCE for a device entry (dsge_api.hip) and its host twin (api_host.hip): both run them before
// their first HIP call and so report the same code and message.  `others`: no required pointer outside the two aggregates is null.
inline int check_common(int batch, int n, int n_max) {
  if (batch < 0) return fail(DSGE_ERR_INVALID, "batch < 0");
  if (n < 1 || n > n_max) return fail(DSGE_ERR_INVALID, "n out of range (1.." + std::to_string(n_max) + ")");
  return DSGE_SUCCESS;
}
// a filter call on a model of m <= m_max variables (`dim`: 'm' or 'n' in the messages) with 1 <= p <= p_max; `family` prefixes the
// messages of an entry with caps of its own
inline int check_filter(const char* family, int batch, int m, int m_max, char dim, int k, const ObsModel& o, int p_max,
                        const ShockCov& q, bool others) {
  const std::string pre = family;
  int rc = check_common(batch, m, m_max);
  if (rc) return rc;
  if (k < 1 || k > m) return fail(DSGE_ERR_INVALID, std::string("k out of range (1..") + dim + ")");
  if (o.p < 1 || o.p > p_max)
    return fail(DSGE_ERR_INVALID, pre + "p out of range (1.." + (p_max == DSGE_MAX_P ? "DSGE_MAX_P" : std::to_string(p_max)) + ")");
  if (o.T_len < 0) return fail(DSGE_ERR_INVALID, "T_len < 0");
  if (q.mode < 0 || q.mode > 3) return fail(DSGE_ERR_INVALID, pre.empty() ? "bad q_mode" : pre + "q_batched is a DSGE_Q_* mode (0..3)");
  if (!others || !q.Q || !o.Z || !o.y) return fail(DSGE_ERR_INVALID, "null pointer");
  return DSGE_SUCCESS;
}
inline int check_kalman(int batch, int m, int k, const ObsModel& o, const ShockCov& q, bool others) {
  return check_filter("", batch, m, DSGE_MAX_N, 'm', k, o, DSGE_MAX_P, q, others);
}
inline int check_smoother(int batch, int m, int k, const ObsModel& o, const ShockCov& q, bool others, bool any_output) {
  int rc = check_kalman(batch, m, k, o, q, others);
  if (rc) return rc;
  return any_output ? DSGE_SUCCESS : fail(DSGE_ERR_INVALID, "no smoothed output requested");
}
// the likelihood across dated breaks: the sizes first (DSGE_ERR_TOO_LARGE), then the filter's own checks, then the HOST list of
// segment starts -- n_seg in 1 .. DSGE_MAX_SEGMENTS, seg_start[0] == 0, strictly increasing, every entry < T_len (when T_len > 0)
inline int check_kalman_segments(int batch, int m, int k, const ObsModel& o, const ShockCov& q, const int32_t* seg_start, int n_seg,
                                 bool others) {
  if (m > DSGE_MAX_N || o.p > DSGE_MAX_P)
    return fail(DSGE_ERR_TOO_LARGE, "segmented filter: m exceeds DSGE_MAX_N or p exceeds DSGE_MAX_P");
  int rc = check_kalman(batch, m, k, o, q, others && seg_start);
  if (rc) return rc;
  if (n_seg < 1 || n_seg > DSGE_MAX_SEGMENTS) return fail(DSGE_ERR_INVALID, "n_seg out of range (1..DSGE_MAX_SEGMENTS)");
  if (seg_start[0] != 0) return fail(DSGE_ERR_INVALID, "seg_start[0] must be 0");
  for (int s = 1; s < n_seg; ++s)
    if (seg_start[s] <= seg_start[s - 1]) return fail(DSGE_ERR_INVALID, "seg_start must be strictly increasing");
  if (o.T_len > 0 && seg_start[n_seg - 1] >= o.T_len) return fail(DSGE_ERR_INVALID, "seg_start: every entry must be < T_len");
  return DSGE_SUCCESS;
}
inline int check_smoother_segments(int batch, int m, int k, const ObsModel& o, const ShockCov& q, const int32_t* seg_start, int n_seg,
                                   bool others, bool any_output) {
  int rc = check_kalman_segments(batch, m, k, o, q, seg_start, n_seg, others);
  if (rc) return rc;
  return any_output ? DSGE_SUCCESS : fail(DSGE_ERR_INVALID, "no output requested");
}
inline int check_simulation_smoother(int batch, int m, int k, const ObsModel& o, const ShockCov& q, bool others, int n_paths,
                                     const double* eps, const double* eta, bool any_output) {
  if (m > DSGE_MAX_N || o.p > DSGE_MAX_P)
    return fail(DSGE_ERR_TOO_LARGE, "simulation smoother: m exceeds DSGE_MAX_N or p exceeds DSGE_MAX_P");
  int rc = check_kalman(batch, m, k, o, q, others);
  if (rc) return rc;
  if (n_paths < 0) return fail(DSGE_ERR_INVALID, "n_paths < 0");
  if (eta && !o.Hdiag) return fail(DSGE_ERR_INVALID, "eta given without Hdiag");
  if (!eps && n_paths > 0 && o.T_len > 0) return fail(DSGE_ERR_INVALID, "null pointer");
  return any_output ? DSGE_SUCCESS : fail(DSGE_ERR_INVALID, "no output requested");
}
inline int check_pipeline(int batch, int n, int k, const ObsModel& o, const ShockCov& q, int solver, bool others) {
  solver &= ~DSGE_SOLVER_FLAG_ZERO_T_ON_FAILURE;
  const bool is_cr = solver == DSGE_SOLVER_CYCLE_REDUCTION || solver == DSGE_SOLVER_SCAN_CYCLE_REDUCTION;
  // (gensys beyond 64 variables exists by spectral division only: dsge_options.gensys_doubling != 0)
  const bool big_ok = is_cr || (solver == DSGE_SOLVER_GENSYS && opt().gensys_doubling != 0);
  int rc = check_filter("", batch, n, big_ok ? DSGE_MAX_N_BIG : DSGE_MAX_N, 'n', k, o, DSGE_MAX_P, q, others);
  if (rc) return rc;
  if (!is_cr && solver != DSGE_SOLVER_BACKWARD_DIRECT && solver != DSGE_SOLVER_GENSYS) return fail(DSGE_ERR_INVALID, "unknown solver code");
  return DSGE_SUCCESS;
}
inline int check_augmented(int batch, int n, int k, const ObsModel& o, const ShockCov& q, int solver, int m, int n_links, bool others) {
  const bool is_cr = solver == DSGE_SOLVER_CYCLE_REDUCTION || solver == DSGE_SOLVER_SCAN_CYCLE_REDUCTION;
  int rc = check_common(batch, n, is_cr ? DSGE_MAX_N_CR : DSGE_MAX_N);
  if (rc) return rc;
  if (m < n || m > DSGE_MAX_N_BIG) return fail(DSGE_ERR_INVALID, "augmented state dimension m out of range (n..DSGE_MAX_N_BIG)");
  if (n_links < 0) return fail(DSGE_ERR_INVALID, "n_links < 0");
  if ((rc = check_filter("", batch, n, DSGE_MAX_N, 'n', k, o, DSGE_MAX_P, q, others))) return rc;
  if (!is_cr && solver != DSGE_SOLVER_BACKWARD_DIRECT && solver != DSGE_SOLVER_GENSYS) return fail(DSGE_ERR_INVALID, "unknown solver code");
  return DSGE_SUCCESS;
}
inline int check_grad(int batch, int n, int k, const ObsModel& o, const ShockCov& q, int solver, bool dense_z, bool others) {
  int rc = check_common(batch, n, 56);
  if (rc) return rc;
  if (dense_z && n + o.p > 56) return fail(DSGE_ERR_INVALID, "gradient path with a dense design matrix: n + p must not exceed 56");
  if ((rc = check_filter("gradient path: ", batch, n, 56, 'n', k, o, 8, q, others))) return rc;
  if (solver != DSGE_SOLVER_CYCLE_REDUCTION && solver != DSGE_SOLVER_GENSYS && solver != DSGE_SOLVER_SCAN_CYCLE_REDUCTION)
    return fail(DSGE_ERR_INVALID, "gradient path: solver must be cycle_reduction, scan_cycle_reduction or gensys");
  return DSGE_SUCCESS;
}
// (S, L, U: the state / lead / retained index lists, host arrays in the entry and in its twin)
inline int check_second_order(int batch, int n, int k, const ObsModel& o, const ShockCov& q, int solver, int nnz, const int32_t* S, int s,
                              const int32_t* L, int l, const int32_t* U, int u, bool others) {
  if (nnz < 0) return fail(DSGE_ERR_INVALID, "nnz < 0");
  int rc = check_filter("second order: ", batch, n, DSGE_MAX_N_CR, 'n', k, o, 8, q, others && S && U && (l <= 0 || L));
  if (rc) return rc;
  if (s < 1 || s > 24) return fail(DSGE_ERR_INVALID, "second order: n_state out of range (1..24)");
  if (l < 0 || l > n || u < s || u > n) return fail(DSGE_ERR_INVALID, "second order: n_lead / n_ret out of range");
  // (the limits of launch_second_order, here as well: a refused call must not have run the first-order solver into status_out,
  //  T_out and R_out.  The set-up kernel's LDS limit alone stays with the launcher, which owns the layout)
  if (u > 40 || k > 12 || k > s) return fail(DSGE_ERR_INVALID, "second order: sizes out of range (s <= u <= 40, k <= min(s, 12))");
  if (2 * u + s * (s + 1) / 2 > 208) return fail(DSGE_ERR_INVALID, "second order: pruned state 2 u + s (s + 1) / 2 exceeds 208");
  if (solver != DSGE_SOLVER_CYCLE_REDUCTION && solver != DSGE_SOLVER_GENSYS)
    return fail(DSGE_ERR_INVALID, "second order: solver must be cycle reduction or gensys");
  for (int i = 0; i < s; ++i)
    if (S[i] < 0 || S[i] >= n) return fail(DSGE_ERR_INVALID, "state_idx out of range");
  for (int i = 0; i < l; ++i)
    if (L[i] < 0 || L[i] >= n) return fail(DSGE_ERR_INVALID, "lead_idx out of range");
  for (int i = 0; i < u; ++i)
    if (U[i] < 0 || U[i] >= n) return fail(DSGE_ERR_INVALID, "ret_idx out of range");
  for (int i = 0; i < s; ++i)
    if (U[i] != S[i]) return fail(DSGE_ERR_INVALID, "second order: the retained variables must list the states first");
  return DSGE_SUCCESS;
}
// the dynamics entries (DSGE_ERR_TOO_LARGE: a well-formed call beyond a capacity)
inline int check_simulate(const double* T, const double* R, const double* eps, int batch, int m, int k, int n_paths, int n_steps,
                          int n_shock_steps, const double* x_out) {
  if (batch < 0 || m < 1 || n_paths < 0 || n_steps < 0 || n_shock_steps < 0) return fail(DSGE_ERR_INVALID, "size out of range");
  if (k < 1 || k > m) return fail(DSGE_ERR_INVALID, "k out of range (1..m)");
  if (n_shock_steps > n_steps) return fail(DSGE_ERR_INVALID, "n_shock_steps > n_steps");
  if (!T || !R || !x_out || (!eps && n_shock_steps > 0)) return fail(DSGE_ERR_INVALID, "null pointer");
  if (m > DSGE_MAX_N_BIG) return fail(DSGE_ERR_TOO_LARGE, "simulate: m exceeds DSGE_MAX_N_BIG");
  return DSGE_SUCCESS;
}
inline int check_irf(const double* T, const double* R, const double* S, int batch, int m, int k, int c, int n_steps,
                     const double* irf_out, const double* fevd_out) {
  if (batch < 0 || m < 1 || c < 0 || n_steps < 0) return fail(DSGE_ERR_INVALID, "size out of range");
  if (k < 1 || k > m) return fail(DSGE_ERR_INVALID, "k out of range (1..m)");
  if (!S && c != k) return fail(DSGE_ERR_INVALID, "S == NULL means S = I: c must equal k");
  if (!T || !R) return fail(DSGE_ERR_INVALID, "null pointer");
  if (!irf_out && !fevd_out) return fail(DSGE_ERR_INVALID, "no output requested");
  if (m > DSGE_MAX_N_BIG) return fail(DSGE_ERR_TOO_LARGE, "impulse responses: m exceeds DSGE_MAX_N_BIG");
  return DSGE_SUCCESS;
}
// the second-order dynamics entries: sizes of the second-order solver (n <= 64, 1 <= s <= 24, k <= 12; k <= s is not required)
inline int check_pruned(const double* T, const double* R, const double* gyy, const double* gyu, const double* guu, const double* gss,
                        const int32_t* S, int s, const double* eps, int batch, int n, int k, int n_paths, int n_steps,
                        int n_shock_steps, bool any_output) {
  if (batch < 0 || n < 1 || s < 1 || k < 1 || n_paths < 0 || n_steps < 0 || n_shock_steps < 0)
    return fail(DSGE_ERR_INVALID, "size out of range");
  if (n_shock_steps > n_steps) return fail(DSGE_ERR_INVALID, "n_shock_steps > n_steps");
  if (!T || !R || !gyy || !gyu || !guu || !gss || !S || (!eps && n_shock_steps > 0)) return fail(DSGE_ERR_INVALID, "null pointer");
  if (!any_output) return fail(DSGE_ERR_INVALID, "no output requested");
  if (n > 64 || s > 24 || k > 12)
    return fail(DSGE_ERR_TOO_LARGE, "pruned dynamics: beyond the second-order solver's sizes (n <= 64, n_state <= 24, k <= 12)");
  if (s > n) return fail(DSGE_ERR_INVALID, "n_state exceeds n");
  for (int i = 0; i < s; ++i)
    if (S[i] < 0 || S[i] >= n || (i > 0 && S[i] <= S[i - 1])) return fail(DSGE_ERR_INVALID, "state_idx must be strictly ascending within 0 .. n-1");
  return DSGE_SUCCESS;
}
// (girf: n_paths baseline paths, at least one; eps == nullptr: baselines without shocks)
inline int check_girf_pruned(const double* T, const double* R, const double* gyy, const double* gyu, const double* guu, const double* gss,
                             const int32_t* S, int s, const double* S_imp, int c, const double* eps, int batch, int n, int k, int n_paths,
                             int n_steps, int n_shock_steps, const double* girf_out) {
  if (c < 0 || n_paths < 1) return fail(DSGE_ERR_INVALID, "size out of range");
  if (!S_imp && c != k) return fail(DSGE_ERR_INVALID, "S_imp == NULL means S_imp = I: c must equal k");
  return check_pruned(T, R, gyy, gyu, guu, gss, S, s, eps, batch, n, k, n_paths, n_steps, n_shock_steps, girf_out != nullptr);
}
// (p: the rows of Z, ignored without Z)
inline int check_shock_decomp(const double* T, const double* R, const double* eps, const double* x, const int32_t* grp, int g,
                              const int32_t* var, int n_out, const double* Z, int batch, int m, int k, int p, int n_paths, int T_len,
                              int remainder, const double* contrib_out, const double* obs_out) {
  if (batch < 0 || m < 1 || n_paths < 0 || T_len < 1 || g < 1 || n_out < 0) return fail(DSGE_ERR_INVALID, "size out of range");
  if (k < 1 || k > m) return fail(DSGE_ERR_INVALID, "k out of range (1..m)");
  if (!T || !R || !x || (!eps && T_len > 1)) return fail(DSGE_ERR_INVALID, "null pointer");
  if (!contrib_out && !obs_out) return fail(DSGE_ERR_INVALID, "no output requested");
  if (obs_out && !Z) return fail(DSGE_ERR_INVALID, "obs_out needs Z");
  if (Z && p < 1) return fail(DSGE_ERR_INVALID, "Z given with p < 1");
  if (m > DSGE_MAX_N_BIG) return fail(DSGE_ERR_TOO_LARGE, "shock decomposition: m exceeds DSGE_MAX_N_BIG");
  if (g > 15) return fail(DSGE_ERR_TOO_LARGE, "shock decomposition: more than 15 groups (group the shocks: one tile holds 16 columns)");
  if (Z && p > DSGE_MAX_P) return fail(DSGE_ERR_TOO_LARGE, "shock decomposition: p exceeds DSGE_MAX_P");
  if (g > k) return fail(DSGE_ERR_INVALID, "n_groups exceeds k");
  if (!grp && g != k) return fail(DSGE_ERR_INVALID, "group_of_shock == NULL means one group per shock: n_groups must equal k");
  if (contrib_out && (n_out < 1 || n_out > m)) return fail(DSGE_ERR_INVALID, "n_out out of range (1..m)");
  if (contrib_out && !var && n_out != m) return fail(DSGE_ERR_INVALID, "var_idx == NULL means all variables: n_out must equal m");
  if (grp) {
    bool used[16] = {};
    for (int j = 0; j < k; ++j) {
      if (grp[j] < 0 || grp[j] >= g) return fail(DSGE_ERR_INVALID, "group_of_shock out of range (0..n_groups-1)");
      used[grp[j]] = true;
    }
    for (int c = 0; c < g; ++c)
      if (!used[c]) return fail(DSGE_ERR_INVALID, "group_of_shock: every group must hold a shock");
  }
  if (var && contrib_out) {
    bool seen[DSGE_MAX_N_BIG] = {};
    for (int i = 0; i < n_out; ++i) {
      if (var[i] < 0 || var[i] >= m) return fail(DSGE_ERR_INVALID, "var_idx out of range (0..m-1)");
      if (seen[var[i]]) return fail(DSGE_ERR_INVALID, "var_idx holds a variable twice");
      seen[var[i]] = true;
    }
  }
  if (shock_decomp_lds_bytes(m, k, Z ? p : 0, g) > LDS_LIMIT)
    return fail(DSGE_ERR_TOO_LARGE, "shock decomposition: [T | R] does not fit the LDS (m = 96 takes k <= 32)");
  return DSGE_SUCCESS;
}

// the conditional forecast: every refusal, before any device is touched; fills c.t_max and c.n_free
inline int check_conditional_forecast(CondFcProblem& c, const double* T, const double* R, const ShockCov& q, const double* Z,
                                      const double* x0, const double* eps, const double* cond_val, const double* x_out,
                                      const double* eps_out, const double* obs_out) {
  if (c.batch < 0 || c.m < 1 || c.p < 1 || c.n_cond < 0 || c.n_shock_steps < 0) return fail(DSGE_ERR_INVALID, "size out of range");
  if (c.n_steps < 1 || c.n_paths < 1) return fail(DSGE_ERR_INVALID, "conditional forecast: n_steps and n_paths must be >= 1");
  if (c.k < 1 || c.k > c.m) return fail(DSGE_ERR_INVALID, "k out of range (1..m)");
  if (eps && c.n_shock_steps > c.n_steps) return fail(DSGE_ERR_INVALID, "n_shock_steps > n_steps");
  if (q.mode < DSGE_Q_DIAG_SHARED || q.mode > DSGE_Q_FULL_BATCHED) return fail(DSGE_ERR_INVALID, "q_mode out of range");
  if (!T || !R || !q.Q || !Z || !x0) return fail(DSGE_ERR_INVALID, "null pointer");
  if (c.n_cond > 0 && (!c.cond_t || !c.cond_j || !cond_val)) return fail(DSGE_ERR_INVALID, "null pointer (conditions)");
  if (!x_out && !eps_out && !obs_out) return fail(DSGE_ERR_INVALID, "no output requested");
  if (c.m > DSGE_MAX_N_BIG) return fail(DSGE_ERR_TOO_LARGE, "conditional forecast: m exceeds DSGE_MAX_N_BIG");
  if (c.p > DSGE_MAX_P) return fail(DSGE_ERR_TOO_LARGE, "conditional forecast: p exceeds DSGE_MAX_P");
  if (c.n_cond > 64) return fail(DSGE_ERR_TOO_LARGE, "conditional forecast: more than 64 conditions");
  c.t_max = -1;
  for (int i = 0; i < c.n_cond; ++i) {
    const int t = c.cond_t[i], j = c.cond_j[i];
    if (t < 0 || t >= c.n_steps) return fail(DSGE_ERR_INVALID, "cond_t out of range (0..n_steps-1)");
    if (j < 0 || j >= c.p) return fail(DSGE_ERR_INVALID, "cond_j out of range (0..p-1)");
    if (i > 0 && (t < c.cond_t[i - 1] || (t == c.cond_t[i - 1] && j <= c.cond_j[i - 1])))
      return fail(DSGE_ERR_INVALID, "the conditions must be strictly ascending in (t, j)");
    c.t_max = t;
  }
  c.n_free = 0;
  for (int j = 0; j < c.k; ++j) c.n_free += !c.free_shock || c.free_shock[j] != 0;
  if (c.n_cond > 0 && c.n_free == 0) return fail(DSGE_ERR_INVALID, "conditional forecast: conditions but no free shock");
  if (condfc_lds_bytes(c.m, c.k, c.p, c.n_cond, c.t_max + 1, c.n_free) > LDS_LIMIT)
    return fail(DSGE_ERR_TOO_LARGE, "conditional forecast: the LDS image exceeds 160 KB (docs/design/conditional_forecast.md)");
  return DSGE_SUCCESS;
}

// the spectral moments: every refusal, before any device is touched
inline int check_spectral_moments(const SpectralProblem& s, const double* T, const double* R, const ShockCov& q, const double* Z,
                                  const double* Hdiag, const double* acov_out, const double* spectrum_out) {
  if (s.batch < 0 || s.m < 1) return fail(DSGE_ERR_INVALID, "size out of range");
  if (s.n_grid < 4 || s.n_grid > DSGE_SPECTRAL_MAX_GRID || (s.n_grid & 1))
    return fail(DSGE_ERR_INVALID, "spectral moments: n_grid must be even and within 4 .. 4096");
  if (s.n_lags < 0 || s.n_lags > s.n_grid / 2) return fail(DSGE_ERR_INVALID, "spectral moments: n_lags out of range (0 .. n_grid / 2)");
  if (s.k < 1 || s.k > s.m) return fail(DSGE_ERR_INVALID, "k out of range (1..m)");
  if (q.mode < DSGE_Q_DIAG_SHARED || q.mode > DSGE_Q_FULL_BATCHED) return fail(DSGE_ERR_INVALID, "q_mode out of range");
  if (!T || !R || !q.Q) return fail(DSGE_ERR_INVALID, "null pointer");
  if (Hdiag && !Z) return fail(DSGE_ERR_INVALID, "spectral moments: Hdiag without Z");
  if (Z && s.p < 1) return fail(DSGE_ERR_INVALID, "spectral moments: p must be >= 1 with Z");
  if (!acov_out && !spectrum_out) return fail(DSGE_ERR_INVALID, "no output requested");
  if (s.m > DSGE_MAX_N) return fail(DSGE_ERR_TOO_LARGE, "spectral moments: m exceeds DSGE_MAX_N");
  if (s.k > DSGE_SPECTRAL_MAX_K) return fail(DSGE_ERR_TOO_LARGE, "spectral moments: k exceeds DSGE_SPECTRAL_MAX_K");
  if (Z && s.p > DSGE_SPECTRAL_MAX_P) return fail(DSGE_ERR_TOO_LARGE, "spectral moments: p exceeds DSGE_SPECTRAL_MAX_P");
  if (spectral_lds_bytes(s.m, s.k, s.p, Z != nullptr) > LDS_LIMIT)
    return fail(DSGE_ERR_TOO_LARGE, "spectral moments: the LDS image exceeds 160 KB (docs/design/spectral_moments.md)");
  return DSGE_SUCCESS;
}

// the anticipated-shock paths: every refusal, before any device is touched
inline int check_anticipated_paths(const AnticipatedProblem& c, const double* B, const double* C, const double* T, const double* R,
                                   const double* eps, const double* Z, const double* x_out, const double* w_out,
                                   const double* obs_out, const double* G_out) {
  if (c.batch < 0 || c.m < 1 || c.p < 0 || c.n_paths < 0 || c.n_steps < 0 || c.n_shock_steps < 0)
    return fail(DSGE_ERR_INVALID, "size out of range");
  if (c.k < 1 || c.k > c.m) return fail(DSGE_ERR_INVALID, "k out of range (1..m)");
  if (c.mode != DSGE_ANT_PERFECT_FORESIGHT && c.mode != DSGE_ANT_NEWS) return fail(DSGE_ERR_INVALID, "anticipated paths: mode out of range");
  if (c.n_lead < 0) return fail(DSGE_ERR_INVALID, "anticipated paths: n_lead < 0");
  if (c.mode == DSGE_ANT_PERFECT_FORESIGHT && c.n_lead != 0)
    return fail(DSGE_ERR_INVALID, "anticipated paths: n_lead must be 0 with perfect foresight");
  if (c.mode == DSGE_ANT_NEWS && c.n_shock_steps > c.n_steps) return fail(DSGE_ERR_INVALID, "news: n_shock_steps > n_steps");
  if (!B || !C || !T || !R || (!eps && c.n_shock_steps > 0)) return fail(DSGE_ERR_INVALID, "null pointer");
  if (!x_out && !w_out && !obs_out && !G_out) return fail(DSGE_ERR_INVALID, "no output requested");
  if (c.p > 0 && !Z) return fail(DSGE_ERR_INVALID, "p > 0 without Z");
  if (obs_out && c.p == 0) return fail(DSGE_ERR_INVALID, "obs_out requested with p == 0");
  if (c.m > DSGE_MAX_N) return fail(DSGE_ERR_TOO_LARGE, "anticipated paths: n exceeds DSGE_MAX_N (65 .. 96 variables are out of scope)");
  if (c.p > DSGE_MAX_P) return fail(DSGE_ERR_TOO_LARGE, "anticipated paths: p exceeds DSGE_MAX_P");
  if (c.n_lead > DSGE_ANT_MAX_LEAD) return fail(DSGE_ERR_TOO_LARGE, "anticipated paths: n_lead exceeds DSGE_ANT_MAX_LEAD");
  if ((long long)c.n_shock_steps * (c.n_lead + 1) > 0x7fffffffLL / c.k)
    return fail(DSGE_ERR_TOO_LARGE, "anticipated paths: n_shock_steps (n_lead + 1) k exceeds 2^31 - 1");
  if (anticipated_lds_bytes(c.m, c.k, c.p) > LDS_LIMIT)
    return fail(DSGE_ERR_TOO_LARGE, "anticipated paths: the LDS image exceeds 160 KB (docs/design/anticipated_shocks.md)");
  return DSGE_SUCCESS;
}

// the paths under an occasionally binding bound: every refusal of the anticipated-shock paths (with one observation row more: the
// unit paths observe c'x), then its own, before any device is touched.  `other`: non-null if an output besides x, w and observed
// is wanted.  n_steps == 0 is the empty call, whatever the horizon
inline int check_constrained_paths(const ConstrainedProblem& c, const double* B, const double* C, const double* T, const double* R,
                                   const double* eps, const double* Z, const double* c_row, const double* bound, const double* x_out,
                                   const double* w_out, const double* obs_out, const void* other) {
  if (int rc = check_anticipated_paths(c.a, B, C, T, R, eps, Z, x_out, w_out, obs_out, (const double*)other)) return rc;
  if (!c_row || !bound) return fail(DSGE_ERR_INVALID, "null pointer");
  if (c.horizon < 1 || c.horizon > DSGE_OBC_MAX_HORIZON)
    return fail(DSGE_ERR_INVALID, "constrained paths: horizon out of range (1..DSGE_OBC_MAX_HORIZON)");
  if (c.a.n_steps > 0 && c.horizon > c.a.n_steps) return fail(DSGE_ERR_INVALID, "constrained paths: horizon > n_steps");
  if (c.shock < 0 || c.shock >= c.a.k) return fail(DSGE_ERR_INVALID, "constrained paths: shock out of range (0..k-1)");
  if (anticipated_lds_bytes(c.a.m, c.a.k, c.a.p > 1 ? c.a.p : 1) > LDS_LIMIT)
    return fail(DSGE_ERR_TOO_LARGE, "constrained paths: the LDS image exceeds 160 KB (docs/design/occasionally_binding.md)");
  return DSGE_SUCCESS;
}

// the stochastic simulation at the bound: the refusals of check_constrained_paths less horizon <= n_steps (a plan may look beyond
// the simulated periods), plus shocks beyond the last period.  `other`: non-null if an output besides x and observed is wanted
inline int check_constrained_simulate(const ConstrainedProblem& c, const double* B, const double* C, const double* T, const double* R,
                                      const double* eps, const double* Z, const double* c_row, const double* bound,
                                      const double* x_out, const double* obs_out, const void* other) {
  if (int rc = check_anticipated_paths(c.a, B, C, T, R, eps, Z, x_out, nullptr, obs_out, (const double*)other)) return rc;
  if (!c_row || !bound) return fail(DSGE_ERR_INVALID, "null pointer");
  if (c.horizon < 1 || c.horizon > DSGE_OBC_MAX_HORIZON)
    return fail(DSGE_ERR_INVALID, "constrained simulation: horizon out of range (1..DSGE_OBC_MAX_HORIZON)");
  if (c.shock < 0 || c.shock >= c.a.k) return fail(DSGE_ERR_INVALID, "constrained simulation: shock out of range (0..k-1)");
  if (anticipated_lds_bytes(c.a.m, c.a.k, c.a.p > 1 ? c.a.p : 1) > LDS_LIMIT || constrained_sim_lds_bytes(c.a.m, c.a.k, c.horizon) > LDS_LIMIT)
    return fail(DSGE_ERR_TOO_LARGE, "constrained simulation: the LDS image exceeds 160 KB (docs/design/stochastic_bound.md)");
  if (c.a.n_shock_steps > c.a.n_steps) return fail(DSGE_ERR_INVALID, "constrained simulation: n_shock_steps > n_steps");
  return DSGE_SUCCESS;
}

inline int check_forecast(const double* T, const double* R, const ShockCov& q, const ObsModel& o, const double* a0, int batch, int m,
                          int k, int n_steps, const double* a_out, const double* p_out, const double* y_out, const double* f_out) {
  const int p = o.p;
  if (batch < 0 || m < 1 || p < 0 || n_steps < 0) return fail(DSGE_ERR_INVALID, "size out of range");
  if (k < 1 || k > m) return fail(DSGE_ERR_INVALID, "k out of range (1..m)");
  if (q.mode < 0 || q.mode > 3) return fail(DSGE_ERR_INVALID, "bad q_mode");
  if (!a_out && !p_out && !y_out && !f_out) return fail(DSGE_ERR_INVALID, "no output requested");
  if (!T || !R || !a0 || ((p_out || f_out) && !q.Q) || (p > 0 && !o.Z)) return fail(DSGE_ERR_INVALID, "null pointer");
  if ((y_out || f_out) && p == 0) return fail(DSGE_ERR_INVALID, "observation outputs requested with p == 0");
  if (m > DSGE_MAX_N || p > DSGE_MAX_P) return fail(DSGE_ERR_TOO_LARGE, "forecast: m exceeds DSGE_MAX_N or p exceeds DSGE_MAX_P");
  return DSGE_SUCCESS;
}

}  // namespace dsge_host
